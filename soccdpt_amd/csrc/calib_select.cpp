// soccdpt_prec_calibrate's selection: one-group-out variances, greedy selection by variance removed per microsecond, measured prune (calib_select.h).
#include "calib_select.h"

#include <algorithm>
#include <cmath>

namespace soccdpt {
namespace calib {

double Err::worst() const { double w = 0; for (double v : e) w = std::max(w, v); return w; }
double Err::worst_l2() const { double w = 0; for (int q = 0; q < kL2; ++q) w = std::max(w, e[q]); return w; }
double Err::worst_holdout() const { double w = 0; for (double v : h) w = std::max(w, v); return w; }
double Err::worst_holdout_l2() const { double w = 0; for (int q = 0; q < kL2; ++q) w = std::max(w, h[q]); return w; }

double Problem::cost_of(const Map& m) const { double c = 0; for (int i = 0; i < G; ++i) c += cost(i, m[i]); return c; }

namespace {

// the additive error model: the all-x3 floor plus, per group, T = the variance the group adds in fp16 and A = what it still adds as x2w (its activation rounding)
struct Additive {
    const Problem& p;
    Err e_x3;
    std::vector<Err> T, A;

    int down(const Map& m, int i) const { return (m[i] == 2 && p.x2w_ok[i]) ? 1 : 0; }   // one level cheaper
    double rem(int i, int state, int q) const { return state == 2 ? 0.0 : (state == 1 ? A[i].e[q] : T[i].e[q]); }
    void predict(const Map& m, Err& out) const {
        for (int q = 0; q < NQ; ++q) {
            double v = e_x3.e[q] * e_x3.e[q];
            for (int i = 0; i < p.G; ++i) v += rem(i, m[i], q);
            out.e[q] = std::sqrt(v);
        }
    }
    Map solve(double target) const {
        const int G = p.G;
        Map m(G, 0);
        for (;;) {   // greedy over single-group upgrades (fp16 -> x2w, fp16 -> x3, x2w -> x3) by violated variance removed per microsecond
            Err e;
            predict(m, e);
            bool viol = false;
            for (double v : e.e) viol |= v > target;
            if (!viol) break;
            int best = -1, best_to = 0;
            double best_rate = 0;
            for (int i = 0; i < G; ++i)
                for (int to = m[i] + 1; to <= 2; ++to) {
                    if (to == 1 && !p.x2w_ok[i]) continue;
                    double gain = 0;
                    for (int q = 0; q < NQ; ++q)
                        if (e.e[q] > target) gain += std::min(rem(i, m[i], q) - rem(i, to, q), std::max(0.0, e.e[q] * e.e[q] - target * target));
                    const double dc = std::max(p.cost(i, to) - p.cost(i, m[i]), 0.25);
                    if (gain > 0 && (best < 0 || gain / dc > best_rate)) { best = i; best_to = to; best_rate = gain / dc; }
                }
            if (best < 0) break;
            m[best] = best_to;
        }
        // predicted prune: single-level demotions, largest saving first, while the prediction stays under the target
        for (bool changed = true; changed;) {
            changed = false;
            int bi = -1;
            double bsave = 0;
            for (int i = 0; i < G; ++i) {
                if (!m[i]) continue;
                const int to = down(m, i);
                Map t = m;
                t[i] = to;
                Err e;
                predict(t, e);
                const double save = p.cost(i, m[i]) - p.cost(i, to);
                if (e.worst() <= target && save > bsave) { bi = i; bsave = save; }
            }
            if (bi >= 0) { m[bi] = down(m, bi); changed = true; }
        }
        return m;
    }
};

}  // namespace

int select(const Problem& p, const Measure& measure, Selection& out) {
    const int G = p.G;
    const double hb = p.headroom * p.budget;   // what the calibration frames are held to
    auto accept = [&](const Err& e) { return e.worst() <= hb && (p.holdout == 0 || e.worst_holdout() <= p.budget); };
    Err &e_x3 = out.e_x3, &e_f16 = out.e_f16, &e_ship = out.e_ship;

    // ---- the corner cases and the shipped map on these weights ----
    const Map all3(G, 2), all16(G, 0);
    if (measure(all3, e_x3, true) || measure(all16, e_f16, true)) return 1;
    if (measure(p.shipped, e_ship, false)) return 1;
    if (e_x3.worst() > hb) {   // even every group in x3 misses the target (the fp16 attention core, or a budget under the f32 noise floor): nothing to select
        out.chosen = all3;
        return measure(all3, out.e_final, true) ? 1 : 0;
    }

    // ---- one-group-out variances ----
    Additive model{p, e_x3, std::vector<Err>(G), std::vector<Err>(G)};
    std::vector<Err>&T = model.T, &A = model.A;
    for (int i = 0; i < G; ++i) {
        Map m = all3;
        Err e;
        m[i] = 0;
        if (measure(m, e, false)) return 1;
        for (int q = 0; q < NQ; ++q) T[i].e[q] = std::max(e.e[q] * e.e[q] - e_x3.e[q] * e_x3.e[q], 0.0);
        A[i] = T[i];
        if (p.x2w_ok[i]) {
            m[i] = 1;
            if (measure(m, e, false)) return 1;
            for (int q = 0; q < NQ; ++q) A[i].e[q] = std::min(T[i].e[q], std::max(e.e[q] * e.e[q] - e_x3.e[q] * e_x3.e[q], 0.0));
        }
    }

    // ---- greedy selection, checked by a measured run: the calibration frames must come in under headroom x budget AND the held-out frames under
    // the budget itself; the additive model is within a few per cent, so tighten and repeat when it was optimistic ----
    Map chosen = all3;
    double target = hb * 0.97;
    for (int attempt = 0; attempt < 6; ++attempt) {
        Map cand = model.solve(target);
        Err e;
        if (measure(cand, e, false)) return 1;
        if (accept(e)) { chosen = cand; break; }
        target *= 0.9;
    }
    // ---- measured prune: demote one group by one level at a time, largest saving first, keeping every demotion the acceptance rule still passes ----
    {
        std::vector<int> order;
        for (int i = 0; i < G; ++i) if (chosen[i]) order.push_back(i);
        auto saving = [&](int i) { return p.cost(i, chosen[i]) - p.cost(i, model.down(chosen, i)); };
        std::sort(order.begin(), order.end(), [&](int a, int b) { return saving(a) > saving(b); });
        for (int i : order) {
            if (saving(i) < 1.0) continue;   // nothing to win
            Map t = chosen;
            t[i] = model.down(chosen, i);
            Err e;
            if (measure(t, e, false)) return 1;
            if (accept(e)) chosen = t;
        }
    }
    // the shipped map wins when it passes the same rule on these weights at no higher cost (keeps the tested default where it is valid)
    if (accept(e_ship) && p.cost_of(p.shipped) <= p.cost_of(chosen)) chosen = p.shipped;
    out.chosen = chosen;
    return measure(chosen, out.e_final, true) ? 1 : 0;   // leaves the handle prepared for the chosen map
}

void per_pixel(const float* ref, const float* got, size_t n, float* work, double& p999, double& pmax) {
    p999 = pmax = 0;
    if (n == 0) return;
    for (size_t i = 0; i < n; ++i) {
        const float r = ref[i], d = got[i];
        const float v = std::fabs(d - r) / std::max(std::fabs(r), 1e-6f);
        work[i] = v == v ? v : 3.0e38f;   // a NaN counts as the worst error
    }
    const size_t k = std::min(n - 1, (size_t)std::max<long long>(0, (long long)(0.999 * (double)n) - 1));   // torch.kthvalue(int(0.999 n)) of bench.py / tests
    std::nth_element(work, work + k, work + n);
    p999 = work[k];
    pmax = *std::max_element(work + k, work + n);
}

}  // namespace calib
}  // namespace soccdpt
