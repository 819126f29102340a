// Stand-alone driver of soccdpt_amd/csrc/calib_select.cpp for tests/test_calib_select_cpu.py (host compiler, address + undefined sanitizers): the
// selection of soccdpt_prec_calibrate against a synthetic error model instead of GPU forwards.
//
//   calib_select_main select G=12 seed=1 factor=1 fail_at=-1 floor=5e-5 no_x2w=0 shipped=x3|best
//   calib_select_main pixels FILE N        FILE = N float32 reference values, then N float32 measured values
//
// The model: group i adds the variance t[i][q] to quantity q in fp16, a[i][q] <= t[i][q] as x2w and nothing in x3, over the floor e_x3; the error is
// sqrt(floor^2 + sum) and, when more than one group is below x3, `factor` times that (the non-additivity the tightened attempts exist for).  The
// held-out frames see 1.05 x the calibration frames' error.  Call `fail_at` (0-based) of measure fails.  One JSON line goes to stdout.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../soccdpt_amd/csrc/calib_select.h"

using namespace soccdpt::calib;

namespace {

struct Model {
    Problem p;
    std::vector<double> t, a;   // [G][NQ]
    double floor = 0, factor = 1;
    int fail_at = -1;
    std::vector<std::string> calls;   // every map handed to measure ('0' / '1' / '2' per group, then 'p' when pixels were wanted)

    double err(const Map& m, int q) const {
        double v = floor * floor;
        int below = 0;
        for (int i = 0; i < p.G; ++i) {
            below += m[i] != 2;
            v += m[i] == 0 ? t[i * NQ + q] : (m[i] == 1 ? a[i * NQ + q] : 0.0);
        }
        return std::sqrt(v) * (below > 1 ? factor : 1.0);
    }
    bool passes(const Map& m) const {   // the acceptance rule on the model's own errors
        for (int q = 0; q < NQ; ++q)
            if (err(m, q) > p.headroom * p.budget || 1.05 * err(m, q) > p.budget) return false;
        return true;
    }
    int measure(const Map& m, Err& out, bool want_pixels) {
        std::string s;
        for (int v : m) s += (char)('0' + v);
        if (want_pixels) s += 'p';
        calls.push_back(s);
        if ((int)calls.size() - 1 == fail_at) return 7;
        out = Err();
        for (int q = 0; q < NQ; ++q) { out.e[q] = err(m, q); out.h[q] = 1.05 * out.e[q]; }
        return 0;
    }
};

std::string text(const Map& m) { std::string s; for (int v : m) s += (char)('0' + v); return s; }

// the cheapest map the model accepts, by exhaustive search (3^G maps: small G only)
Map cheapest_passing(const Model& md) {
    const int G = md.p.G;
    Map m(G, 0), best(G, 2);
    double best_cost = md.p.cost_of(best);
    for (;;) {
        const double c = md.p.cost_of(m);
        if (c < best_cost && md.passes(m)) { best = m; best_cost = c; }
        int i = 0;
        while (i < G && m[i] == 2) m[i++] = 0;
        if (i == G) break;
        if (++m[i] == 1 && !md.p.x2w_ok[i]) m[i] = 2;
    }
    return best;
}

int run_select(const std::map<std::string, std::string>& arg) {
    auto num = [&](const char* k, double dflt) { auto it = arg.find(k); return it == arg.end() ? dflt : atof(it->second.c_str()); };
    const int G = (int)num("G", 12);
    if (G < 1 || G > 4096) { fprintf(stderr, "G out of range\n"); return 2; }
    std::mt19937_64 rng((unsigned long long)num("seed", 1));
    auto uni = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };   // [0, 1)
    Model md;
    Problem& p = md.p;
    p.G = G; p.budget = 5e-4; p.headroom = 0.85; p.holdout = 1;
    md.floor = num("floor", 5e-5); md.factor = num("factor", 1.0); md.fail_at = (int)num("fail_at", -1);
    const bool no_x2w = num("no_x2w", 0) != 0;
    md.t.resize((size_t)G * NQ); md.a.resize((size_t)G * NQ);
    for (int i = 0; i < G; ++i) {
        const double scale = 4e-6 / G * uni() * uni();   // every group in fp16: about 1e-3, twice the budget
        for (int q = 0; q < NQ; ++q) {
            md.t[i * NQ + q] = scale * uni();
            md.a[i * NQ + q] = md.t[i * NQ + q] * uni() * 0.6;
        }
        p.cost_x3.push_back(4.0 + 26.0 * uni());
        p.cost_x2w.push_back(p.cost_x3[i] * (0.3 + 0.4 * uni()));
        p.x2w_ok.push_back(!no_x2w && i % 5 != 4);
    }
    p.shipped.assign(G, 2);
    auto sh = arg.find("shipped");
    if (sh != arg.end() && sh->second == "best") p.shipped = cheapest_passing(md);

    Selection sel;
    const int rc = select(p, [&](const Map& m, Err& e, bool px) { return md.measure(m, e, px); }, sel);

    std::string ok;
    for (char c : p.x2w_ok) ok += c ? '1' : '0';
    printf("{\"rc\": %d, \"G\": %d, \"x2w_ok\": \"%s\", \"shipped\": \"%s\", \"hb\": %.17g, \"budget\": %.17g, \"calls\": [", rc, G, ok.c_str(), text(p.shipped).c_str(),
           p.headroom * p.budget, p.budget);
    for (size_t i = 0; i < md.calls.size(); ++i) printf("%s\"%s\"", i ? ", " : "", md.calls[i].c_str());
    printf("]");
    if (rc == 0)
        printf(", \"chosen\": \"%s\", \"final_worst\": %.17g, \"final_holdout\": %.17g, \"worst_x3\": %.17g, \"worst_f16\": %.17g, \"worst_shipped\": %.17g, "
               "\"cost_chosen\": %.17g, \"cost_shipped\": %.17g",
               text(sel.chosen).c_str(), sel.e_final.worst(), sel.e_final.worst_holdout(), sel.e_x3.worst(), sel.e_f16.worst(), sel.e_ship.worst(),
               p.cost_of(sel.chosen), p.cost_of(p.shipped));
    printf("}\n");
    return 0;
}

int run_pixels(const char* path, size_t n) {
    std::vector<float> ref(n), got(n), work(n);
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return 2; }
    const bool ok = n == 0 || (fread(ref.data(), 4, n, f) == n && fread(got.data(), 4, n, f) == n);
    fclose(f);
    if (!ok) { fprintf(stderr, "%s: short read\n", path); return 2; }
    double p999 = -1, pmax = -1;
    per_pixel(ref.data(), got.data(), n, work.data(), p999, pmax);
    printf("{\"n\": %zu, \"p999\": %.17g, \"pmax\": %.17g}\n", n, p999, pmax);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "pixels")) return run_pixels(argv[2], (size_t)strtoull(argv[3], nullptr, 10));
    if (argc >= 2 && !strcmp(argv[1], "select")) {
        std::map<std::string, std::string> arg;
        for (int i = 2; i < argc; ++i) {
            const char* eq = strchr(argv[i], '=');
            if (!eq) { fprintf(stderr, "expected key=value: %s\n", argv[i]); return 2; }
            arg[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
        }
        return run_select(arg);
    }
    fprintf(stderr, "usage: %s select key=value... | pixels FILE N\n", argv[0]);
    return 2;
}
