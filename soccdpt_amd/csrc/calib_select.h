// The decision procedure of soccdpt_prec_calibrate, host-only (standard library; no HIP, no Handle): given what each group costs in each operand
// format and a callback that measures a candidate map, pick the cheapest map whose measured errors pass.  calibrate.cpp supplies the GPU-backed
// callback; tests/calib_select_main.cpp a synthetic one (tests/test_calib_select_cpu.py), which is how the failure and fall-back paths are reached.
#pragma once
#include <cstddef>
#include <functional>
#include <vector>

namespace soccdpt {
namespace calib {

constexpr int kL2 = 7;        // the relative-L2 quantities (calibrate.h kCalibQuantities)
constexpr int NQ = kL2 + 1;   // + the optional per-pixel constraint as an eighth, scaled so that the same budget applies

// one measured forward: the NQ errors over the calibration frames (e) and, separately, over the held-out frames (h)
struct Err {
    double e[NQ] = {0, 0, 0, 0, 0, 0, 0, 0};
    double h[NQ] = {0, 0, 0, 0, 0, 0, 0, 0};
    double p999 = 0, pmax = 0, h_p999 = 0, h_pmax = 0;   // per-pixel relative error of the inverse depth (only when measured)
    double worst() const;
    double worst_l2() const;
    double worst_holdout() const;
    double worst_holdout_l2() const;
};

// a map = one state per group: 0 fp16, 1 x2w (fp16 activations, x3 weight pairs), 2 x3
typedef std::vector<int> Map;

struct Problem {
    int G = 0;
    std::vector<double> cost_x2w, cost_x3;   // device time of the group's state over fp16, microseconds
    std::vector<char> x2w_ok;                // may the group take state 1?
    Map shipped;                             // the shipped map of the backbone
    double budget = 0, headroom = 0;         // calibration frames are held to headroom x budget, held-out frames to the budget
    int holdout = 0;                         // number of held-out frames (0: no hold-out rule)
    double cost(int i, int state) const { return state == 0 ? 0.0 : (state == 2 ? cost_x3[i] : cost_x2w[i]); }
    double cost_of(const Map& m) const;
};

// the forward under the map and its errors against the reference (want_pixels: also the per-pixel percentiles) -> 0, or non-zero on failure
typedef std::function<int(const Map&, Err&, bool want_pixels)> Measure;

struct Selection {
    Map chosen;
    Err e_final, e_ship, e_f16, e_x3;   // the chosen map (its last measured run), the shipped map, every group fp16, every group x3
};

// -> 0 and `out`; 1 as soon as a measure call fails (no further call is made).  The last successful call measured out.chosen.
int select(const Problem& p, const Measure& measure, Selection& out);

// |got - ref| / max(|ref|, 1e-6) over n values (a NaN counts as 3e38): its 99.9th percentile (torch.kthvalue(int(0.999 n))) and maximum.
// `work` holds n floats.
void per_pixel(const float* ref, const float* got, size_t n, float* work, double& p999, double& pmax);

}  // namespace calib
}  // namespace soccdpt
