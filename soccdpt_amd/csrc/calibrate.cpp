// soccdpt_prec_calibrate: the precision map of a SOCCDPT_PREC_MIXED handle derived on the weights bound to it, inside the library.
//
// What it stands in for: the reference computes in fp32 whatever checkpoint BaseModel.load_net binds (/root/reference/SOccDPT/model/base_model.py:5-37,
// model/SOccDPT.py:29-57,634-636, model/loader.py:126-139); the mixed arithmetic is only a drop-in for THAT when its per-site operand formats keep
// the outputs within the tolerance on THOSE weights.  Round 4 shipped maps fitted by an out-of-tree script to one synthetic draw; this is the same
// procedure (one-group-out variances, greedy selection by variance removed per microsecond, measured prune) behind the C ABI, with the library's
// own exact-f32 arithmetic on the same weights as the reference.  Nothing here touches the CPU oracle.
//
// This file drives the GPU (the f32 twin, one prepare + forward per candidate map, error read-back, restore on failure, fingerprint); which maps to
// try and which to keep is decided in calib_select.cpp, which knows nothing of HIP and is tested on the CPU (tests/test_calib_select_cpu.py).
#include "calibrate.h"

#include <cmath>
#include <cstring>
#include <functional>

#include "calib_select.h"
#include "prec_cost_table.h"

namespace soccdpt {

namespace {

const char* const kQuant[kCalibQuantities] = {"feat0", "feat1", "feat2", "feat3", "path1", "inv", "seg_logits"};

struct QuantGeo { size_t off[kCalibQuantities]; size_t n[kCalibQuantities]; size_t total; size_t biggest; };

// compact f32 sizes of the seven quantities at batch B
int quant_geometry(Handle& h, int B, QuantGeo& g, std::string& err) {
    g.total = 0; g.biggest = 0;
    for (int q = 0; q < kCalibQuantities; ++q) {
        size_t n;
        if (q == 5) n = (size_t)B * h.img * h.img;
        else {
            size_t off, el; int kind, H, W, C;
            if (model_workspace_tensor(h, B, kQuant[q], &off, &el, &kind, &H, &W, &C)) { err = std::string("soccdpt_prec_calibrate: no workspace tensor ") + kQuant[q]; return 1; }
            n = (size_t)B * H * W * C;
        }
        g.off[q] = g.total; g.n[q] = n;
        g.total += (n + 63) / 64 * 64;
        g.biggest = std::max(g.biggest, n);
    }
    return 0;
}

struct Scratch {
    char* twin_prepared; size_t twin_prepared_bytes;
    char* twin_ws; size_t twin_ws_bytes;
    float* ref;        // seven reference tensors, compact f32
    float* tmp;        // one decoded tensor
    float* inv; float* seg;   // network outputs of the run being measured
    double* partial; double* out2;
    unsigned long long* fp;
    size_t total;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

int lay_scratch(Handle& h, Handle* twin, int B, const QuantGeo& g, char* base, Scratch& s) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    s.twin_prepared_bytes = twin ? twin->prepared_bytes : 0;
    s.twin_ws_bytes = twin ? model_workspace_bytes(*twin, B) : 0;
    s.twin_prepared = take(s.twin_prepared_bytes);
    s.twin_ws = take(s.twin_ws_bytes);
    s.ref = reinterpret_cast<float*>(take(g.total * 4));
    s.tmp = reinterpret_cast<float*>(take(g.biggest * 4));
    s.inv = reinterpret_cast<float*>(take((size_t)B * h.img * h.img * 4));
    s.seg = reinterpret_cast<float*>(take((size_t)B * h.img * h.img * h.cfg.num_classes * 4));
    s.partial = reinterpret_cast<double*>(take((size_t)kCalibPartialBlocks * 2 * 8));
    s.out2 = reinterpret_cast<double*>(take(kCalibQuantities * 4 * 8));   // {sum d^2, sum ref^2} x 7 over the calibration frames, then x 7 over the held-out frames
    s.fp = reinterpret_cast<unsigned long long*>(take(8));
    s.total = o;
    return 0;
}

Handle* make_twin(const Handle& h, std::string& err) {
    Handle* t = new Handle();
    t->cfg = h.cfg;
    t->cfg.precision = SOCCDPT_PREC_F32;
    t->device = h.device;
    t->mlp_fuse_max = h.mlp_fuse_max;
    if (model_init(*t, err)) { delete t; return nullptr; }
    if (t->weights.size() != h.weights.size()) { err = "soccdpt_prec_calibrate: weight lists differ"; delete t; return nullptr; }
    for (size_t i = 0; i < h.weights.size(); ++i) t->weights[i].ptr = h.weights[i].ptr;
    return t;
}

// decode the seven quantities of the forward that just ran on `hh` (workspace ws, output inv) into dst[q] (q-th slot of a QuantGeo layout), or compare
int extract(Handle& hh, int B, const char* ws, const float* inv, const QuantGeo& g, int q, float* dst, hipStream_t st, std::string& err) {
    if (q == 5) return launch_calib_decode(inv, 0, B, hh.img, hh.img, 1, dst, st, err);
    size_t off, el; int kind, H, W, C;
    if (model_workspace_tensor(hh, B, kQuant[q], &off, &el, &kind, &H, &W, &C)) { err = std::string("soccdpt_prec_calibrate: no workspace tensor ") + kQuant[q]; return 1; }
    return launch_calib_decode(ws + off, kind, B, H, W, C, dst, st, err);
}

}  // namespace

size_t calib_scratch_bytes(Handle& h, int B) {
    if (h.cfg.precision != SOCCDPT_PREC_MIXED || B <= 0) return 0;
    std::string err;
    Handle* t = make_twin(h, err);
    if (!t) return 0;
    QuantGeo g;
    Scratch s;
    size_t bytes = 0;
    if (!quant_geometry(h, B, g, err) && !lay_scratch(h, t, B, g, nullptr, s)) bytes = s.total + 256;
    delete t;
    return bytes;
}

// sum over four tensors of (2 i + 1) x (64-bit sum of the tensor's f32 bit patterns): tells one checkpoint from another (not a hash of everything:
// four tensors spread over decoder, heads and encoder).  -> 0 and *out, 1 when one of the tensors is not bound, < 0 on error
int calib_fingerprint(Handle& h, unsigned long long* tmp, hipStream_t st, unsigned long long* out, std::string& err) {
    const ModelP& P = h.params;
    const PRef refs[4] = {P.layer_rn[0], P.refine[0].out_conv.w, P.seg.c0_w, h.arch.hybrid ? P.hy.vit[0].qkv.w : P.swin.blk[0][0].qkv_w};
    if (hipMemsetAsync(tmp, 0, 8, st) != hipSuccess) { err = "soccdpt_prepare: fingerprint memset failed"; return -1; }
    for (int i = 0; i < 4; ++i) {
        if (!h.W(refs[i])) return 1;   // not bound, or a backbone without this tensor
        const WeightSlot& w = h.weights[refs[i].i];
        if (launch_calib_fingerprint(w.ptr, w.numel(), (unsigned long long)(2 * i + 1), tmp, st, err)) return -1;
    }
    unsigned long long got = 0;
    if (hipMemcpyAsync(&got, tmp, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { err = "soccdpt_prepare: fingerprint read-back failed"; return -1; }
    *out = got;
    return 0;
}

int calib_weights_are_the_shipped_draw(Handle& h, unsigned long long* tmp, hipStream_t st, std::string& err) {
    // the constants are those of soccdpt_amd/utils/synth.py synth_state_dict(backbone, salt = 0), the draw tools/precision_map.py derived the shipped maps on
    unsigned long long want = 0;
    switch (h.cfg.backbone) {
        case SOCCDPT_BACKBONE_SWIN2T16_256: want = 0x1a63bad6fc751bull; break;
        case SOCCDPT_BACKBONE_SWIN2B24_384: want = 0x1c0e44312bb69eull; break;
        case SOCCDPT_BACKBONE_VITB_RN50_384: want = 0x77b3b69d1638caull; break;
        default: return 0;   // SOCCDPT_BACKBONE_SWIN2L24_384, _SWINL12_384: no shipped map, so no weights are its draw
    }
    unsigned long long got = 0;
    const int rc = calib_fingerprint(h, tmp, st, &got, err);
    if (rc < 0) return -1;
    if (rc > 0) return 0;
    return got == want ? 1 : 0;
}

namespace {

using calib::Err;
using calib::Map;
static_assert(calib::kL2 == kCalibQuantities, "calib_select.h and calibrate.h count the same quantities");

// a state of the selection (0 fp16, 1 x2w, 2 x3) <-> a Handle::prec_map code (absent = fp16, 4 = x2w, 3 = x3)
int state_to_code(int state) { return state == 2 ? 3 : 4; }   // state != 0
int code_to_state(int code) { return code == 3 ? 2 : (code == 4 ? 1 : 0); }

// The measure callback of calib::select: one forward of `h` under a map and its errors against the reference held in `s.ref` -- relative L2 of the seven
// quantities (+ the optional per-pixel constraint as an eighth, scaled so that the same budget applies) over the calibration frames [0, Bc) and,
// separately, over the held-out frames [Bc, B).
struct Measurer {
    // what it works on: one member per type, so the initialiser list cannot swap two of them unnoticed
    Handle& h;
    const std::vector<std::string>& groups;
    const Scratch& s;
    const QuantGeo& g;
    std::string& err;
    // the rest is set by name (calib_run)
    const float* x = nullptr;
    int B = 0, Bc = 0, V = 0;
    float budget = 0.f;
    double pp_budget = 0.0;
    void* prepared = nullptr; size_t prepared_bytes = 0;
    void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t st = nullptr;
    std::vector<float> ref_inv, got_inv, pix_err;   // the inverse depth on the host: the per-pixel percentiles are taken there (exact selection, 0.5 - 1.2 M values)
    int forwards = 0;
    bool touched = false;   // has the handle's map been replaced?

    int operator()(const Map& m, Err& out, bool want_pixels) {
        const size_t npix = (size_t)B * h.img * h.img, pix_frame = (size_t)h.img * h.img;
        touched = true;
        h.prec_map.clear();
        for (size_t i = 0; i < groups.size(); ++i)
            if (m[i]) h.prec_map[groups[i]] = state_to_code(m[i]);
        h.ws_key = Handle::WsKey();
        h.is_prepared = false;
        if (model_prepare(h, prepared, prepared_bytes, st, err)) return 1;
        if (model_network(h, x, B, s.inv, s.seg, ws, ws_bytes, st, err)) return 1;
        for (int q = 0; q < kCalibQuantities; ++q) {
            if (extract(h, B, static_cast<const char*>(ws), s.inv, g, q, s.tmp, st, err)) return 1;
            const size_t nf = g.n[q] / (size_t)B;
            if (launch_calib_sqdiff(s.tmp, s.ref + g.off[q], nf * Bc, s.partial, s.out2 + 2 * q, st, err)) return 1;
            if (V > 0 && launch_calib_sqdiff(s.tmp + nf * Bc, s.ref + g.off[q] + nf * Bc, nf * V, s.partial, s.out2 + 2 * (kCalibQuantities + q), st, err)) return 1;
            if (q == 5 && (want_pixels || pp_budget > 0) && hipMemcpyAsync(got_inv.data(), s.tmp, npix * 4, hipMemcpyDeviceToHost, st) != hipSuccess) {
                err = "soccdpt_prec_calibrate: read-back of the inverse depth failed";
                return 1;
            }
        }
        double host[4 * kCalibQuantities];
        if (hipMemcpyAsync(host, s.out2, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
            err = "soccdpt_prec_calibrate: a calibration forward failed";
            return 1;
        }
        out = Err();
        for (int q = 0; q < kCalibQuantities; ++q) {
            out.e[q] = host[2 * q + 1] > 0 ? std::sqrt(host[2 * q] / host[2 * q + 1]) : 0.0;
            if (V > 0) { const double* hh = host + 2 * (kCalibQuantities + q); out.h[q] = hh[1] > 0 ? std::sqrt(hh[0] / hh[1]) : 0.0; }
        }
        if (want_pixels || pp_budget > 0) {
            const size_t split = (size_t)Bc * pix_frame;
            calib::per_pixel(ref_inv.data(), got_inv.data(), split, pix_err.data(), out.p999, out.pmax);
            calib::per_pixel(ref_inv.data() + split, got_inv.data() + split, npix - split, pix_err.data(), out.h_p999, out.h_pmax);
            if (pp_budget > 0) { out.e[kCalibQuantities] = out.p999 * budget / pp_budget; out.h[kCalibQuantities] = out.h_p999 * budget / pp_budget; }
        }
        ++forwards;
        return 0;
    }
};

int count_state(const Map& m, int state) { int n = 0; for (int v : m) n += v == state; return n; }

void fill_report(soccdpt_calib_report* rep, const calib::Problem& p, const calib::Selection& sel, int forwards, int Bc, float budget, double pp_budget) {
    if (!rep) return;
    const Map& chosen = sel.chosen;
    const Map& shipped = p.shipped;
    const Err &e_final = sel.e_final, &e_ship = sel.e_ship, &e_f16 = sel.e_f16, &e_x3 = sel.e_x3;
    const int V = p.holdout;
    memset(rep, 0, sizeof(*rep));
    rep->n_groups = p.G; rep->n_x3 = count_state(chosen, 2); rep->n_x2w = count_state(chosen, 1); rep->n_x3_shipped = count_state(shipped, 2); rep->n_x2w_shipped = count_state(shipped, 1);
    rep->forwards = forwards;
    rep->met_budget = e_final.worst() <= budget ? 1 : 0; rep->shipped_met_budget = e_ship.worst() <= budget ? 1 : 0; rep->budget = budget;
    rep->worst_calibrated = (float)e_final.worst_l2(); rep->worst_shipped = (float)e_ship.worst_l2(); rep->worst_all_fp16 = (float)e_f16.worst_l2(); rep->worst_all_x3 = (float)e_x3.worst_l2();
    for (int q = 0; q < kCalibQuantities; ++q) { rep->err_calibrated[q] = (float)e_final.e[q]; rep->err_shipped[q] = (float)e_ship.e[q]; rep->err_holdout[q] = (float)e_final.h[q]; }
    rep->cost_us_calibrated = (float)p.cost_of(chosen); rep->cost_us_shipped = (float)p.cost_of(shipped);
    rep->calib_frames = Bc; rep->holdout_frames = V; rep->headroom = (float)p.headroom;
    rep->met_headroom = e_final.worst() <= p.headroom * p.budget ? 1 : 0;
    rep->met_holdout = V > 0 ? (e_final.worst_holdout() <= (double)budget ? 1 : 0) : -1;
    rep->worst_holdout = (float)e_final.worst_holdout_l2(); rep->worst_holdout_shipped = (float)e_ship.worst_holdout_l2();
    rep->per_pixel_budget = (float)pp_budget;
    rep->inv_p999_calibrated = (float)e_final.p999; rep->inv_max_calibrated = (float)e_final.pmax;
    rep->inv_p999_holdout = (float)e_final.h_p999; rep->inv_max_holdout = (float)e_final.h_pmax;
    rep->inv_p999_all_fp16 = (float)e_f16.p999; rep->inv_p999_all_x3 = (float)e_x3.p999;
}

}  // namespace

int calib_run(Handle& h, const float* x, int B, const soccdpt_calib_options& opt, void* prepared, size_t prepared_bytes, void* ws, size_t ws_bytes, void* scratch,
              size_t scratch_bytes, soccdpt_calib_report* rep, hipStream_t st, std::string& err) {
    const float budget = opt.budget;
    const int V = opt.holdout, Bc = B - V;                                     // frames [0, Bc) select the map, frames [Bc, B) only verify it
    const double headroom = opt.headroom > 0.f ? (double)opt.headroom : 0.85;   // internal target on the calibration frames = headroom x budget
    const double pp_budget = opt.per_pixel_p999 > 0.f ? (double)opt.per_pixel_p999 : 0.0;
    if (h.cfg.precision != SOCCDPT_PREC_MIXED) { err = "soccdpt_prec_calibrate: the handle was not created with SOCCDPT_PREC_MIXED"; return 1; }
    if (!x || B <= 0 || !(budget > 0.f) || !prepared || !ws || !scratch) { err = "soccdpt_prec_calibrate: bad argument"; return 1; }
    if (V < 0 || Bc < 1 || !(headroom > 0.0 && headroom <= 1.0)) { err = "soccdpt_prec_calibrate: holdout must leave at least one calibration frame, headroom must be in (0, 1]"; return 1; }
    if (h.n_streams != 1 || h.use_graph) { err = "soccdpt_prec_calibrate: calibrate on one stream without graph replay (soccdpt_set_streams(1), soccdpt_set_graph(0))"; return 1; }
    for (const auto& w : h.weights)
        if (!w.ptr) { err = "soccdpt_prec_calibrate: weight not bound: " + w.key; return 1; }
    if (prepared_bytes < h.prepared_bytes || ws_bytes < model_workspace_bytes(h, B)) { err = "soccdpt_prec_calibrate: prepared arena or workspace too small"; return 1; }
    Handle* twin = make_twin(h, err);
    if (!twin) return 1;
    QuantGeo g;
    Scratch s;
    if (quant_geometry(h, B, g, err) || lay_scratch(h, twin, B, g, static_cast<char*>(scratch), s)) { delete twin; return 1; }
    if (s.total > scratch_bytes) { delete twin; err = "soccdpt_prec_calibrate: scratch too small (soccdpt_prec_calibrate_scratch_bytes)"; return 1; }

    const std::vector<std::string> groups = model_prec_groups(h);
    Measurer measure{h, groups, s, g, err};
    measure.x = x; measure.B = B; measure.Bc = Bc; measure.V = V;
    measure.budget = budget; measure.pp_budget = pp_budget;
    measure.prepared = prepared; measure.prepared_bytes = prepared_bytes;
    measure.ws = ws; measure.ws_bytes = ws_bytes;
    measure.st = st;

    // ---- the reference: exact-f32 arithmetic on the same weights and frames ----
    int rc = model_prepare(*twin, s.twin_prepared, s.twin_prepared_bytes, st, err);
    if (!rc) rc = model_network(*twin, x, B, s.inv, s.seg, s.twin_ws, s.twin_ws_bytes, st, err);
    for (int q = 0; q < kCalibQuantities && !rc; ++q) rc = extract(*twin, B, s.twin_ws, s.inv, g, q, s.ref + g.off[q], st, err);
    const size_t npix = (size_t)B * h.img * h.img;
    if (!rc) {
        measure.ref_inv.resize(npix); measure.got_inv.resize(npix); measure.pix_err.resize(npix);
        if (hipMemcpyAsync(measure.ref_inv.data(), s.ref + g.off[5], npix * 4, hipMemcpyDeviceToHost, st) != hipSuccess) { err = "soccdpt_prec_calibrate: reference read-back failed"; rc = 1; }
    }
    if (!rc && hipStreamSynchronize(st) != hipSuccess) { err = "soccdpt_prec_calibrate: the f32 reference run failed"; rc = 1; }
    delete twin;
    if (rc) return 1;
    ++measure.forwards;

    // the handle as it was handed over: every failure below puts it back (a failed launch used to leave a half-built map, unprepared)
    const std::unordered_map<std::string, int> map_on_entry = h.prec_map;
    const int source_on_entry = h.prec_source;

    // ---- the selection problem: what each group costs over fp16 (compiled-in table, prec_cost_table.h), which may take x2w, and the shipped map ----
    calib::Problem p;
    p.G = (int)groups.size();
    p.budget = (double)budget; p.headroom = headroom; p.holdout = V;
    p.shipped.assign(p.G, 0);
    model_prec_default(h);
    for (int i = 0; i < p.G; ++i) {
        p.cost_x3.push_back((double)prec_cost_us(h.cfg.backbone, groups[i].c_str()));
        p.cost_x2w.push_back((double)prec_cost_x2w_us(h.cfg.backbone, groups[i].c_str()));
        p.x2w_ok.push_back(model_prec_x2w_ok(groups[i]) ? 1 : 0);
        auto it = h.prec_map.find(groups[i]);
        if (it != h.prec_map.end()) p.shipped[i] = code_to_state(it->second);
    }
    h.prec_map = map_on_entry;

    calib::Selection sel;
    rc = calib::select(p, std::ref(measure), sel);   // the last measured run leaves the handle prepared for the chosen map
    if (rc && measure.touched) {   // put the handle back as it was handed over, prepared again if that still works (its own error is not the one reported)
        h.prec_map = map_on_entry;
        h.prec_source = source_on_entry;
        h.ws_key = Handle::WsKey();
        h.is_prepared = false;
        model_drop_graph(h);
        std::string e2;
        (void)model_prepare(h, prepared, prepared_bytes, st, e2);
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (!rc) {
        h.prec_source = 1;
        model_drop_graph(h);
        fill_report(rep, p, sel, measure.forwards, Bc, budget, pp_budget);
        // what the map was derived on: soccdpt_prepare compares it and falls back to all-x3 when other weights have been bound or loaded since
        unsigned long long fp = 0;
        h.calib_fp_valid = calib_fingerprint(h, s.fp, st, &fp, err) == 0;
        h.calib_fp = fp;
    }
    return rc;
}

}  // namespace soccdpt
