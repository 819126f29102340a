// soccdpt_op_train_aux (include/soccdpt_hip.h: tests): one of the training step's non-GEMM launchers of train.hip / train_hybrid.hip -- or the step's own
// composition of a few of them -- on caller-supplied tensors.  No kernel lives here: every launch goes through the tr_* / th_* launcher the step calls, in the
// order train_step.cpp / train_hybrid_step.cpp call them.  aux_plan() checks the arguments and sizes the scratch for both entry points, so a call that is
// refused has launched nothing.
#include <cstdint>

#include "train_internal.h"

namespace soccdpt {
namespace {

using trn::ln_bwd_on;

constexpr int64_t kMaxInt = 0x7fffffff;

struct AuxPlan {
    size_t floats = 0;   // scratch the launchers ask for, in f32 elements (doubles counted twice)
};

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int aux_plan(const soccdpt_train_aux_args& a, AuxPlan& p, std::string& err) {
    auto bad = [&](const char* m) { err = std::string("soccdpt_op_train_aux: ") + m; return 1; };
    auto dims = [&](int n) {
        for (int i = 0; i < n; ++i)
            if (a.dim[i] < 1 || a.dim[i] > kMaxInt) return false;
        return true;
    };
    auto ins = [&](int n) {
        for (int i = 0; i < n; ++i)
            if (!a.in[i]) return false;
        return true;
    };
    auto outs = [&](int n) {
        for (int i = 0; i < n; ++i)
            if (!a.out[i]) return false;
        return true;
    };
    const char* const kDims = "dimensions must be positive (and fit an int)";
    const char* const kNull = "a required pointer is null";
    const int64_t* d = a.dim;
    switch (a.kind) {
        case SOCCDPT_AUX_LN_BWD:
            if (!dims(2)) return bad(kDims);
            if (!ins(3) || !outs(1)) return bad(kNull);
            if (!(a.f[0] > 0.f)) return bad("LN_BWD: eps must be positive");
            if (a.out[2] && !a.out[1]) return bad("LN_BWD: dgamma needs xhat");
            if ((a.out[2] || a.out[3]) && a.out[0] == a.in[2]) return bad("LN_BWD: dy may be dout itself only without dgamma / dbeta (their sums read dout after dy is written)");
            p.floats = (size_t)tr_colsum_chunks((size_t)d[0], (int)d[1]) * 2 * (size_t)d[1];
            return 0;
        case SOCCDPT_AUX_COLSUM:
        case SOCCDPT_AUX_COLSUM2:
            if (!dims(2)) return bad(kDims);
            if (!a.in[0] || !outs(a.kind == SOCCDPT_AUX_COLSUM2 ? 2 : 1)) return bad(kNull);
            p.floats = (size_t)tr_colsum_chunks((size_t)d[0], (int)d[1]) * (a.kind == SOCCDPT_AUX_COLSUM2 ? 2 : 1) * (size_t)d[1];
            return 0;
        case SOCCDPT_AUX_BN_FWD:
            if (!dims(2)) return bad(kDims);
            if (!ins(3) || !a.out[0] || !a.out[3] || !a.out[4]) return bad(kNull);
            if (!a.out[1] != !a.out[2]) return bad("BN_FWD: running_mean and running_var come together");
            if (!(a.f[0] > 0.f) || !(a.f[2] >= 0.f && a.f[2] < 1.f)) return bad("BN_FWD: eps must be positive and p in [0, 1)");
            p.floats = 2 * ((size_t)128 * d[1] + d[1]);   // (128 C + C) doubles
            return 0;
        case SOCCDPT_AUX_BN_BWD:
            if (!dims(2)) return bad(kDims);
            if (!ins(6) || !outs(3)) return bad(kNull);
            if (!(a.f[2] >= 0.f && a.f[2] < 1.f)) return bad("BN_BWD: p in [0, 1)");
            p.floats = 2 * (((size_t)d[0] * d[1] + 63) / 64 * 64) + (size_t)tr_colsum_chunks((size_t)d[0], (int)d[1]) * (size_t)d[1];
            return 0;
        case SOCCDPT_AUX_GN_BWD:
            if (!dims(4)) return bad(kDims);
            if (!ins(5)) return bad(kNull);
            if (!a.out[0] && !a.out[1] && !a.out[2]) return bad("GN_BWD: no output requested");
            if (d[2] > 1024 || d[2] % d[3]) return bad("GN_BWD: C <= 1024 and C % cpg == 0");
            if (d[0] * d[1] > kMaxInt) return bad(kDims);
            p.floats = (size_t)d[0] * th_gn_bwd_chunks((int)d[0], (int)d[1], (int)d[2]) * 2 * (size_t)d[2] + (size_t)d[0] * (size_t)(d[2] / d[3]) * 2;
            return 0;
        case SOCCDPT_AUX_WS_BWD:
            if (!dims(4)) return bad(kDims);
            if (!ins(3) || !outs(1)) return bad(kNull);
            if (d[1] * d[2] * d[2] > d[3]) return bad("WS_BWD: Kpad is smaller than the fan-in");
            if (!(a.f[0] > 0.f)) return bad("WS_BWD: eps must be positive");
            return 0;
        case SOCCDPT_AUX_BILINEAR_BWD:
            if (!dims(6)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (d[5] % 4 == 0 && (!aligned16(a.in[0]) || !aligned16(a.out[0]))) return bad("BILINEAR_BWD: C % 4 == 0 reads and writes float4: 16-byte aligned tensors");
            return 0;
        case SOCCDPT_AUX_MAXPOOL_BWD:
            if (!dims(4)) return bad(kDims);
            if (!ins(5) || !outs(2)) return bad(kNull);
            if (d[1] & 1) return bad("MAXPOOL_BWD: the input side must be even (the kernels pad behind the image only)");
            if (d[2] % d[3]) return bad("MAXPOOL_BWD: C % cpg == 0");
            return 0;
        case SOCCDPT_AUX_DEPTH_TAIL:
            if (!dims(2)) return bad(kDims);
            if (!ins(4) || !outs(3)) return bad(kNull);
            if (d[1] == 32 && (!aligned16(a.in[0]) || !aligned16(a.in[1]) || !aligned16(a.out[1]))) return bad("DEPTH_TAIL: K == 32 reads and writes float4: 16-byte aligned e, w4, de");
            return 0;
        case SOCCDPT_AUX_SMALLK:
            if (!dims(3)) return bad(kDims);
            if (d[2] > 4) return bad("SMALLK: K > 4");
            if (!a.in[0] || (!a.out[0] && !a.out[1]) || (a.out[0] && !a.in[1]) || (a.out[1] && !a.in[2])) return bad(kNull);
            p.floats = a.out[1] ? (size_t)256 * d[2] * d[1] : 0;
            return 0;
        case SOCCDPT_AUX_GELU_BWD:
            if (!dims(1)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_AUX_RELU_BWD:
            if (!dims(1)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_AUX_RELU_BWD_HALO:
            if (!dims(4)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_AUX_SEG_ACT_BWD:
            if (!dims(3)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_AUX_MERGE_SCATTER:
            if (!dims(3)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (d[1] & 1) return bad("MERGE_SCATTER: R must be even");
            return 0;
        case SOCCDPT_AUX_SCALE_ROWS:
            if (!dims(3)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            if (d[1] % 4 || !aligned16(a.in[0]) || !aligned16(a.out[0])) return bad("SCALE_ROWS: C % 4 == 0 and 16-byte aligned tensors");
            return 0;
        case SOCCDPT_AUX_UNSCALE_CHECK:
            if (!dims(1)) return bad(kDims);
            if (!outs(2)) return bad(kNull);
            return 0;
        case SOCCDPT_AUX_DROP_PATH_FILL:
            if (!dims(1) || a.dim[1] < 0 || a.dim[1] > kMaxInt) return bad(kDims);
            if (!outs(1)) return bad(kNull);
            if (!(a.f[0] >= 0.f && a.f[0] < 1.f)) return bad("DROP_PATH_FILL: p in [0, 1)");
            return 0;
        default: return bad("unknown kind");
    }
}

size_t plan_bytes(const AuxPlan& p) {
    const size_t b = (p.floats * sizeof(float) + 255) & ~size_t(255);
    return b ? b : 256;   // never 0: 0 means bad arguments
}

template <typename T> const T* in(const soccdpt_train_aux_args& a, int i) { return static_cast<const T*>(a.in[i]); }
template <typename T> T* out(const soccdpt_train_aux_args& a, int i) { return static_cast<T*>(a.out[i]); }

}  // namespace

size_t train_aux_scratch_bytes(const soccdpt_train_aux_args& a, std::string& err) {
    AuxPlan p;
    if (aux_plan(a, p, err)) return 0;
    return plan_bytes(p);
}

int train_aux(const soccdpt_train_aux_args& a, void* scratch, size_t scratch_bytes, hipStream_t st, std::string& err) {
    AuxPlan p;
    if (aux_plan(a, p, err)) return 1;
    if (!scratch || reinterpret_cast<uintptr_t>(scratch) % 256) { err = "soccdpt_op_train_aux: the scratch must be 256-byte aligned"; return 1; }
    if (scratch_bytes < plan_bytes(p)) { err = "soccdpt_op_train_aux: scratch too small"; return 1; }
    float* S = static_cast<float*>(scratch);
    const int64_t* d = a.dim;
    auto F = [&](int i) { return in<float>(a, i); };
    auto O = [&](int i) { return out<float>(a, i); };
    switch (a.kind) {
        case SOCCDPT_AUX_LN_BWD:
            return ln_bwd_on(S, st, err, F(0), F(1), F(2), O(0), O(1), (size_t)d[0], (int)d[1], O(2), O(3), a.f[0]);
        case SOCCDPT_AUX_COLSUM:
            return tr_colsum(F(0), F(1), O(0), S, (size_t)d[0], (int)d[1], a.flags & 1, st, err);
        case SOCCDPT_AUX_COLSUM2:
            return tr_colsum2(F(0), F(1), O(0), O(1), S, (size_t)d[0], (int)d[1], st, err);
        case SOCCDPT_AUX_BN_FWD: {   // train_step.cpp train_forward, seg head
            const size_t M = (size_t)d[0];
            const int C = (int)d[1];
            TRY(tr_bn_stats(F(0), O(0), O(1), O(2), S, C, M, a.f[0], a.f[1], st, err));
            return tr_bn_relu_dropout_fwd(F(0), O(0), F(1), F(2), O(3), out<uint8_t>(a, 4), M, C, a.f[2], a.seed, st, err);
        }
        case SOCCDPT_AUX_BN_BWD: {   // train_step.cpp train_backward, seg head: G[0] = dz, G[3] = xhat, S_col
            const size_t M = (size_t)d[0];
            const int C = (int)d[1];
            const size_t n = (M * C + 63) / 64 * 64;
            float *dz = S, *xh = S + n, *col = S + 2 * n;
            float *dbeta = O(0), *dgamma = O(1);
            TRY(tr_bn_relu_dropout_bwd_pre(F(0), F(1), in<uint8_t>(a, 2), dz, M * C, a.f[2], st, err));
            TRY(tr_bn_xhat(F(3), F(4), xh, M, C, st, err));
            TRY(tr_colsum(dz, nullptr, dbeta, col, M, C, 0, st, err));
            TRY(tr_colsum(dz, xh, dgamma, col, M, C, 0, st, err));
            return tr_bn_bwd(dz, F(3), F(4), F(5), dbeta, dgamma, O(2), M, C, st, err);
        }
        case SOCCDPT_AUX_GN_BWD:
            return th_gn_bwd(F(0), F(1), F(2), F(3), F(4), O(0), O(1), O(2), S, (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.flags & 1, st, err);
        case SOCCDPT_AUX_WS_BWD:
            return th_ws_bwd(F(0), F(1), F(2), O(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.f[0], st, err);
        case SOCCDPT_AUX_BILINEAR_BWD:
            return tr_bilinear_bwd(F(0), O(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], a.flags & 1, st, err);
        case SOCCDPT_AUX_MAXPOOL_BWD:
            return th_maxpool_bwd(F(0), F(1), F(2), F(3), F(4), out<uint8_t>(a, 0), O(1), (int)d[0], (int)d[1], (int)d[2], (int)d[3], st, err);
        case SOCCDPT_AUX_DEPTH_TAIL:   // train_forward's tail, then train_backward's first launch
            TRY(tr_depth_tail_fwd(F(0), F(1), F(2), O(0), (size_t)d[0], (int)d[1], st, err));
            return tr_depth_tail_bwd(F(3), O(0), F(0), F(1), O(1), O(2), (size_t)d[0], (int)d[1], st, err);
        case SOCCDPT_AUX_SMALLK:
            if (a.out[1]) TRY(tr_smallk_wgrad(F(0), F(2), O(1), S, (size_t)d[0], (int)d[1], (int)d[2], st, err));
            if (a.out[0]) TRY(tr_smallk_dgrad(F(0), F(1), O(0), (size_t)d[0], (int)d[1], (int)d[2], st, err));
            return 0;
        case SOCCDPT_AUX_GELU_BWD:
            return tr_gelu_bwd(F(0), F(1), O(0), (size_t)d[0], st, err);
        case SOCCDPT_AUX_RELU_BWD:
            return tr_relu_bwd(F(0), F(1), F(2), O(0), (size_t)d[0], st, err);
        case SOCCDPT_AUX_RELU_BWD_HALO:
            return tr_relu_bwd_halo(F(0), F(1), F(2), O(0), (int)d[0], (int)d[1], (int)d[2], (int)d[3], st, err);
        case SOCCDPT_AUX_SEG_ACT_BWD:
            return tr_seg_act_bwd(F(0), F(1), O(0), (int)d[0], (int)d[1], (int)d[2], a.flags & 1, st, err);
        case SOCCDPT_AUX_MERGE_SCATTER:
            return tr_merge_scatter(F(0), O(0), (int)d[0], (int)d[1], (int)d[2], st, err);
        case SOCCDPT_AUX_SCALE_ROWS:
            return tr_scale_rows(F(0), O(0), F(1), (size_t)d[0], (int)d[1], (int)d[2], st, err);
        case SOCCDPT_AUX_UNSCALE_CHECK:
            return tr_unscale_check(O(0), (size_t)d[0], a.f[0], out<int>(a, 1), st, err);
        case SOCCDPT_AUX_DROP_PATH_FILL:
            return tr_drop_path_fill(O(0), (int)d[0], a.f[0], a.seed, (unsigned)d[1], st, err);
    }
    err = "soccdpt_op_train_aux: unknown kind";
    return 1;
}

}  // namespace soccdpt
