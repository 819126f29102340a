// soccdpt_op_fwd_aux (include/soccdpt_hip.h: tests): one of the forward path's non-GEMM launchers of elementwise.hip / hybrid.hip -- or the forward's own
// composition of two of them -- on caller-supplied tensors.  No kernel lives here: every launch goes through the launch_* function model.cpp, train_step.cpp and
// train_hybrid_step.cpp call.  fwd_plan() checks what the entry itself dereferences or composes (kinds, dimensions, required pointers, and the conditions
// of a composition's SECOND launcher, so that a refused call has launched nothing); every other contract is the launcher's own and is refused there, before
// its launch: the product path calls the launchers directly.
#include <cstdint>

#include "kernels.h"

namespace soccdpt {
namespace {

constexpr int64_t kMaxInt = 0x7fffffff;

int fwd_plan(const soccdpt_fwd_aux_args& a, std::string& err) {
    auto bad = [&](const char* m) { err = std::string("soccdpt_op_fwd_aux: ") + m; return 1; };
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
    const char* const kFmt = "unknown operand format";
    const int64_t* d = a.dim;
    const int fmt = (a.flags >> 4) & 0xf, hfmt = (a.flags >> 8) & 0xf;
    const bool hf_ok = fmt == 0 || fmt == 1 || fmt == 3, mode_ok = fmt <= 3;
    switch (a.kind) {
        case SOCCDPT_FWD_PATCH_EMBED:
            if (!dims(3)) return bad(kDims);
            if (!ins(5) || !a.out[0] || !a.out[2]) return bad(kNull);
            if (!hf_ok) return bad(kFmt);
            if (d[2] > 128 && d[2] != 192) return bad("PATCH_EMBED: C0 > 128 (and not 192)");   // launch_patch_embed's own conditions: it is the second launch (out[2]: [48][patch_w_ld(C0)])
            if (d[1] % 32) return bad("PATCH_EMBED: the image side must be a multiple of 32");
            if (fmt == 3 && d[2] % 16) return bad("PATCH_EMBED: x3 rows are multiples of 16 elements");
            return 0;
        case SOCCDPT_FWD_LN_RESIDUAL:
            if (!dims(2) || d[2] < 0 || d[2] > kMaxInt || d[3] < 0 || d[3] > kMaxInt) return bad(kDims);
            if (!ins(3) || !a.out[0]) return bad(kNull);
            if (!hf_ok || (hfmt && hfmt != 1 && hfmt != 2 && hfmt != 4)) return bad(kFmt);
            if (a.in[3] && d[3] < 1) return bad("LN_RESIDUAL: row_scale needs rows_per_scale");
            if ((a.out[2] || a.out[3]) && (d[2] < 1 || d[0] % (d[2] * d[2]))) return bad("LN_RESIDUAL: a halo needs the token grid's side (M = B res^2)");
            return 0;
        case SOCCDPT_FWD_MERGE_GATHER:
            if (!dims(4)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_FWD_BILINEAR:
            if (!dims(6)) return bad(kDims);
            if (!ins(1) || (!a.out[0] && !a.out[1] && !a.out[2])) return bad(kNull);
            if (!hf_ok) return bad(kFmt);
            return 0;
        case SOCCDPT_FWD_SEG_TAIL:
            if (!dims(3)) return bad(kDims);
            if (!ins(3) || !outs(2)) return bad(kNull);
            if (fmt > 1) return bad(kFmt);
            if (d[0] * d[1] * d[2] > kMaxInt / 16) return bad(kDims);
            return 0;
        case SOCCDPT_FWD_CVT:
            if (!dims(1)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (!hf_ok && fmt != 5) return bad(kFmt);
            return 0;
        case SOCCDPT_FWD_CONV_W:
            if (!dims(2)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (!hf_ok) return bad(kFmt);
            return 0;
        case SOCCDPT_FWD_BN_FOLD:
            if (!dims(1)) return bad(kDims);
            if (!ins(4) || !outs(2)) return bad(kNull);
            return 0;
        case SOCCDPT_FWD_QKV_BIAS:
            if (!dims(1)) return bad(kDims);
            if (!ins(2) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_FWD_LOGIT_SCALE:
            if (!dims(1)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_FWD_CPB_TABLE:
            if (!dims(1) || d[1] < 0 || d[1] > kMaxInt || d[2] < 1 || d[2] > kMaxInt) return bad(kDims);
            if (d[0] > 1024 || d[2] > 4096) return bad(kDims);   // (2 ws - 1)^2 H in an int
            if (!ins(3) || !outs(1)) return bad(kNull);
            return 0;
        case SOCCDPT_FWD_WS_CONV_W:
            if (!dims(4)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (!mode_ok) return bad(kFmt);
            if (!(a.f[0] > 0.f)) return bad("WS_CONV_W: eps must be positive");
            return 0;
        case SOCCDPT_FWD_STEM_IM2COL:
            if (!dims(2)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (!mode_ok) return bad(kFmt);
            return 0;
        case SOCCDPT_FWD_GN_RELU_MAXPOOL:
            if (!dims(4)) return bad(kDims);
            if (!ins(4) || !outs(1)) return bad(kNull);
            if (!mode_ok) return bad(kFmt);
            return 0;
        case SOCCDPT_FWD_VIT_TOKENS_LN:
            if (!dims(3) || d[1] < 2) return bad(kDims);
            if (!ins(5) || !outs(2)) return bad(kNull);
            if (!mode_ok) return bad(kFmt);
            if (!(a.f[0] > 0.f)) return bad("VIT_TOKENS_LN: eps must be positive");
            if (d[0] * d[1] > kMaxInt) return bad(kDims);
            return 0;
        case SOCCDPT_FWD_LN_ROWS:
            if (!dims(2)) return bad(kDims);
            if (!ins(2) || !outs(2)) return bad(kNull);
            if (!mode_ok) return bad(kFmt);
            if (!(a.f[0] > 0.f)) return bad("LN_ROWS: eps must be positive");
            return 0;
        case SOCCDPT_FWD_POS_EMBED_RESIZE:
            if (!dims(3)) return bad(kDims);
            if (!ins(1) || !outs(1)) return bad(kNull);
            if (d[0] > 4096 || d[1] > 4096) return bad(kDims);
            return 0;
        default: return bad("unknown kind");
    }
}

template <typename T> const T* in(const soccdpt_fwd_aux_args& a, int i) { return static_cast<const T*>(a.in[i]); }
template <typename T> T* out(const soccdpt_fwd_aux_args& a, int i) { return static_cast<T*>(a.out[i]); }

int run(const soccdpt_fwd_aux_args& a, int* path, hipStream_t st, std::string& err) {
    const int64_t* d = a.dim;
    auto F = [&](int i) { return in<float>(a, i); };
    auto O = [&](int i) { return out<float>(a, i); };
    auto H = [&](int i) { return out<bf16_t>(a, i); };
    const int fmt = (a.flags >> 4) & 0xf, hfmt = ((a.flags >> 8) & 0xf) - 1;
    switch (a.kind) {
        case SOCCDPT_FWD_PATCH_EMBED:   // model.cpp: the weight is prepared once, the forward reads the prepared one
            if (launch_patch_w(F(1), O(2), (int)d[2], st, err)) return 1;
            return launch_patch_embed(F(0), O(2), F(2), F(3), F(4), O(0), H(1), fmt, (int)d[0], (int)d[1], (int)d[2], st, err);
        case SOCCDPT_FWD_LN_RESIDUAL:
            return launch_ln_residual(F(0), F(1), F(2), O(0), H(1), H(2), O(3), fmt, (int)d[0], (int)d[1], a.flags & 1, (int)d[2], (a.flags >> 1) & 1, st, err, F(3),
                                      a.in[3] ? (int)d[3] : 1, hfmt, path);
        case SOCCDPT_FWD_MERGE_GATHER:
            return launch_merge_gather(a.in[0], a.out[0], (int)d[0], (int)d[1], (int)d[2], (int)d[3], st, err);
        case SOCCDPT_FWD_BILINEAR:
            return launch_bilinear(a.in[0], a.flags & 1, O(0), H(1), O(2), (a.flags >> 1) & 1, fmt, (int)d[0], (int)d[1], (int)d[2], (int)d[3], (int)d[4], (int)d[5], st,
                                   err, path);
        case SOCCDPT_FWD_SEG_TAIL:
            return launch_seg_tail(a.in[0], (a.flags >> 1) & 1, fmt, F(1), F(2), O(0), O(1), (int)d[0], (int)d[1], (int)d[2], a.flags & 1, st, err, path);
        case SOCCDPT_FWD_CVT:
            return launch_cvt_bf16(F(0), H(0), (size_t)d[0], fmt, st, err);
        case SOCCDPT_FWD_CONV_W:
            return launch_conv_w(F(0), F(1), a.out[0], a.flags & 1, fmt, (int)d[0], (int)d[1], st, err);
        case SOCCDPT_FWD_BN_FOLD:
            return launch_bn_fold(F(0), F(1), F(2), F(3), O(0), O(1), (int)d[0], st, err);
        case SOCCDPT_FWD_QKV_BIAS:
            return launch_qkv_bias(F(0), F(1), O(0), (int)d[0], st, err);
        case SOCCDPT_FWD_LOGIT_SCALE:
            return launch_logit_scale(F(0), O(0), (int)d[0], st, err);
        case SOCCDPT_FWD_CPB_TABLE:
            return launch_cpb_table(F(0), F(1), F(2), O(0), (int)d[0], (int)d[1], (int)d[2], st, err);
        case SOCCDPT_FWD_WS_CONV_W:
            return launch_ws_conv_w(F(0), a.out[0], fmt, (int)d[0], (int)d[1], (int)d[2], (int)d[3], a.f[0], st, err);
        case SOCCDPT_FWD_STEM_IM2COL:
            return launch_stem_im2col(F(0), a.out[0], fmt, (int)d[0], (int)d[1], st, err);
        case SOCCDPT_FWD_GN_RELU_MAXPOOL:
            return launch_gn_relu_maxpool(F(0), F(1), F(2), F(3), a.out[0], fmt, (int)d[0], (int)d[1], (int)d[2], (int)d[3], st, err);
        case SOCCDPT_FWD_VIT_TOKENS_LN:
            return launch_vit_tokens_ln(F(0), F(1), F(2), O(0), F(3), F(4), a.out[1], fmt, (int)d[0], (int)d[1], (int)d[2], a.f[0], st, err);
        case SOCCDPT_FWD_LN_ROWS:
            return launch_ln_rows(O(0), F(0), F(1), a.out[1], fmt, (int)d[0], (int)d[1], a.f[0], st, err);
        case SOCCDPT_FWD_POS_EMBED_RESIZE:
            return launch_pos_embed_resize(F(0), O(0), (int)d[0], (int)d[1], (int)d[2], st, err);
    }
    err = "unknown kind";
    return 1;
}

}  // namespace

int fwd_aux(const soccdpt_fwd_aux_args& a, unsigned* path, hipStream_t st, std::string& err) {
    if (fwd_plan(a, err)) return 1;
    int p = 0;
    if (run(a, &p, st, err)) {
        err = "soccdpt_op_fwd_aux: " + err;
        return 1;
    }
    if (path) *path = (unsigned)p;
    return 0;
}

}  // namespace soccdpt
