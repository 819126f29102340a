// Shared declarations of the training step's translation units (train_step.cpp: Swin-V2 encoders, decoder, heads; train_hybrid_step.cpp: the
// ViT-hybrid encoder).
#pragma once
#include <algorithm>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "train.h"

namespace soccdpt {
namespace trn {

struct TArena {
    char* base;
    size_t off = 0;
    explicit TArena(void* p) : base(static_cast<char*>(p)) {}
    float* f(size_t n) {
        off = (off + 255) & ~size_t(255);
        float* p = base ? reinterpret_cast<float*>(base + off) : nullptr;
        off += n * sizeof(float);
        return p;
    }
};

constexpr size_t kTrainSkPartFloats = (size_t)8 << 20;   // 32 MB of f32 split-K partials
constexpr size_t kTrainSkCountWords = 4096;
constexpr size_t kTrainTnArenaFloats = (size_t)160 << 20;   // 640 MB: the weight-gradient partials of one backward pass wait here for the batched sum (train.h TnDefer); flushed when full

struct BlkT {
    float *qkv_bias, *scale, *table, *bias_acc;
    const float* xin;
    float *qkv, *attn, *a_pre, *x1, *hpre, *hact, *m_pre, *xout;
    float* dp;   // stochastic depth: [2][B] per-sample scales of the attention / MLP branch (0 or 1 / (1 - p_block)); see train_forward
};

// ViT-hybrid encoder tape (train_hybrid_step.cpp)
struct RnBlkT {
    const float* xin;                           // [B*rin*rin][cin]
    float *w_ds, *w_c1, *w_c2, *w_c3;           // standardised weights, tap-major
    float *ds_raw, *ds_stats, *c1_raw, *c1_stats, *t1 /*halo*/, *c2_raw, *c2_stats, *t2, *c3_raw, *c3_stats, *out;
};
struct VitBlkT {
    const float* xin;
    float *ln1, *qkv, *attn, *x1, *ln2, *hpre, *hact, *xout, *rowstat;
};
struct HyTape {
    float *a0, *w_stem, *stem_raw, *stem_stats, *pool;
    uint8_t* pool_idx;
    std::vector<RnBlkT> blk;
    float *pe_y, *x0;
    std::vector<VitBlkT> vb;
    float *cat[2], *ro_pre[2], *ro_act[2], *pp4_in /*halo*/, *w_pp4;
    float* gn_part[2] = {nullptr, nullptr};   // per-tile GroupNorm partials of the convolution(s) whose output is waiting for its gn_apply: [0] conv1 / conv2 / conv3, [1] the shortcut projection
    int gn_bm[2] = {0, 0};                     // M-tile rows of the launch that last filled each buffer
    size_t gn_part_floats = 0;
    float *GT, *GR, *xg;                       // token-stream / residual-stream gradients, strided-shortcut operand
};

struct Tape {
    HyTape hy;
    const float* xt_tn_src = nullptr;   // the halo image whose copy in conv3_wgrad_tn's layout is in S_T2, or nullptr: conv3_bwd's reuse_xt only holds within one layout
    // encoder
    float *patches, *pe_wpad, *pe_pre, *x0;
    std::vector<BlkT> blk[4];
    float *mg[3], *mr_pre[3], *mx[3];
    float* feat[4];   // zero-halo
    // decoder (level 0 = finest); *_relu / t1 / t2 are zero-halo images
    float *lrn_raw[4], *lrn_relu[4], *t1[4], *out_raw[4], *out_relu[4], *t2[4], *u[4], *oc[4];
    float *w_lrn[4], *w_rcu[4][2][2];
    float *path1, *d1, *d1u, *e, *inv, *seg;
    float *w_d0, *w_d2, *w_s0;
    float *c_raw, *bn_stats, *r, *logits;
    uint8_t* keep;
    // halo zone [halo_lo, halo_hi): zero-filled at the start of every forward
    size_t halo_lo = 0, halo_hi = 0;
    // backward scratch
    float *G[5], *GX, *GP, *DOC, *DF[4];
    float *S_T1, *S_T2, *S_halo, *S_wt, *S_dw, *S_col, *S_vec;
    float *dS, *rowstat, *dscale_part, *dtable, *dt, *S_cpb;
    float* sk_part;
    float* tn_arena;
    ScratchNeed S_cap;   // floats of S_T1, S_T2, S_halo, S_wt and S_dw (carve / carve_layer): every helper holds its plan's need against them (check_fit)
    unsigned* sk_count;
    // dgrad weight operands of the whole backward pass, staged by stage_weights() in a few batched launches (4 bytes per element reserved per weight)
    float* WT = nullptr;
    std::vector<long long> wt_off;                        // per Handle::weights index: element offset of its slot in WT, -1 = not staged (odd shapes)
    std::unordered_map<const float*, long long> wt_by_ptr;   // bound weight pointer -> slot offset, filled by stage_weights()
    size_t maxAct = 0;
    float dropout_p = 0.f;
};

struct Ctx {
    Handle& h;
    Tape& T;
    int B;
    hipStream_t st;
    std::string& err;
    unsigned path = 0;   // SOCCDPT_ROUTE_* bits (soccdpt_hip.h), set where linear_bwd / conv3_bwd / conv_gen_bwd / gemm / gemm_wgrad take their decisions; read by train_layer_bwd
    TnDefer tn;   // deferred weight-gradient sums of this pass (flushed by train_backward / train_backward_encoder before they return)
    std::unordered_set<const void*> grad_ptrs;   // the bound parameter-gradient buffers: only sums that land THERE may wait (a gradient written into scratch is read by its caller's next launch)
    bool may_defer(const float* dW, const float* db) const { return tn.arena && grad_ptrs.count(dW) && (!db || grad_ptrs.count(db)); }
    void arm_defer(float* arena, size_t cap) { tn.arena = arena; tn.cap = cap; for (const auto& w : h.weights) if (w.grad) grad_ptrs.insert(w.grad); }
    const float* W(PRef r) const { return h.W(r); }
    float* Gd(PRef r) const { return h.G(r); }
};

#define TRY(call) do { if (call) return 1; } while (0)

inline unsigned route_fmt_bit(OpFmt f) {
    return f == OpFmt::F32 ? SOCCDPT_ROUTE_FMT_F32 : f == OpFmt::BF16 ? SOCCDPT_ROUTE_FMT_BF16 : f == OpFmt::F16 ? SOCCDPT_ROUTE_FMT_F16 : SOCCDPT_ROUTE_FMT_X3;
}
inline unsigned route_wgrad_bit(WgradPath p) {
    return p == WgradPath::TN ? SOCCDPT_ROUTE_WGRAD_TN : p == WgradPath::Transpose ? SOCCDPT_ROUTE_WGRAD_TRANSPOSE : p == WgradPath::X3Shift ? SOCCDPT_ROUTE_WGRAD_X3SHIFT :
           p == WgradPath::HaloShift ? SOCCDPT_ROUTE_WGRAD_HALOSHIFT : p == WgradPath::None ? 0u : SOCCDPT_ROUTE_WGRAD_IM2COLT;
}
// A helper's first step: what its plan (train_plan.h) may touch of the shared scratch regions must fit what carve() reserved.  Nothing is launched otherwise.
inline int check_fit(Ctx& c, const char* who, const ScratchNeed& need) {
    if (need.fits(c.T.S_cap)) return 0;
    c.err = std::string(who) + ": scratch region too small: " + need.misfit(c.T.S_cap);
    return 1;
}
// A weight gradient its caller wants INSIDE S_dw (derived weights: standardised ResNetV2 kernels, the padded patch embedding at kPeGradOffset) counts towards
// the need of the helper that writes it
inline ScratchNeed with_dw_target(const Tape& T, ScratchNeed need, const float* dW, size_t n) {
    if (dW && dW >= T.S_dw && dW < T.S_dw + T.S_cap.dw) need.dw = std::max(need.dw, (size_t)(dW - T.S_dw) + n);
    return need;
}
inline OpFmt amp_fmt(const Ctx& c) { return static_cast<OpFmt>(c.h.train_amp); }   // the operand format soccdpt_train_set_amp selected
int gemm(Ctx& c, IgemmDesc d, OpFmt fmt = OpFmt::F32);   // operands of format fmt, f32 outputs
// a GEMM of the train-mode FORWARD: exact f32, or -- any train amp mode -- its operands converted to x3 into scratch first (outputs stay f32)
int gemm_fwd(Ctx& c, IgemmDesc d, size_t x_elems, size_t w_elems);
int gemm_wgrad(Ctx& c, IgemmDesc d, OpFmt fmt);   // operands as written by the caller's staging kernels
int cvt_op(Ctx& c, const float* in, void* out, size_t n, OpFmt fmt);   // f32 -> bf16 / fp16 / x3 (launch_cvt_bf16)
int copy_d2d(Ctx& c, void* dst, const void* src, size_t bytes, const char* what);
// Transposed (Linear / 1x1) or rotated tap-major (3x3) copies of every regularly shaped bound weight in the amp mode's operand format, for the dgrad GEMMs of
// this backward pass: two or three launches instead of one per layer.  linear_bwd / conv3_bwd use a staged copy when they find one (staged_wt) and stage their
// own otherwise (derived weights: padded patch embedding, standardised ResNetV2 kernels).
int stage_weights(Ctx& c);
struct WtStage { const float* src; long long off; int R, C, kind; };   // one weight [R][C] (kind 0) or [R][C][3][3] (kind 1) and the element offset of its slot in Tape::WT
int wt_slot_kind(const int64_t* shape, size_t ndim);   // the kind of slot a weight of this shape has in Tape::WT, -1 = none (converted by its layer)
int stage_weight_list(Ctx& c, const std::vector<WtStage>& list);   // the launches of stage_weights over an explicit list
const void* staged_wt(const Ctx& c, const float* W);
// y = x W^T + b backward.  dY [M][N], X [M][K], W [N][K].  dX_out = dY W (+ dX_res); dW = dY^T X; db = colsum(dY).
int linear_bwd(Ctx& c, const float* dY, const float* X, const float* W, size_t M, int N, int K, float* dX_out, const float* dX_res, float* dW, float* db);
int conv3_bwd(Ctx& c, const float* dY, const float* Xhalo, const float* W, int r, int N, int C, float* dX_out, const float* dX_res, float* dW, float* db,
              bool reuse_xt = false);   // reuse_xt: the im2col^T of Xhalo is still in S_T2 from the previous call
// The 3x3 staging conv3_bwd shares with the ViT-hybrid encoder's conv_gen_bwd (stride 1 / pad 1; the callers differ in the weight layout and the output permute)
int conv3_dy_halo(Ctx& c, const float* dY, int r, int N, OpFmt fmt);   // dY as a zero-bordered image of format fmt in S_halo
int conv3_dgrad_s1(Ctx& c, const void* Wrot, int r, int N, int C, OpFmt fmt, float* dX_out, const float* dX_res);   // over S_halo and the rotated filter [C][9][N]
// weight gradient from S_halo and Xhalo as stored (train_wgrad_tn.hip) in the layout of the caller's plan p (already checked): tap-major into `out`, or --
// param_layout -- [N][C][3][3] by this pass's batched sum
int conv3_wgrad_tn(Ctx& c, const ConvPlan& p, const float* Xhalo, int N, int C, bool reuse_xt, float* out, float* bias, bool param_layout);
int ln_bwd(Ctx& c, const float* y, const float* g, const float* dout, float* dy, float* xhat, size_t M, int C, float* dg, float* dbeta, float eps = 1e-5f);
// the same over an explicit column-sum scratch, stream and error string (soccdpt_op_train_aux has no Ctx)
int ln_bwd_on(float* s_col, hipStream_t st, std::string& err, const float* y, const float* g, const float* dout, float* dy, float* xhat, size_t M, int C, float* dg,
              float* dbeta, float eps);
IgemmDesc conv_desc(const void* X, int Cin, const void* Wt, int N, int r, int B);
bool any_grad(const Handle& h, Span s);   // is a gradient bound to any tensor of the span?

// train_hybrid_step.cpp
// Backward of a 3x3 convolution with tap-major weights Wtap [N][9][C] over a zero-haloed input [B][Hi+2][Hi+2][C], output Ho x Ho; dWtap_out [N][9][C]
int conv_gen_bwd(Ctx& c, const float* dY, const float* Xhalo, const float* Wtap, int Hi, int Ho, int N, int C, int stride, int pad, float* dX_out, float* dWtap_out,
                 float* db);
void hy_carve_halo(const Handle& h, int B, TArena& ar, Tape& T);   // inside the zero-filled zone
void hy_carve(const Handle& h, int B, TArena& ar, Tape& T, size_t& maxAct);
int hy_forward(Ctx& c, const float* x);       // fills T.feat[0..3]
int hy_backward(Ctx& c);                       // consumes T.DF[0..3]

}  // namespace trn
}  // namespace soccdpt
