// Launchers of train.hip (backward / train-mode forward kernels; the staging launchers write the operand format they are given) and the training
// entry points of train_step.cpp.
#pragma once
#include <vector>
#include "internal.h"
#include "kernels.h"
#include "train_plan.h"

namespace soccdpt {

constexpr int op_cvt_hf(OpFmt f) { return f == OpFmt::X3 ? 3 : f == OpFmt::F16 ? 5 : 0; }             // launch_cvt_bf16's `hf` (kernels.h); F32 has no conversion
constexpr int op_igemm_f16(OpFmt f) { return f == OpFmt::F16 ? 1 : 0; }                                // IgemmDesc::f16

// Every dgrad weight operand of one backward pass staged by a handful of launches instead of one per layer (round 4: 81 launches, 0.7 ms per bf16-amp step).
// kind 0: [R][C] -> [C][R] (tr_transpose with Rp = R); kind 1: conv weight [R = N][C][3][3] -> tr_conv_w_dgrad's layout.  Same element
// conversions as the single forms, so the staged copies are bit-identical to theirs.
struct TrBatchEntry {
    const float* src;
    void* dst;
    int R, C, kind, tile0;   // tile0: first block of this entry in the launch's grid
};
constexpr int kTrBatchMax = 64;
struct TrBatchTable {
    TrBatchEntry e[kTrBatchMax];
    int n;
};
int tr_weight_batch(const TrBatchTable& t, int total_tiles, OpFmt fmt, hipStream_t st, std::string& err);
int tr_transpose(const float* in, void* out, OpFmt fmt, int R, int C, int Rp, hipStream_t st, std::string& err);
int tr_im2colT(const float* halo, void* out, OpFmt fmt, int B, int H, int W, int C, size_t Mp, hipStream_t st, std::string& err);
int tr_dy_halo_T(const float* dy, void* out, OpFmt fmt, int B, int r, int N, int margin, int ld, hipStream_t st, std::string& err, int rpp = 0);
int tr_x_halo_T_x3(const float* halo, void* out, int B, int r, int C, int col0, int ld, int rpp, hipStream_t st, std::string& err);
int tr_conv_w_dgrad(const float* w, void* out, OpFmt fmt, int N, int C, hipStream_t st, std::string& err);
int tr_wgrad_permute(const float* in, float* out, int N, int C, hipStream_t st, std::string& err);
int tr_to_halo(const float* in, float* out, int B, int H, int W, int C, hipStream_t st, std::string& err);
int tr_to_halo_full(const float* in, void* out, OpFmt fmt, int B, int H, int W, int C, hipStream_t st, std::string& err);   // whole image incl. a zero border
// f32 -> bf16 / IEEE fp16 / x3 of two tensors, one launch.  Element counts: multiples of 4 (x3: of 16).
int tr_cvt_pair(const float* in0, void* out0, size_t n0, const float* in1, void* out1, size_t n1, OpFmt fmt, hipStream_t st, std::string& err);
int tr_colsum_chunks(size_t M, int N);   // row chunks of tr_colsum / tr_colsum2: their scratch is chunks * N (colsum2: 2N) floats
int tr_colsum(const float* a, const float* b, float* out, float* scratch, size_t M, int N, int accumulate, hipStream_t st, std::string& err);
int tr_colsum2(const float* a, const float* b, float* out_ab, float* out_a, float* scratch, size_t M, int N, hipStream_t st, std::string& err);   // sum a*b and sum a in one pass
int tr_axpy(float* y, const float* x, size_t n, hipStream_t st, std::string& err);
int tr_relu_bwd(const float* dy, const float* ref, const float* add, float* dx, size_t n, hipStream_t st, std::string& err);
int tr_relu_bwd_halo(const float* dy, const float* ref_halo, const float* add, float* dx, int B, int H, int W, int C, hipStream_t st, std::string& err);
int tr_gelu_bwd(const float* dy, const float* pre, float* dx, size_t n, hipStream_t st, std::string& err);
int tr_ln_bwd(const float* y, const float* g, const float* dout, float* dy, float* xhat, int M, int C, float eps, hipStream_t st, std::string& err);
int tr_bilinear_bwd(const float* dhi, float* dlo, int B, int h, int w, int H, int W, int C, int accumulate, hipStream_t st, std::string& err);
int tr_bn_stats(const float* x, float* stats, float* rmean, float* rvar, void* scratch, int C, size_t M, float eps, float momentum, hipStream_t st, std::string& err);
int tr_bn_relu_dropout_fwd(const float* x, const float* stats, const float* gamma, const float* beta, float* out, uint8_t* keep, size_t M, int C, float p, uint32_t seed, hipStream_t st, std::string& err);
int tr_bn_relu_dropout_bwd_pre(const float* dout, const float* out, const uint8_t* keep, float* dz, size_t n, float p, hipStream_t st, std::string& err);
int tr_bn_bwd(const float* dz, const float* x, const float* stats, const float* gamma, const float* dbeta, const float* dgamma, float* dx, size_t M, int C, hipStream_t st, std::string& err);
int tr_bn_xhat(const float* x, const float* stats, float* xh, size_t M, int C, hipStream_t st, std::string& err);
int tr_smallk_dgrad(const float* dl, const float* w, float* dx, size_t M, int C, int K, hipStream_t st, std::string& err);
int tr_smallk_wgrad(const float* dl, const float* x, float* dw, float* scratch, size_t M, int C, int K, hipStream_t st, std::string& err);
int tr_seg_act_bwd(const float* dseg, const float* seg, float* dup, int B, int K, int S, int sigmoid, hipStream_t st, std::string& err);
int tr_depth_tail_fwd(const float* e, const float* w4, const float* b4, float* inv, size_t M, int K, hipStream_t st, std::string& err);
int tr_depth_tail_bwd(const float* dinv, const float* inv, const float* e, const float* w4, float* de, float* rowterm, size_t M, int K, hipStream_t st, std::string& err);
int tr_merge_scatter(const float* dg, float* dx, int B, int R, int C, hipStream_t st, std::string& err);
int tr_patch_im2col(const float* x, float* out, int B, int S, hipStream_t st, std::string& err);
int tr_pad_cols(const float* in, float* out, int N, int cin, int cout, hipStream_t st, std::string& err);
// Cosine window attention backward on the matrix cores (train_attn.hip): rowstat holds {m + ln l, delta}; dscale_part has tr_attention_bwd_mfma_slots(ws) per
// (window, head); refused before anything is launched: a null pointer, what window_attention_geometry refuses (the shift is 0 or ws / 2), a window size without
// an instantiation, x3
int tr_attention_bwd_mfma(const float* qkv, const float* attn_out, const float* dO, const float* table, const float* scale, float* dS, float* rowstat,
                          float* dscale_part, float* dqkv, int B, int res, int ws, int shift, int heads, hipStream_t st, std::string& err, OpFmt fmt);   // fmt: F32, BF16 or F16 products
int tr_attention_bwd_mfma_slots(int ws);
// Weight gradient from operands as stored (train_wgrad_tn.hip): out[Nout][taps * C] = sum_k A[k][n] B[k + shift(tap)][c], 16-bit or x3 operands; shapes:
// tr_wgrad_tn_ok (train_plan.h)
// Deferred reduction of the weight-gradient partials (round 6): every tr_wgrad_tn call used to be followed by its own tn_reduce launch -- 74 launches of ~14 us per
// bf16-amp step whose work is a few hundred KB each.  With a TnDefer the partials of successive calls stay in an arena (bump allocation, flushed when full) and ONE
// batched launch per <= 48 gradients sums them -- in split order, like tn_reduce_kernel: the same bits -- at the end of the backward pass (tn_flush).  perm_C > 0: the
// batched launch also writes the 3x3 gradient from the kernel's tap-major [N][9][C] into the parameter layout [N][C][3][3] (tr_wgrad_permute's job).
struct TnPending { const float* part; float* out; const float* bpart; float* bout; unsigned long long n4; int splits, nb, perm_N, perm_C; };
struct TnDefer {
    float* arena = nullptr;
    size_t cap = 0, used = 0;
    std::vector<TnPending> pend;
};
int tn_flush(TnDefer& d, hipStream_t st, std::string& err);
int tr_wgrad_tn(const void* A, long ldA, const void* B, long ldB, size_t K, int Nout, int C, int taps, int rp, OpFmt fmt, float* part, size_t part_floats,
                float* out, hipStream_t st, std::string& err, float* bias_out = nullptr, TnDefer* defer = nullptr, int perm_C = 0);
int tr_attn_param_grads(float* dS, const float* dscale_part, const float* table, const float* ls, const float* w0, const float* b0, const float* w2, float* dtable, float* dt, float* hid, float* dls, float* dw0, float* db0, float* dw2, int nwin, int ws, int pws, int heads, int dscale_slots, hipStream_t st, std::string& err);
int tr_drop_path_fill(float* out, int B, float p, unsigned seed, unsigned stream_id, hipStream_t st, std::string& err);
int tr_scale_rows(const float* in, float* out, const float* scale, size_t M, int C, int rows_per_scale, hipStream_t st, std::string& err);
int tr_unscale_check(float* g, size_t n, float inv_scale, int* found, hipStream_t st, std::string& err);
int tr_qv_bias_grad(const float* dqkv_bias, float* dq, float* dv, int C, hipStream_t st, std::string& err);

// train_hybrid.hip: ViT-hybrid encoder (ResNetV2 stem and stages, ViT-B blocks, readout)
int th_gn_bwd_chunks(int B, int HW, int C);   // pixel chunks per sample: th_gn_bwd's scratch is B * chunks * 2C + B * (C / cpg) * 2 floats
int th_gn_bwd(const float* dout, const float* x, const float* stats, const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, float* scratch, int B,
              int HW, int C, int cpg, int relu, hipStream_t st, std::string& err);
int th_ws_bwd(const float* dwh, const float* wh, const float* w, float* dw, int Cout, int Cin, int k, int Kpad, float eps, hipStream_t st, std::string& err);
int th_conv_w_dgrad_tap(const float* wt, float* out, int N, int C, hipStream_t st, std::string& err);
int th_im2colT_gen(const float* halo, float* out, int B, int Hi, int Ho, int C, int stride, int pad, size_t Mp, hipStream_t st, std::string& err);
int th_col2im(const float* dcol, float* dx, int B, int Hi, int Ho, int C, int stride, int pad, int accumulate, hipStream_t st, std::string& err);
int th_stride_gather(const float* in, float* out, int B, int Hi, int Ho, int C, int stride, hipStream_t st, std::string& err);
int th_stride_scatter_add(const float* dg, float* dx, int B, int Hi, int Ho, int C, int stride, hipStream_t st, std::string& err);
int th_maxpool_bwd(const float* dpool, const float* raw, const float* stats, const float* gamma, const float* beta, uint8_t* idx, float* dA, int B, int Hi, int C, int cpg,
                   hipStream_t st, std::string& err);
int th_readout_cat(const float* tok, float* cat, int B, int NT, int E, hipStream_t st, std::string& err);
int th_readout_cat_bwd(const float* dcat, float* dtok, int B, int NT, int E, int accumulate, hipStream_t st, std::string& err);
int th_tokens_to_patches(const float* dtok, float* dpatch, int B, int NT, int E, hipStream_t st, std::string& err);
// train_attn.hip: global softmax attention backward of the ViT blocks on the matrix cores; fmt: F32, BF16 or F16 products
int th_vit_attention_bwd_mfma(const float* qkv, const float* O, const float* dO, float* rowstat, float* dqkv, int B, int N, int heads, hipStream_t st, std::string& err, OpFmt fmt);

// train_step.cpp: SOccDPT_V3 training step (model/SOccDPT.py:660-685 in train mode + autograd) on SOCCDPT_PREC_F32 handles; arithmetic by soccdpt_train_set_amp (OpFmt)
size_t train_workspace_bytes(Handle& h, int B);
int train_backward_encoder(Handle& h, int B, const float* const* d_feat, void* ws, size_t ws_bytes, hipStream_t st, std::string& err);
int train_workspace_tensor(Handle& h, int B, const char* name, size_t* byte_offset, size_t* elems);
int train_forward(Handle& h, const float* x, int B, float* inv, float* seg, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, hipStream_t st, std::string& err);
int train_backward(Handle& h, const float* x, int B, const float* d_inv, const float* d_seg, void* ws, size_t ws_bytes, hipStream_t st, std::string& err);
// One call of linear_bwd / conv3_bwd / conv_gen_bwd on caller-supplied tensors (soccdpt_op_train_layer_bwd, include/soccdpt_hip.h: tests); *path_out: SOCCDPT_ROUTE_* bits
size_t train_layer_bwd_scratch_bytes(const soccdpt_train_layer_bwd_args& a, std::string& err);   // 0: bad arguments
int train_layer_bwd(Handle& h, const soccdpt_train_layer_bwd_args& a, void* scratch, size_t scratch_bytes, unsigned* path_out, hipStream_t st, std::string& err);

// One non-GEMM launcher (or the step's composition of a few) on caller-supplied tensors (soccdpt_op_train_aux, include/soccdpt_hip.h: tests)
size_t train_aux_scratch_bytes(const soccdpt_train_aux_args& a, std::string& err);   // 0: bad arguments
int train_aux(const soccdpt_train_aux_args& a, void* scratch, size_t scratch_bytes, hipStream_t st, std::string& err);

}  // namespace soccdpt
