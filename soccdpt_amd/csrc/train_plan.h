// Scratch plans of the training backward: which weight-gradient path a layer takes, the layout of its staged operands in the five shared scratch
// regions of the training workspace (Tape::S_T1, S_T2, S_halo, S_wt, S_dw) and how many floats of each region the call may touch.  linear_bwd,
// conv3_bwd, conv_gen_bwd and gemm_fwd compute their plan first, hold its need against the capacities carve() recorded (Tape::S_cap) and take every
// layout number from it; soccdpt_op_train_layer_bwd sizes its scratch from the same plans.  Pure host arithmetic: no HIP header
// (tests/train_plan_main.cpp builds against this file with the host compiler alone).
//
// The contracts between the staging code and the kernels, each next to the field that carries it:
//   kTnOverread              tr_wgrad_tn (taps == 1) masks its edge tiles but loads whole 128-column tiles: behind the last row of either operand up to
//                            127 elements are read and dropped.  The need of a TN Linear counts them, so they stay inside the operand's own region.
//   LinearPlan::Mtn, ConvPlan::Kp
//                            K of the TN kernel is a multiple of its 64-row k-tile: rows M .. Mtn (Kh .. Kp) of both operands are zero rows the helper
//                            writes.  Row strides are the layer's N and C: multiples of 32 (16-bit: 8 would do, x3 needs 16), tr_wgrad_tn_ok's rule.
//   ConvPlan::mrg            TN 3x3: tap (ky, kx) reads the X operand (ky - 1) rp + (kx - 1) rows further on, so rp + 1 zero rows sit in front of and behind it.
//   ConvPlan::rpp, head, copy, ld (x3-shift)
//                            an x3 tensor is cut in 8-element units, so every view the GEMM reads starts at a multiple of 16 elements: the pixel rows are
//                            padded to rpp = roundup(rp, 16), the horizontal taps select one of three copies pre-shifted by -1 / 0 / +1 pixel (stride `copy`)
//                            and head, rpp, copy, ld are all multiples of 16.  Each copy is [head zeros][C][ld][head zeros]: the +- rpp views stay inside it.
//   ConvPlan::head, copy, ncopies (halo-shift)
//                            tap (ky, kx) is the view at head + (ky - 1) rp + (kx - 1) of ONE transposed halo image [C][ld]; `head` zeroed elements in
//                            front absorb the most negative shift, the zero tail of every row (ld >= Mh + 2 margin) the others.  16-bit operands: every
//                            tap's base must stay 4-byte aligned, so the taps with kx != 1 read a second copy shifted by one element (copy is even, the
//                            odd tap offsets become even) -- which holds for the vertical taps only while rp is even.  RULE: 16-bit halo-shift needs an
//                            even pixel pitch; 16-bit layers with an odd r take the explicit im2col^T instead (none of the three models has one; whether
//                            the hardware tolerates 2-byte aligned bases has not been measured).
//   ConvPlan::Mp, LinearPlan::Mp
//                            K of the transposing paths, a k-tile multiple (16-bit: 128, else 32); the staging kernels write the padding as zeros.
//   wt_grp_rows              the shifted-view GEMMs read groups of C weight rows: C % 64 == 0 (a weight tile never straddles two taps).
// The igemm reads and writes nothing behind the rows a plan counts (which is why no M-tile slack is added): its loads clamp the row index of both
// operands (igemm_kernel.h: `m = m < d.M ? m : d.M - 1`, likewise n) and every epilogue store, the split-K partials included, is under `m < d.M && n < N`.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "op_fmt.h"

namespace soccdpt {

// Shapes tr_wgrad_tn takes (train_wgrad_tn.hip; the callers fall back to a transposing path otherwise): K rows, out [Nout][taps * C]
inline bool tr_wgrad_tn_ok(size_t K, int Nout, int C, int taps) {
    if (K % 64 != 0 || K < 256) return false;
    if (taps == 9) return Nout % 128 == 0 && C % 128 == 0;   // a column tile must not straddle two taps
    return taps == 1 && Nout % 32 == 0 && C % 32 == 0;         // edge tiles are masked (kTnOverread)
}

namespace trn {

constexpr size_t kTnOverread = 127;       // elements tr_wgrad_tn may read behind the last row of an operand (taps == 1)
constexpr size_t kPeGradOffset = 65536;   // floats into S_dw at which the Swin encoders keep the 64-column padded patch-embedding gradient

inline size_t roundup(size_t v, size_t m) { return (v + m - 1) / m * m; }
inline size_t op_floats(size_t elems, OpFmt f) { return (elems * op_size(f) + 3) / 4; }   // floats that hold `elems` elements of format f

// Floats of each scratch region one call may touch: what it writes (zero padding included) and what its kernels may read behind that
struct ScratchNeed {
    size_t t1 = 0, t2 = 0, halo = 0, wt = 0, dw = 0;
    void merge(const ScratchNeed& o);
    bool fits(const ScratchNeed& cap) const { return misfit(cap).empty(); }
    std::string misfit(const ScratchNeed& cap) const;   // "" or the first region that does not fit, for an error message
};
constexpr size_t ScratchNeed::* kRegion[5] = {&ScratchNeed::t1, &ScratchNeed::t2, &ScratchNeed::halo, &ScratchNeed::wt, &ScratchNeed::dw};
constexpr const char* kRegionName[5] = {"S_T1", "S_T2", "S_halo", "S_wt", "S_dw"};
inline void ScratchNeed::merge(const ScratchNeed& o) { for (auto r : kRegion) this->*r = std::max(this->*r, o.*r); }
inline std::string ScratchNeed::misfit(const ScratchNeed& cap) const {
    for (int i = 0; i < 5; ++i)
        if (this->*kRegion[i] > cap.*kRegion[i])
            return std::string(kRegionName[i]) + " needs " + std::to_string(this->*kRegion[i]) + " floats and has " + std::to_string(cap.*kRegion[i]);
    return "";
}

// the SOCCDPT_ROUTE_WGRAD_* paths; Im2colGen: conv_gen_bwd's im2col^T at any stride (same route bit as Im2colT)
enum class WgradPath { None, TN, Transpose, X3Shift, Im2colT, HaloShift, Im2colGen };

// What a call asks for.  (reuse_xt changes no number: the staged copy it reuses is counted either way.)
struct PlanReq {
    bool dX, dW;
    bool staged_w;   // the dgrad weight operand waits in Tape::WT: S_wt stays unused
    bool defer;      // the weight-gradient sum may wait for the batched launch (Ctx::may_defer): a TN 3x3 gradient then skips S_dw
};

struct LinearPlan {
    OpFmt fmt;        // the amp mode's format where the shapes permit it, exact f32 otherwise
    WgradPath wgrad;
    size_t Mtn;       // TN: rows of dY (S_T1) and X (S_T2) with the zero rows appended
    int Mp;           // Transpose: row stride of dY^T [N][Mp] (S_T1) and X^T [K][Mp] (S_T2)
    ScratchNeed need;
};

// y = x W^T backward: dY [M][N], X [M][K], W [N][K]
inline LinearPlan plan_linear(size_t M, int N, int K, OpFmt mode, PlanReq q) {
    LinearPlan p{};
    const bool fits = mode == OpFmt::X3 ? N % 32 == 0 && K % 32 == 0 && K > 32 : N % 32 == 0 && K % 4 == 0 && K > 32;
    p.fmt = fits ? mode : OpFmt::F32;
    p.Mtn = roundup(M, 64);
    p.Mp = (int)roundup(M, op_is16(p.fmt) ? 128 : 32);
    const bool tn = p.fmt != OpFmt::F32 && q.dW && tr_wgrad_tn_ok(p.Mtn, N, K, 1);
    p.wgrad = !q.dW ? WgradPath::None : tn ? WgradPath::TN : WgradPath::Transpose;
    if (tn) {   // one launch converts both operands; dY serves the dgrad too
        p.need.t1 = op_floats(p.Mtn * N + kTnOverread, p.fmt);
        p.need.t2 = op_floats(p.Mtn * K + kTnOverread, p.fmt);
    } else {
        if (q.dX && p.fmt != OpFmt::F32) p.need.t1 = op_floats(M * N, p.fmt);
        if (q.dW) {
            p.need.t1 = std::max(p.need.t1, op_floats((size_t)N * p.Mp, p.fmt));
            p.need.t2 = op_floats((size_t)K * p.Mp, p.fmt);
        }
    }
    if (q.dX && !q.staged_w) p.need.wt = op_floats((size_t)N * K, p.fmt);   // W^T [K][N]
    return p;
}

// 3x3 convolution backward over a zero-haloed input [B][r+2][r+2][C], dY [B*r*r][N].  Elements are of format fmt.
struct ConvPlan {
    OpFmt fmt;
    WgradPath wgrad;
    bool col2im;      // conv_gen_bwd, strided: dgrad as dcol = dY Wtap (S_T2) + col2im instead of the stride-1 convolution over S_halo
    int rp;           // r + 2: pixel pitch of the halo image
    size_t Kh, Kp;    // halo pixels B rp rp, and padded to the TN kernel's k-tile.  S_halo: the dY image [Kh][N], TN: + (Kp - Kh) zero rows
    size_t mrg;       // TN: zero rows in front of and behind X in S_T2: [mrg][Kh][Kp - Kh + mrg] rows of C
    int rpp;          // X3Shift: pixel pitch
    int Mh;           // X3Shift / HaloShift: pixels of the transposed image (B rp rpp / B rp rp)
    int margin;       // ... zero columns in front of the first pixel of every row
    int ld;           // ... row stride of dY^T [N][ld] (S_T1) and of every copy of X^T [C][ld] (S_T2) = K of the GEMM
    size_t head;      // ... zeroed elements in front of (X3Shift: and behind) each copy
    size_t copy;      // ... elements from one copy to the next
    int ncopies;      // ... 3 (X3Shift), 2 (HaloShift, 16-bit) or 1
    int Mp;           // Im2colT / Im2colGen: row stride of dY^T [N][Mp] (S_T1) and the im2col^T [9 C][Mp] (S_T2)
    ScratchNeed need;
};

inline size_t conv3_tn_rows(int B, int r) { return roundup((size_t)B * (r + 2) * (r + 2), 64); }   // K of the TN 3x3 weight gradient

namespace detail {
inline ConvPlan conv_base(int B, int r) {
    ConvPlan p{};
    p.rp = r + 2;
    p.Kh = (size_t)B * p.rp * p.rp;
    p.Kp = conv3_tn_rows(B, r);
    p.mrg = (size_t)p.rp + 1;
    return p;
}
inline void conv_tn(ConvPlan& p, int N, int C) {   // conv3_wgrad_tn
    p.wgrad = WgradPath::TN;
    p.need.halo = op_floats(p.Kp * N, p.fmt);
    p.need.t2 = op_floats((2 * p.mrg + p.Kp) * C, p.fmt);
}
}  // namespace detail

// y = conv3x3(Xhalo, W) backward, stride 1 / pad 1, W [N][C][3][3] (conv3_bwd)
inline ConvPlan plan_conv3(int B, int r, int N, int C, OpFmt mode, PlanReq q) {
    ConvPlan p = detail::conv_base(B, r);
    p.fmt = N % 32 == 0 && C % 32 == 0 ? mode : OpFmt::F32;
    const bool x3 = p.fmt == OpFmt::X3, amp = op_is16(p.fmt);
    const size_t M = (size_t)B * r * r, w = (size_t)9 * N * C;
    if (q.dX) {
        p.need.halo = op_floats(p.Kh * N, p.fmt);
        if (!q.staged_w) p.need.wt = op_floats(w, p.fmt);   // rotated filter [C][9][N]
    }
    if (!q.dW) return p;
    if (p.fmt != OpFmt::F32 && tr_wgrad_tn_ok(p.Kp, N, C, 9)) {
        detail::conv_tn(p, N, C);
        if (!q.defer) p.need.dw = w;   // tap-major, permuted at once
        return p;
    }
    p.need.dw = w;   // the GEMM's tap-major output, permuted at once
    if (x3 && C % 64 == 0) {
        p.wgrad = WgradPath::X3Shift;
        p.rpp = (int)roundup(p.rp, 16);
        p.Mh = B * p.rp * p.rpp;
        p.margin = p.rpp + 16;
        p.ld = (int)roundup(2 * (size_t)p.margin + p.Mh, 32);
        p.head = (size_t)p.rpp + 16;
        p.copy = (size_t)C * p.ld + 2 * p.head;
        p.ncopies = 3;
    } else if (C % 64 != 0 || x3 || (amp && p.rp % 2 != 0)) {   // (layer1_rn of tiny_256, C = 96: a weight tile would straddle two taps)
        p.wgrad = WgradPath::Im2colT;
        p.Mp = (int)roundup(M, amp ? 128 : 32);
        p.need.t1 = op_floats((size_t)N * p.Mp, p.fmt);
        p.need.t2 = op_floats((size_t)9 * C * p.Mp, p.fmt);
        return p;
    } else {
        p.wgrad = WgradPath::HaloShift;
        p.Mh = (int)p.Kh;
        p.margin = r + 3;
        p.ld = (int)roundup(2 * (size_t)p.margin + p.Mh, 128);
        p.head = (size_t)(p.margin + 13) / 8 * 8;   // the most negative shift reads base - (r + 4)
        p.copy = (size_t)(C + 1) * p.ld + 64 + p.head;
        p.ncopies = amp ? 2 : 1;
    }
    p.need.t1 = op_floats((size_t)N * p.ld, p.fmt);
    p.need.t2 = op_floats(p.ncopies * p.copy, p.fmt);
    return p;
}

// 3x3 convolution backward with tap-major weights [N][9][C] over [B][Hi+2][Hi+2][C], output Ho x Ho (conv_gen_bwd).  The 16-bit modes take the
// un-strided convolutions of TN shape the way conv3_bwd does; everything else runs in f32.
inline ConvPlan plan_conv_gen(int B, int Hi, int Ho, int N, int C, int stride, int pad, OpFmt mode, PlanReq q) {
    ConvPlan p = detail::conv_base(B, Ho);
    const bool s1 = stride == 1 && pad == 1;
    const size_t Mo = (size_t)B * Ho * Ho, w = (size_t)9 * N * C;
    p.fmt = op_is16(mode) && s1 && Hi == Ho && tr_wgrad_tn_ok(p.Kp, N, C, 9) ? mode : OpFmt::F32;
    p.col2im = !s1;
    if (p.fmt != OpFmt::F32) {
        p.need.halo = op_floats(p.Kh * N, p.fmt);
        if (q.dX) { p.need.dw = w; p.need.wt = op_floats(w, p.fmt); }   // the rotated filter in f32 (S_dw), then converted (S_wt)
        if (q.dW) detail::conv_tn(p, N, C);
        return p;
    }
    if (q.dX) {
        p.need.wt = w;   // the rotated filter [C][9][N], or Wtap^T [9 C][N]
        if (s1) p.need.halo = p.Kh * N;
        else p.need.t2 = Mo * 9 * C;   // dcol [Mo][9][C]
    }
    if (q.dW) {
        p.wgrad = WgradPath::Im2colGen;
        p.Mp = (int)roundup(Mo, 32);
        p.need.t1 = (size_t)N * p.Mp;
        p.need.t2 = std::max(p.need.t2, (size_t)9 * C * p.Mp);
    }
    return p;
}

// Forward GEMM of the train-mode step (gemm_fwd): in any amp mode the operands are converted to x3 into S_T2 (X) and S_wt (W), shapes permitting
struct FwdPlan {
    bool x3;
    ScratchNeed need;
};
inline FwdPlan plan_gemm_fwd(size_t x_elems, size_t w_elems, OpFmt mode, bool desc_ok) {   // desc_ok: the descriptor's own conditions (gemm_fwd)
    FwdPlan p{};
    p.x3 = mode != OpFmt::F32 && desc_ok && x_elems % 16 == 0 && w_elems % 16 == 0;
    if (p.x3) { p.need.t2 = x_elems; p.need.wt = w_elems; }
    return p;
}

}  // namespace trn
}  // namespace soccdpt
