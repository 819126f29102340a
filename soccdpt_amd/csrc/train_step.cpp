// Training step of SOccDPT_V3 (Swin-V2 encoders here, the ViT-hybrid encoder in train_hybrid_step.cpp; decoder and heads shared): train-mode
// forward that keeps every activation the backward needs (the "tape"),
// and the backward that autograd runs for the reference (scripts/train_SOccDPT.py:360-393 over model/SOccDPT.py:660-685, model/dpt.py:142-232,
// model/blocks.py:391-497 and timm's SwinTransformerV2).  Arithmetic by soccdpt_train_set_amp: 0 = exact f32 (every GEMM-shaped gradient through the f32
// MFMA igemm), 3 = x3 split-fp16 operands in every GEMM of the step (f32-grade), 1 / 2 = bf16 / fp16 operands in the gradient GEMMs with an x3 forward;
// the tape, the weights and the gradients are f32 in every mode.  Weight gradients: split-K igemm over transposed operands (gemm_wgrad), or -- 16-bit and x3
// modes, shapes permitting -- from the operands as stored (train_wgrad_tn.hip).  Attention backward: train_attn.hip.  The rest: train.hip.
// Train mode differs from eval in the seg head (model/SOccDPT.py:660-671: BatchNorm2d on batch statistics with running-buffer updates, Dropout(0.1) live)
// and in the encoder's stochastic depth (timm's drop_path_rate = 0.1, soccdpt_train_set_drop_path).
//
// Gradients are WRITTEN (not accumulated) to the buffers bound with soccdpt_bind_grad; a weight without a bound gradient is frozen and its
// weight-gradient GEMM is skipped (the reference freezes / partially unfreezes the encoder: model/loss.py:110-152).
#include <cstdio>

#include "train_internal.h"

#include <cstring>
#include <memory>

namespace soccdpt {
namespace trn {

// One walk decides the layout; with base == nullptr it only measures.
void carve(const Handle& h, int B, TArena& ar, Tape& T) {
    const Arch& a = h.arch;
    const int F = h.cfg.features, G = a.grid();
    const size_t M0 = (size_t)B * G * G;
    auto halo = [&](int r, int C) { return ar.f((size_t)B * (r + 2) * (r + 2) * C); };
    // ---- halo zone ----
    ar.f(0);
    T.halo_lo = (ar.off + 255) & ~size_t(255);
    for (int l = 0; l < 4; ++l) {
        const int r = a.fres(l);
        T.feat[l] = halo(r, a.fdim(l));
        T.lrn_relu[l] = halo(r, F);
        T.t1[l] = l < 3 ? halo(r, F) : nullptr;
        T.out_relu[l] = l < 3 ? halo(r, F) : nullptr;
        T.t2[l] = halo(r, F);
    }
    const int r1 = 2 * a.fres(0), r0 = 4 * a.fres(0);
    T.path1 = halo(r1, F);
    T.d1u = halo(r0, F / 2);
    T.sk_count = reinterpret_cast<unsigned*>(ar.f(kTrainSkCountWords));   // split-K arrival counters: zero at rest (zeroed with the halos)
    if (a.hybrid) hy_carve_halo(h, B, ar, T);
    ar.f(0);
    T.halo_hi = (ar.off + 255) & ~size_t(255);
    size_t maxAct = M0 * 64;
    size_t maxDS = 0, maxStat = 0, maxTab = 0, maxPart = 0;
    if (a.hybrid) hy_carve(h, B, ar, T, maxAct);
    else {
    // ---- encoder tape ----
    T.patches = ar.f(M0 * 64);
    T.pe_wpad = ar.f((size_t)a.embed * 64);
    T.pe_pre = ar.f(M0 * a.embed);
    T.x0 = ar.f(M0 * a.embed);
    for (int s = 0; s < 4; ++s) {
        const int C = a.dim(s), res = a.res(s), H = a.heads[s], ws = a.ws(s);
        const size_t M = (size_t)B * res * res;
        T.blk[s].assign(a.depths[s], BlkT{});
        for (int j = 0; j < a.depths[s]; ++j) {
            BlkT& b = T.blk[s][j];
            b.qkv_bias = ar.f(3 * C);
            b.scale = ar.f(H);
            b.table = ar.f((size_t)(2 * ws - 1) * (2 * ws - 1) * H);
            b.bias_acc = ar.f(attn_bias_elems(ws, H));
            b.dp = ar.f(2 * (size_t)B + 2);
            b.qkv = ar.f(M * 3 * C);
            b.attn = ar.f(M * C);
            b.a_pre = ar.f(M * C);
            b.x1 = ar.f(M * C);
            b.hpre = ar.f(M * 4 * C);
            b.hact = ar.f(M * 4 * C);
            b.m_pre = ar.f(M * C);
            b.xout = ar.f(M * C);
        }
        maxAct = std::max(maxAct, M * 4 * C);
        const size_t nwin = (size_t)B * (res / ws) * (res / ws), N = (size_t)ws * ws;
        maxDS = std::max(maxDS, nwin * H * N * N);
        maxStat = std::max(maxStat, nwin * H * N * 2);
        maxPart = std::max(maxPart, nwin * H * (size_t)tr_attention_bwd_mfma_slots(ws));
        maxTab = std::max(maxTab, (size_t)(2 * ws - 1) * (2 * ws - 1) * H);
        if (s < 3) {
            T.mg[s] = ar.f(M * C);            // [M/4][4C]
            T.mr_pre[s] = ar.f(M / 4 * 2 * C);
            T.mx[s] = ar.f(M / 4 * 2 * C);
        }
    }
    }
    // ---- decoder tape ----
    for (int l = 0; l < 4; ++l) {
        const size_t M = (size_t)B * a.fres(l) * a.fres(l);
        T.lrn_raw[l] = ar.f(M * F);
        T.out_raw[l] = l < 3 ? ar.f(M * F) : nullptr;
        T.u[l] = ar.f(M * F);
        T.oc[l] = ar.f(M * F);
        T.w_lrn[l] = ar.f((size_t)F * 9 * a.fdim(l));
        for (int u = 0; u < 2; ++u)
            for (int c = 0; c < 2; ++c) T.w_rcu[l][u][c] = ar.f((size_t)F * 9 * F);
        maxAct = std::max(maxAct, M * F);
    }
    const size_t M1 = (size_t)B * r1 * r1, M0p = (size_t)B * r0 * r0;
    T.d1 = ar.f(M1 * (F / 2));
    T.e = ar.f(M0p * 32);
    T.inv = ar.f(M0p);
    T.seg = ar.f(M0p * 3);
    T.w_d0 = ar.f((size_t)(F / 2) * 9 * F);
    T.w_d2 = ar.f((size_t)32 * 9 * (F / 2));
    T.w_s0 = ar.f((size_t)F * 9 * F);
    T.c_raw = ar.f(M1 * F);
    T.bn_stats = ar.f(2 * F);
    T.r = ar.f(M1 * F);
    T.logits = ar.f(M1 * 4);
    T.keep = reinterpret_cast<uint8_t*>(ar.f((M1 * F + 3) / 4));
    maxAct = std::max(maxAct, std::max(M1 * F, M0p * (size_t)(F / 2)));
    maxAct = std::max(maxAct, M0p * 33);
    T.maxAct = maxAct;
    // ---- backward scratch ----
    const size_t Cmax0 = a.hybrid ? 1024 : (size_t)a.dim(3);
    for (auto& g : T.G) g = ar.f(maxAct);
    T.GX = ar.f(a.hybrid ? 64 : M0 * a.embed);   // the largest token-stream gradient (stage 0; later stages are smaller)
    T.GP = ar.f(M1 * F);
    T.DOC = ar.f((size_t)B * a.fres(0) * a.fres(0) * F);
    for (int l = 0; l < 4; ++l) T.DF[l] = ar.f((size_t)B * a.fres(l) * a.fres(l) * a.fdim(l));
    const size_t Cmax = a.hybrid ? 1024 : a.dim(3);
    const size_t wmax = std::max(std::max((size_t)9 * F * F, 4 * Cmax * Cmax), a.hybrid ? (size_t)9 * 768 * 768 : 0);
    ScratchNeed& cap = T.S_cap;   // hand-derived maxima over the network's layers; every helper checks its plan against them (check_fit)
    cap.t1 = maxAct + 128 * 4 * Cmax0;
    cap.t2 = std::max(std::max(M1 * 9 * F, M0p * 9 * (size_t)(F / 2)), maxAct) + 128 * 9 * Cmax0;
    cap.halo = std::max((size_t)B * (r1 + 2) * (r1 + 2) * F, (size_t)B * (r0 + 2) * (r0 + 2) * (size_t)(F / 2)) + 64 * (size_t)F;   // + the k-tile padding rows of train_wgrad_tn.hip
    cap.wt = cap.dw = wmax;
    T.S_T1 = ar.f(cap.t1);
    T.S_T2 = ar.f(cap.t2);
    T.S_halo = ar.f(cap.halo);
    T.S_wt = ar.f(cap.wt);
    T.S_dw = ar.f(cap.dw);
    T.S_col = ar.f((size_t)1 << 20);
    {   // slots of the staged dgrad weight operands (stage_weights): Linear [N][K] and 1x1 conv weights with N, K multiples of 32 and K > 32, 3x3 conv weights with N, C multiples of 32
        T.wt_off.assign(h.weights.size(), -1);
        size_t tot = 0;
        for (size_t i = 0; i < h.weights.size(); ++i) {
            const auto& sh = h.weights[i].shape;
            if (wt_slot_kind(sh.data(), sh.size()) < 0) continue;
            T.wt_off[i] = (long long)tot;
            tot += (h.weights[i].numel() + 63) & ~size_t(63);
        }
        T.WT = ar.f(tot);
    }
    T.sk_part = ar.f(kTrainSkPartFloats);
    T.tn_arena = ar.f(kTrainTnArenaFloats);
    T.S_vec = ar.f(std::max((size_t)4 * Cmax, (size_t)4 * F) * 2);
    T.dS = ar.f(maxDS);
    T.rowstat = ar.f(maxStat);
    T.dscale_part = ar.f(maxPart);
    T.dtable = ar.f(maxTab);
    T.dt = ar.f(maxTab);
    T.S_cpb = ar.f(a.hybrid ? 64 : (size_t)2 * (2 * a.window - 1) * (2 * a.window - 1) * 512);
}

// A GEMM over operands of format fmt (f32 outputs).  X3: three fp16 MFMAs per product, f32-grade results; same tile set and split-K decisions
// as the exact-f32 GEMMs.  BF16 / F16: the igemm's own 16-bit tiles.
int gemm(Ctx& c, IgemmDesc d, OpFmt fmt) {
    d.f32 = fmt == OpFmt::F32 ? 1 : 0;
    d.x3 = fmt == OpFmt::X3 ? 1 : 0;
    d.f16 = op_igemm_f16(fmt);
    if (op_is16(fmt)) return launch_igemm(d, c.st, c.err);
    // Small grids with a long K (coarse decoder levels, stage-3 Linear layers, their dgrads): split K like the weight-gradient GEMMs do
    const long tiles = (long)((d.M + 63) / 64) * ((d.N + 63) / 64);
    const long nk = (long)d.taps * d.Cin / 32;
    if (tiles <= 96 && nk >= 48 && !d.ln_g && !d.gn_stats && !d.out_dot && d.stride == 1 && d.pad == 1 && d.in_halo == 1 && !d.Hi && !d.gather1 && !d.grp_rows &&
        (size_t)tiles <= kTrainSkCountWords) {
        long S = (256 + tiles - 1) / tiles;
        if (S > nk / 8) S = nk / 8;
        if (S > 16) S = 16;
        while (S > 1 && (size_t)S * d.M * d.N > kTrainSkPartFloats) --S;
        if (S > 1) {
            d.splitk = (int)S; d.sk_part = c.T.sk_part; d.sk_count = c.T.sk_count; d.sk_part_floats = kTrainSkPartFloats; d.sk_count_words = kTrainSkCountWords;
            c.path |= SOCCDPT_ROUTE_DGRAD_SPLITK;
        }
    }
    return launch_igemm(d, c.st, c.err);
}

int cvt_op(Ctx& c, const float* in, void* out, size_t n, OpFmt fmt) {
    if (fmt == OpFmt::F32) { c.err = "cvt_op: f32 operands are used as stored"; return 1; }
    return launch_cvt_bf16(in, static_cast<bf16_t*>(out), n, op_cvt_hf(fmt), c.st, c.err);   // fp16: IEEE conversion, an overflow of the scaled gradient becomes inf
}

// Forward GEMM.  With any train amp mode (the 16-bit modes too: their forward stays f32-grade, so the ReLU masks are those of the f32 step) the operands -- f32 tape tensors and f32 (tap-major) weights -- are converted to the x3 split-fp16
// format into backward scratch (S_T2 / S_wt, idle during the forward) and the product runs as three fp16 MFMAs per k-step; everything the launch
// writes stays f32 (out_f32, and out_op as an f32 tensor: out_op_f32), so the tape and the backward are unchanged.  x_elems / w_elems: elements of
// the X buffer (a halo image counts its border) and of the weight matrix.
int gemm_fwd(Ctx& c, IgemmDesc d, size_t x_elems, size_t w_elems) {
    const FwdPlan p = plan_gemm_fwd(x_elems, w_elems, amp_fmt(c), d.Cin % 32 == 0 && (d.taps == 9 || d.ldx % 16 == 0) && !d.ln_g && !d.grp_rows && !d.gather1 &&
                                                                      d.stride == 1 && d.pad == 1 && d.in_halo == 1);
    if (!p.x3) return gemm(c, d);
    TRY(check_fit(c, "gemm_fwd", p.need));
    TRY(tr_cvt_pair(static_cast<const float*>(d.X), c.T.S_T2, x_elems, static_cast<const float*>(d.Wt), c.T.S_wt, w_elems, OpFmt::X3, c.st, c.err));
    d.X = c.T.S_T2; d.Wt = c.T.S_wt; d.out_op_f32 = 1;
    return gemm(c, d, OpFmt::X3);
}

// Weight-gradient GEMM over TRANSPOSED operands: few output tiles, K = pixels.  Split K so that about two workgroups per CU exist; the partial tiles are
// summed in split order -- by a second launch (sk_defer) for the big tiles and for >= 4 splits, by the last workgroup to arrive otherwise: deterministic
// either way.  fmt: what the CALLER's staging kernels wrote (the amp mode applies per GEMM: shapes that do not fit stay f32); 16-bit operands have K padded
// to 128 by the caller.
int gemm_wgrad(Ctx& c, IgemmDesc d, OpFmt fmt) {
    const bool amp = op_is16(fmt), x3 = fmt == OpFmt::X3;
    d.f32 = fmt == OpFmt::F32 ? 1 : 0;
    d.x3 = x3 ? 1 : 0;
    d.f16 = op_igemm_f16(fmt);
    // Tiles.  Default for the wide layers (M, N multiples of 128, >= 8 tiles): the 8-wave 128 x 128 tile -- these launches are L2 -> LDS fill bound and it
    // carries 64 FLOP per staged byte (16-bit) against 21 for 32 x 64 -- with the DEFERRED reduction (igemm.h sk_defer).  Rounds 2 and early 3 measured
    // the big tiles slower (f32 4 waves 51.2 vs 45.2 ms, x3 37.5 vs 36.6 ms per step): that was the last-arriver reduction, one workgroup walking 14
    // partial tiles of 64 KB with L2-bypassing loads (~400 us per launch).  The other shapes keep the small tiles.
    long tiles = amp ? (long)((d.M + 31) / 32) * ((d.N + 63) / 64) : (long)((d.M + 63) / 64) * ((d.N + 63) / 64);
    long nk = (long)d.taps * d.Cin / (amp ? 128 : 32);
    const bool big = d.M % 128 == 0 && d.N % 128 == 0 && d.Cin % 64 == 0 && (long)(d.M / 128) * (d.N / 128) >= 8 &&
                     (!d.wt_grp_rows || d.wt_grp_rows % 128 == 0);
    if (big) {
        d.tune = amp ? 46 : 3;
        tiles = (long)(d.M / 128) * (d.N / 128);
        nk = (long)d.taps * d.Cin / (amp ? 64 : 32);
    }
    long S = (512 + tiles - 1) / tiles;
    if (x3 || big) S = 512 / tiles > 0 ? 512 / tiles : 1;   // fill-bound at two workgroups per CU: at most ONE round of them (576 workgroups = 1.125 rounds cost 1 ms per step)
    if (S > nk / (amp ? 2 : 8)) S = nk / (amp ? 2 : 8);
    if (S > 64) S = 64;
    while (S > 1 && (size_t)S * d.M * d.N > kTrainSkPartFloats) --S;
    if (S > 1 && (size_t)tiles <= kTrainSkCountWords) {
        d.splitk = (int)S; d.sk_part = c.T.sk_part; d.sk_count = c.T.sk_count; d.sk_part_floats = kTrainSkPartFloats; d.sk_count_words = kTrainSkCountWords;
        if ((big || S >= 4) && d.N % 4 == 0) d.sk_defer = 1;   // many splits: sum them in a second chip-wide launch instead of in the last workgroup
        c.path |= (big ? SOCCDPT_ROUTE_WGRAD_BIG_TILE : 0u) | (d.sk_defer ? SOCCDPT_ROUTE_WGRAD_SK_DEFER : 0u);
    } else if (big) {
        d.tune = -1;
    }
    return launch_igemm(d, c.st, c.err);
}

int copy_d2d(Ctx& c, void* dst, const void* src, size_t bytes, const char* what) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c.st);
    if (e != hipSuccess) { c.err = std::string(what) + ": " + hipGetErrorString(e); return 1; }
    return 0;
}

int wt_slot_kind(const int64_t* sh, size_t ndim) {
    const bool lin = (ndim == 2 || (ndim == 4 && sh[2] == 1 && sh[3] == 1)) && sh[0] % 32 == 0 && sh[1] % 32 == 0 && sh[1] > 32;
    const bool c3 = ndim == 4 && sh[2] == 3 && sh[3] == 3 && sh[0] % 32 == 0 && sh[1] % 32 == 0;
    return lin ? 0 : c3 ? 1 : -1;
}

int stage_weight_list(Ctx& c, const std::vector<WtStage>& list) {
    Tape& T = c.T;
    T.wt_by_ptr.clear();
    if (!T.WT) return 0;
    const OpFmt fmt = amp_fmt(c);
    TrBatchTable t;
    t.n = 0;
    int tiles = 0;
    auto flush = [&]() -> int {
        if (t.n) TRY(tr_weight_batch(t, tiles, fmt, c.st, c.err));
        t.n = 0;
        tiles = 0;
        return 0;
    };
    for (const WtStage& w : list) {
        TrBatchEntry& e = t.e[t.n++];
        e.src = w.src;
        e.dst = T.WT + w.off;
        e.R = w.R;
        e.C = w.C;
        e.kind = w.kind;
        e.tile0 = tiles;
        tiles += e.kind ? (int)(((size_t)e.R * e.C * 9 + 1023) / 1024) : ((e.C + 31) / 32) * ((e.R + 31) / 32);
        T.wt_by_ptr[w.src] = w.off;
        if (t.n == kTrBatchMax) TRY(flush());
    }
    return flush();
}

int stage_weights(Ctx& c) {
    std::vector<WtStage> list;
    for (size_t i = 0; i < c.h.weights.size() && c.T.WT; ++i) {
        const auto& w = c.h.weights[i];
        if (c.T.wt_off[i] < 0 || !w.ptr) continue;
        list.push_back(WtStage{w.ptr, c.T.wt_off[i], (int)w.shape[0], (int)w.shape[1], (w.shape.size() == 4 && w.shape[2] == 3) ? 1 : 0});
    }
    return stage_weight_list(c, list);
}

const void* staged_wt(const Ctx& c, const float* W) {
    const auto it = c.T.wt_by_ptr.find(W);
    return it == c.T.wt_by_ptr.end() ? nullptr : static_cast<const void*>(c.T.WT + it->second);
}

// y = x W^T + b backward.  dY [M][N], X [M][K], W [N][K].  dX_out = dY W (+ dX_res); dW = dY^T X; db = colsum(dY).
int linear_bwd(Ctx& c, const float* dY, const float* X, const float* W, size_t M, int N, int K, float* dX_out, const float* dX_res, float* dW, float* db) {
    Tape& T = c.T;
    // The operand format of the layer's two gradient GEMMs: the amp mode's where the shapes permit it (x3: f32-grade, 4 bytes per element), exact f32 otherwise.
    // Weight gradient from the operands as stored (train_wgrad_tn.hip) where it can be: no transposes.  Token counts that are not a k-tile multiple (577-token
    // ViT sequences) get zero rows appended to both operands (zero bytes are x3 zeros too).
    const LinearPlan p = plan_linear(M, N, K, amp_fmt(c), PlanReq{dX_out != nullptr, dW != nullptr, staged_wt(c, W) != nullptr, false});
    TRY(check_fit(c, "linear_bwd", with_dw_target(T, p.need, dW, (size_t)N * K)));
    const OpFmt fmt = p.fmt;
    const size_t es = op_size(fmt), Mtn = p.Mtn;
    const bool tn = p.wgrad == WgradPath::TN;
    c.path |= route_fmt_bit(fmt) | route_wgrad_bit(p.wgrad);
    // Both operand conversions of the layer go in ONE launch then: dY for the two gradient GEMMs, X for the weight gradient (round 5; two launches of a
    // scalar kernel per layer before).  tr_wgrad_tn_ok's N, K % 32 == 0 give tr_cvt_pair the element counts it needs.
    char* const yS = reinterpret_cast<char*>(T.S_T1);   // dY and X in the launch format
    char* const xS = reinterpret_cast<char*>(T.S_T2);
    // a gradient written into scratch (standardised ResNetV2 kernels, the padded patch embedding) is read by its caller's next launch: summed at once; parameter gradients wait for the batched sum
    TnDefer* const df = c.may_defer(dW, db) ? &c.tn : nullptr;   // (the qkv bias gradient, e.g., goes through scratch into q_bias / v_bias)
    if (tn) TRY(tr_cvt_pair(dY, yS, M * N, X, xS, M * K, fmt, c.st, c.err));
    if (dX_out) {
        IgemmDesc d;
        d.M = (int)M; d.N = K; d.Cin = N; d.ldx = N; d.res1 = dX_res; d.out_f32 = dX_out;
        d.Wt = staged_wt(c, W);
        c.path |= d.Wt ? SOCCDPT_ROUTE_W_STAGED : SOCCDPT_ROUTE_W_FALLBACK;
        if (!d.Wt) { TRY(tr_transpose(W, T.S_wt, fmt, N, K, N, c.st, c.err)); d.Wt = T.S_wt; }   // [K][N]
        if (fmt != OpFmt::F32 && !tn) TRY(cvt_op(c, dY, yS, M * N, fmt));
        d.X = fmt == OpFmt::F32 ? static_cast<const void*>(dY) : yS;
        TRY(gemm(c, d, fmt));
    }
    if (tn) {
        c.path |= df ? SOCCDPT_ROUTE_SUM_DEFERRED : SOCCDPT_ROUTE_SUM_IMMEDIATE;
        if (Mtn > M) {
            hipError_t e = hipMemsetAsync(yS + M * N * es, 0, (Mtn - M) * N * es, c.st);
            if (e == hipSuccess) e = hipMemsetAsync(xS + M * K * es, 0, (Mtn - M) * K * es, c.st);
            if (e != hipSuccess) { c.err = std::string("linear_bwd memset: ") + hipGetErrorString(e); return 1; }
        }
        // (the bias gradient = column sums of dY rides in the same launch: one more MFMA per fragment against ones, train_wgrad_tn.hip)
        TRY(tr_wgrad_tn(yS, N, xS, K, Mtn, N, K, 1, 0, fmt, T.sk_part, kTrainSkPartFloats, dW, c.st, c.err, db, df));
        db = nullptr;
    } else if (dW) {
        const int Mp = p.Mp;   // k-tile multiple; the padding rows are zero
        TRY(tr_transpose(dY, yS, fmt, (int)M, N, Mp, c.st, c.err));   // [N][Mp]
        TRY(tr_transpose(X, xS, fmt, (int)M, K, Mp, c.st, c.err));    // [K][Mp]
        IgemmDesc d;
        d.X = yS; d.Wt = xS; d.M = N; d.N = K; d.Cin = Mp; d.ldx = Mp; d.out_f32 = dW;
        TRY(gemm_wgrad(c, d, fmt));
    }
    if (db) TRY(tr_colsum(dY, nullptr, db, T.S_col, M, N, 0, c.st, c.err));
    return 0;
}

// dY [B*r*r][N] as the zero-bordered image [B][r+2][r+2][N] of format fmt in S_halo: the X operand of the stride-1 / pad-1 dgrad (conv3_dgrad_s1) and the
// A operand of conv3_wgrad_tn
int conv3_dy_halo(Ctx& c, const float* dY, int r, int N, OpFmt fmt) {
    return tr_to_halo_full(dY, c.T.S_halo, fmt, c.B, r, r, N, c.st, c.err);   // writes the zero border itself; N % 8 == 0 (every reader needs N % 32 == 0: the dgrad GEMM's K, the TN kernel's tiles)
}

// Stride-1 / pad-1 dgrad: dX_out [B*r*r][C] = conv3x3(the dY image in S_halo, Wrot) (+ dX_res), the forward's implicit GEMM over the rotated filter
// Wrot [C][9][N] in format fmt
int conv3_dgrad_s1(Ctx& c, const void* Wrot, int r, int N, int C, OpFmt fmt, float* dX_out, const float* dX_res) {
    IgemmDesc d;
    d.M = c.B * r * r; d.N = C; d.Cin = N; d.taps = 9; d.H = r; d.W = r; d.res1 = dX_res; d.out_f32 = dX_out;
    d.X = c.T.S_halo; d.Wt = Wrot;
    return gemm(c, d, fmt);
}

// Weight gradient of a stride-1 / pad-1 3x3 convolution from the operands as stored, in halo pixel order (train_wgrad_tn.hip; shapes: tr_wgrad_tn_ok over
// conv3_tn_rows): A = the dY image of conv3_dy_halo in S_halo, B = the input's halo image converted to the operand format into S_T2; tap (ky, kx) reads B
// (ky - 1)(r + 2) + (kx - 1) rows further on.  K is padded to a k-tile with zero rows of A; B gets zero margins of ConvPlan::mrg rows on both sides (border
// pixels of A are zero, but 0 * NaN is not).  reuse_xt: B is left as it is when S_T2 still holds Xhalo's copy (Tape::xt_tn_src).  bias: the column sums of dY ride in the
// launch (its zero border adds nothing).  param_layout: `out` is a bound gradient [N][C][3][3] that the batched sum of this pass writes (Ctx::may_defer holds);
// otherwise `out` receives the kernel's tap-major [N][9][C] at once.
int conv3_wgrad_tn(Ctx& c, const ConvPlan& p, const float* Xhalo, int N, int C, bool reuse_xt, float* out, float* bias, bool param_layout) {
    Tape& T = c.T;
    const OpFmt fmt = p.fmt;
    const size_t es = op_size(fmt);
    char* const hS = reinterpret_cast<char*>(T.S_halo);
    char* const xS = reinterpret_cast<char*>(T.S_T2);
    const size_t Kh = p.Kh, Kp = p.Kp, mrg = p.mrg;
    hipError_t e = Kp > Kh ? hipMemsetAsync(hS + Kh * N * es, 0, (Kp - Kh) * N * es, c.st) : hipSuccess;
    if (!reuse_xt || T.xt_tn_src != Xhalo) {
        T.xt_tn_src = Xhalo;
        if (e == hipSuccess) e = hipMemsetAsync(xS, 0, mrg * C * es, c.st);
        if (e == hipSuccess) e = hipMemsetAsync(xS + (mrg + Kh) * C * es, 0, (Kp - Kh + mrg) * C * es, c.st);
        if (e == hipSuccess) TRY(cvt_op(c, Xhalo, xS + mrg * C * es, Kh * C, fmt));
    }
    if (e != hipSuccess) { c.err = std::string("conv3_wgrad_tn memset: ") + hipGetErrorString(e); return 1; }
    return tr_wgrad_tn(hS, N, xS + mrg * C * es, C, Kp, N, C, 9, p.rp, fmt, T.sk_part, kTrainSkPartFloats, out, c.st, c.err, bias, param_layout ? &c.tn : nullptr,
                       param_layout ? C : 0);
}

// y = conv3x3(Xhalo, W) + b backward.  dY plain [B*r*r][N], Xhalo [B][r+2][r+2][C], W [N][C][3][3].
int conv3_bwd(Ctx& c, const float* dY, const float* Xhalo, const float* W, int r, int N, int C, float* dX_out, const float* dX_res, float* dW, float* db,
              bool reuse_xt) {
    Tape& T = c.T;
    const int B = c.B;
    const size_t M = (size_t)B * r * r;
    const bool defer = c.may_defer(dW, db);
    const ConvPlan p = plan_conv3(B, r, N, C, amp_fmt(c), PlanReq{dX_out != nullptr, dW != nullptr, staged_wt(c, W) != nullptr, defer});
    TRY(check_fit(c, "conv3_bwd", p.need));
    const OpFmt fmt = p.fmt;   // the amp mode's operand format where the shapes permit it
    const bool amp = op_is16(fmt);
    const size_t es = op_size(fmt);
    c.path |= route_fmt_bit(fmt) | route_wgrad_bit(p.wgrad);
    char* const yS = reinterpret_cast<char*>(T.S_T1);
    char* const xS = reinterpret_cast<char*>(T.S_T2);
    if (dX_out) {
        TRY(conv3_dy_halo(c, dY, r, N, fmt));
        const void* Wrot = staged_wt(c, W);
        c.path |= Wrot ? SOCCDPT_ROUTE_W_STAGED : SOCCDPT_ROUTE_W_FALLBACK;
        if (!Wrot) { TRY(tr_conv_w_dgrad(W, T.S_wt, fmt, N, C, c.st, c.err)); Wrot = T.S_wt; }   // [C][9][N], rotated
        TRY(conv3_dgrad_s1(c, Wrot, r, N, C, fmt, dX_out, dX_res));
    }
    if (p.wgrad == WgradPath::TN) {
        if (!dX_out) TRY(conv3_dy_halo(c, dY, r, N, fmt));   // (otherwise the image the dgrad launch staged)
        c.path |= defer ? SOCCDPT_ROUTE_SUM_DEFERRED : SOCCDPT_ROUTE_SUM_IMMEDIATE;
        if (defer) {   // the batched sum writes the parameter layout itself
            TRY(conv3_wgrad_tn(c, p, Xhalo, N, C, reuse_xt, dW, db, true));
        } else {
            TRY(conv3_wgrad_tn(c, p, Xhalo, N, C, reuse_xt, T.S_dw, db, false));
            TRY(tr_wgrad_permute(T.S_dw, dW, N, C, c.st, c.err));
        }
        db = nullptr;
    } else if (p.wgrad == WgradPath::Im2colT) {   // (layer1_rn of tiny_256, C = 96: a weight tile would straddle two taps) explicit im2col^T
        TRY(tr_transpose(dY, yS, fmt, (int)M, N, p.Mp, c.st, c.err));             // [N][Mp]
        TRY(tr_im2colT(Xhalo, xS, fmt, B, r, r, C, (size_t)p.Mp, c.st, c.err));   // [9C][Mp]
        IgemmDesc d;
        d.X = yS; d.Wt = xS; d.M = N; d.N = 9 * C; d.Cin = p.Mp; d.ldx = p.Mp; d.out_f32 = T.S_dw;
        TRY(gemm_wgrad(c, d, fmt));
        TRY(tr_wgrad_permute(T.S_dw, dW, N, C, c.st, c.err));
    } else if (dW) {
        // No im2col: both operands transposed in halo pixel order, tap (ky, kx) = the plain GEMM over a shifted view of the transposed halo image (train.hip:
        // dy_halo_T_kernel), ONE GEMM with M = N out-channels, N = 9 groups of C rows of the weight operand (one view per tap), K = ld halo-order pixels.
        // HaloShift (f32 and 16-bit): element shifts into one image, 16-bit a second copy for the odd ones.  X3Shift: pixel rows pitched to rpp and three
        // copies pre-shifted by -1 / 0 / +1 pixel (x_halo_T_kernel).  The layouts and their contracts: train_plan.h.
        const bool x3 = p.wgrad == WgradPath::X3Shift;
        TRY(tr_dy_halo_T(dY, yS, fmt, B, r, N, p.margin, p.ld, c.st, c.err, p.rpp));
        if (!reuse_xt || T.xt_tn_src) {
            T.xt_tn_src = nullptr;
            for (int cp = 0; cp < p.ncopies; ++cp) {
                char* base = xS + cp * p.copy * es;
                // the headroom (HaloShift: + the first row's left margin; every other gap is the zero tail of a row) and, X3Shift, the same behind the copy
                hipError_t e = hipMemsetAsync(base, 0, (p.head + (x3 ? 0 : p.margin)) * es, c.st);
                if (e == hipSuccess && x3) e = hipMemsetAsync(base + (p.head + (size_t)C * p.ld) * es, 0, p.head * es, c.st);
                if (e != hipSuccess) { c.err = std::string("conv3_bwd memset: ") + hipGetErrorString(e); return 1; }
                if (x3) TRY(tr_x_halo_T_x3(Xhalo, base + p.head * es, B, r, C, p.margin - (cp - 1), p.ld, p.rpp, c.st, c.err));
                else TRY(tr_transpose(Xhalo, base + (p.head + p.margin - cp) * es, fmt, p.Mh, C, p.ld, c.st, c.err));
            }
        }
        IgemmDesc d;
        d.X = yS; d.Wt = xS; d.M = N; d.N = 9 * C; d.Cin = p.ld; d.ldx = p.ld; d.out_f32 = T.S_dw;
        d.wt_grp_rows = C; d.wt_base = (int)p.head;
        if (x3) { d.wt_rp = p.rpp; d.wt_kx = (int)p.copy; }
        else { d.wt_rp = p.rp; d.wt_odd = amp ? (int)p.copy - 1 : 0; }   // 16-bit: taps with kx != 1 read copy 1 (x[k + 1] at k) so that every base stays 4-byte aligned
        TRY(gemm_wgrad(c, d, fmt));
        TRY(tr_wgrad_permute(T.S_dw, dW, N, C, c.st, c.err));
    }
    if (db) TRY(tr_colsum(dY, nullptr, db, T.S_col, M, N, 0, c.st, c.err));
    return 0;
}

// out = LN(y) g + b backward: d y -> dy; gamma / beta gradients
int ln_bwd_on(float* s_col, hipStream_t st, std::string& err, const float* y, const float* g, const float* dout, float* dy, float* xhat, size_t M, int C, float* dg,
              float* dbeta, float eps) {
    TRY(tr_ln_bwd(y, g, dout, dy, xhat, (int)M, C, eps, st, err));
    if (dg && dbeta) return tr_colsum2(dout, xhat, dg, dbeta, s_col, M, C, st, err);   // one pass over dout for both (same addition order as the single forms)
    if (dg) TRY(tr_colsum(dout, xhat, dg, s_col, M, C, 0, st, err));
    if (dbeta) TRY(tr_colsum(dout, nullptr, dbeta, s_col, M, C, 0, st, err));
    return 0;
}
int ln_bwd(Ctx& c, const float* y, const float* g, const float* dout, float* dy, float* xhat, size_t M, int C, float* dg, float* dbeta, float eps) {
    return ln_bwd_on(c.T.S_col, c.st, c.err, y, g, dout, dy, xhat, M, C, dg, dbeta, eps);
}

IgemmDesc conv_desc(const void* X, int Cin, const void* Wt, int N, int r, int B) {
    IgemmDesc d;
    d.X = X; d.Wt = Wt; d.M = B * r * r; d.N = N; d.Cin = Cin; d.taps = 9; d.H = r; d.W = r;
    return d;
}

bool any_grad(const Handle& h, Span s) {
    for (int i = s.lo; i < s.hi; ++i)
        if (h.weights[i].grad) return true;
    return false;
}

// the backward kernels are instantiated and tested for these three models' widths; a wider Swin-V2 (dpt_swin2_large_384: 1536 channels, 48 heads) runs the forward path only
static bool train_backbone_ok(const Handle& h) {
    return h.cfg.backbone == SOCCDPT_BACKBONE_SWIN2T16_256 || h.cfg.backbone == SOCCDPT_BACKBONE_SWIN2B24_384 || h.cfg.backbone == SOCCDPT_BACKBONE_VITB_RN50_384;
}

int check_train(Handle& h, int B, const void* ws, size_t ws_bytes, std::string& err) {
    if (h.cfg.precision != SOCCDPT_PREC_F32) { err = "soccdpt_train_*: the training step is built for SOCCDPT_PREC_F32 handles only"; return 1; }
    if (h.arch.hybrid && h.arch.grid() != 24) { err = "soccdpt_train_*: the ViT-hybrid encoder trains at 384 x 384 (position embedding used as stored)"; return 1; }
    if (h.cfg.features != 256 || h.cfg.num_classes != 3) { err = "soccdpt_train_*: features must be 256 and num_classes 3"; return 1; }
    if (h.cfg.backbone == SOCCDPT_BACKBONE_SWINL12_384) { err = "soccdpt_train_*: no training step is built for dpt_swin_large_384 (Swin-V1-L): it is forward-only"; return 1; }
    if (!train_backbone_ok(h)) { err = "soccdpt_train_*: the training step is built for dpt_swin2_tiny_256, dpt_swin2_base_384 and dpt_hybrid_384; dpt_swin2_large_384 is forward-only"; return 1; }
    if (B < 1 || !ws) { err = "soccdpt_train_*: bad arguments"; return 1; }
    for (const auto& w : h.weights)
        if (!w.ptr) { err = "soccdpt_train_*: weight not bound: " + w.key; return 1; }
    if (ws_bytes < train_workspace_bytes(h, B)) { err = "soccdpt_train_*: workspace too small"; return 1; }
    return 0;
}


// ---- one layer backward on caller-supplied tensors (soccdpt_op_train_layer_bwd: tests) ----
namespace {

// the scratch of one call: the five regions carve() reserves for the whole network sized by this call's plan, merged over the operand formats (so the size does
// not depend on the amp mode) and kLayerSlackFloats each; the weight slot; the arena of deferred sums
struct LayerGeom { ScratchNeed s; size_t slot = 0, arena = 0; };
constexpr size_t kLayerSlackFloats = 64;
// what survives between calls on one handle: the Tape (Tape::xt_tn_src: whose staged copy S_T2 holds) and what the copy was staged for
struct LayerState {
    Tape T;
    const void* scratch = nullptr;
    const float* X = nullptr;
    int B = 0, r = 0, C = 0, amp = -1;
    bool valid = false;
};

int layer_geom(const soccdpt_train_layer_bwd_args& a, LayerGeom& g, std::string& err) {
    auto bad = [&](const char* m) { err = std::string("soccdpt_op_train_layer_bwd: ") + m; return 1; };
    if (a.kind != SOCCDPT_LAYER_LINEAR && a.kind != SOCCDPT_LAYER_CONV3 && a.kind != SOCCDPT_LAYER_CONV_GEN) return bad("kind is SOCCDPT_LAYER_LINEAR, _CONV3 or _CONV_GEN");
    if (a.N <= 0 || a.C <= 0 || a.N % 4 || a.C % 4 || a.N > 8192 || a.C > 8192) return bad("N and C must be positive multiples of 4 (at most 8192)");
    if (!a.dY || !a.X || !a.W) return bad("dY, X and W must be given");
    if (!a.dX && !a.dW && !a.db) return bad("no output requested");
    if (a.dX_res && !a.dX) return bad("dX_res without dX");
    if (a.dX && a.N % 32) return bad("dX needs N % 32 == 0 (the dgrad GEMM's K)");
    int r = a.r;
    if (a.kind == SOCCDPT_LAYER_LINEAR) {
        if (a.M <= 0 || a.M > (1 << 22)) return bad("M must be positive (at most 2^22)");
        if (a.reuse_xt) return bad("reuse_xt is a SOCCDPT_LAYER_CONV3 flag");
    } else {
        if (a.kind == SOCCDPT_LAYER_CONV_GEN) {
            if (a.reuse_xt || a.dX_res) return bad("SOCCDPT_LAYER_CONV_GEN takes no reuse_xt and no dX_res");
            if (a.N % 32 || a.C % 32) return bad("SOCCDPT_LAYER_CONV_GEN needs N, C % 32 == 0");
            if (a.Hi <= 0 || a.Ho <= 0 || a.Hi > 1024) return bad("Hi and Ho must be positive (Hi at most 1024)");
            const bool s1 = a.stride == 1 && a.pad == 1 && a.Ho == a.Hi;
            const bool s2 = a.stride == 2 && a.pad == 1 && a.Ho == (a.Hi - 1) / 2 + 1;
            const bool same2 = a.stride == 2 && a.pad == 0 && a.Hi % 2 == 0 && a.Ho == a.Hi / 2;   // 'SAME' at stride 2: one zero row / column behind an even image
            if (!s1 && !s2 && !same2) return bad("SOCCDPT_LAYER_CONV_GEN: (stride, pad, Hi, Ho) is (1, 1, H, H), (2, 1, H, (H - 1) / 2 + 1) or (2, 0, H even, H / 2)");
            r = a.Ho;
        } else if (a.r <= 0 || a.r > 1024) return bad("r must be positive (at most 1024)");
        if (a.B <= 0 || a.B > 64) return bad("B must be positive (at most 64)");
    }
    const bool linear = a.kind == SOCCDPT_LAYER_LINEAR;
    const size_t N = a.N, C = a.C, taps = linear ? 1 : 9;
    const size_t krows = linear ? roundup((size_t)a.M, 64) : conv3_tn_rows(a.B, r);   // K of the TN weight-gradient kernel
    if (a.stage_weight && a.kind != SOCCDPT_LAYER_CONV_GEN) {   // (conv_gen_bwd's tap-major weights are derived ones: never staged)
        const int64_t sh[4] = {a.N, a.C, 3, 3};
        if (wt_slot_kind(sh, linear ? 2 : 4) >= 0) g.slot = roundup(N * C * taps, 64);
    }
    if (a.defer) {   // the TN kernel's splits: at most 64, at most one per two k-tiles of at least 32 rows, partials within kTrainSkPartFloats (tr_wgrad_tn)
        const size_t smax = std::min<size_t>(64, std::max<size_t>(1, krows / 64));
        g.arena = std::min(smax * (N * taps * C + roundup(N, 4)), kTrainSkPartFloats) + 64;
    }
    const PlanReq q{a.dX != nullptr, a.dW != nullptr, g.slot != 0, a.defer != 0};
    for (OpFmt f : {OpFmt::F32, OpFmt::BF16, OpFmt::F16, OpFmt::X3})
        g.s.merge(linear ? plan_linear((size_t)a.M, a.N, a.C, f, q).need
                         : a.kind == SOCCDPT_LAYER_CONV3 ? plan_conv3(a.B, a.r, a.N, a.C, f, q).need : plan_conv_gen(a.B, a.Hi, a.Ho, a.N, a.C, a.stride, a.pad, f, q).need);
    for (auto r : kRegion) g.s.*r += kLayerSlackFloats;
    return 0;
}

void carve_layer(const LayerGeom& g, TArena& ar, Tape& T) {
    T.S_cap = g.s;
    T.S_T2 = ar.f(g.s.t2);   // first: at the same place whatever N is (reuse_xt)
    T.sk_count = reinterpret_cast<unsigned*>(ar.f(kTrainSkCountWords));
    T.S_T1 = ar.f(g.s.t1);
    T.S_halo = ar.f(g.s.halo);
    T.S_wt = ar.f(g.s.wt);
    T.S_dw = ar.f(g.s.dw);
    T.S_col = ar.f((size_t)1 << 20);
    T.WT = g.slot ? ar.f(g.slot) : nullptr;
    T.sk_part = ar.f(kTrainSkPartFloats);
    T.tn_arena = g.arena ? ar.f(g.arena) : nullptr;
}

}  // namespace
}  // namespace trn
using namespace trn;

size_t train_layer_bwd_scratch_bytes(const soccdpt_train_layer_bwd_args& a, std::string& err) {
    LayerGeom g;
    if (layer_geom(a, g, err)) return 0;
    TArena ar(nullptr);
    Tape T;
    carve_layer(g, ar, T);
    return ar.off + 256;
}

int train_layer_bwd(Handle& h, const soccdpt_train_layer_bwd_args& a, void* scratch, size_t scratch_bytes, unsigned* path_out, hipStream_t st, std::string& err) {
    LayerGeom g;
    if (layer_geom(a, g, err)) return 1;
    if (!scratch || reinterpret_cast<uintptr_t>(scratch) % 256) { err = "soccdpt_op_train_layer_bwd: the scratch must be 256-byte aligned"; return 1; }
    if (!h.layer_state) h.layer_state = std::make_shared<LayerState>();
    LayerState& S = *static_cast<LayerState*>(h.layer_state.get());
    const bool conv3 = a.kind == SOCCDPT_LAYER_CONV3;
    if (a.reuse_xt && !(S.valid && S.scratch == scratch && S.X == a.X && S.B == a.B && S.r == a.r && S.C == a.C && S.amp == h.train_amp)) {
        err = "soccdpt_op_train_layer_bwd: reuse_xt needs the previous call on this handle to have been a SOCCDPT_LAYER_CONV3 one on the same scratch, X, B, r, C and operand format";
        return 1;
    }
    S.valid = false;
    Tape& T = S.T;
    if (!a.reuse_xt) T.xt_tn_src = nullptr;
    TArena ar(scratch);
    carve_layer(g, ar, T);
    if (scratch_bytes < ar.off + 256) { err = "soccdpt_op_train_layer_bwd: scratch too small"; return 1; }
    T.wt_by_ptr.clear();
    {
        hipError_t e = hipMemsetAsync(T.sk_count, 0, kTrainSkCountWords * sizeof(unsigned), st);   // the split-K arrival counters are zero at rest
        if (e != hipSuccess) { err = std::string("soccdpt_op_train_layer_bwd memset: ") + hipGetErrorString(e); return 1; }
    }
    Ctx c{h, T, conv3 || a.kind == SOCCDPT_LAYER_CONV_GEN ? a.B : 1, st, err};
    if (a.defer) {   // dW / db take the route of bound parameter gradients
        c.arm_defer(T.tn_arena, g.arena);
        if (a.dW) c.grad_ptrs.insert(a.dW);
        if (a.db) c.grad_ptrs.insert(a.db);
    }
    if (g.slot) TRY(stage_weight_list(c, {WtStage{a.W, 0, a.N, a.C, conv3 ? 1 : 0}}));
    if (a.kind == SOCCDPT_LAYER_LINEAR) TRY(linear_bwd(c, a.dY, a.X, a.W, (size_t)a.M, a.N, a.C, a.dX, a.dX_res, a.dW, a.db));
    else if (conv3) TRY(conv3_bwd(c, a.dY, a.X, a.W, a.r, a.N, a.C, a.dX, a.dX_res, a.dW, a.db, a.reuse_xt != 0));
    else TRY(conv_gen_bwd(c, a.dY, a.X, a.W, a.Hi, a.Ho, a.N, a.C, a.stride, a.pad, a.dX, a.dW, a.db));
    TRY(tn_flush(c.tn, st, err));
    if (path_out) *path_out = c.path;
    if (conv3) { S.scratch = scratch; S.X = a.X; S.B = a.B; S.r = a.r; S.C = a.C; S.amp = h.train_amp; S.valid = true; }
    return 0;
}

// Named tape tensors for tests / debugging: f32, plain [rows][C] unless noted.
int train_workspace_tensor(Handle& h, int B, const char* name, size_t* byte_offset, size_t* elems) {
    if (B < 1 || !name) return 1;
    char base[256];
    TArena ar(base);   // a non-null base: offsets come out as pointer differences
    Tape T;
    carve(h, B, ar, T);
    const Arch& a = h.arch;
    const int F = h.cfg.features, r1 = 2 * a.fres(0), r0 = 4 * a.fres(0);
    const size_t M1 = (size_t)B * r1 * r1, M0p = (size_t)B * r0 * r0;
    const float* p = nullptr;
    size_t n = 0;
    const std::string k = name;
    if (k == "seg_conv") { p = T.c_raw; n = M1 * F; }                 // seg_head.0 output (pre-BatchNorm)
    else if (k == "seg_act") { p = T.r; n = M1 * F; }                 // after BatchNorm + ReLU + Dropout
    else if (k == "seg_logits") { p = T.logits; n = M1 * 3; }
    else if (k == "depth_conv2") { p = T.e; n = M0p * 32; }           // output_conv.2 output (pre-ReLU)
    else if (k == "depth_conv0") { p = T.d1; n = M1 * (size_t)(F / 2); }
    else if (k == "d_path1") { p = T.GP; n = M1 * F; }                // gradient w.r.t. path_1 (after the backward)
    else if (k.compare(0, 10, "drop_path.") == 0 && !a.hybrid) {      // "drop_path.<stage>.<block>": the [2][B] DropPath scales of one Swin block
        int s2 = -1, j2 = -1;
        if (sscanf(k.c_str() + 10, "%d.%d", &s2, &j2) == 2 && s2 >= 0 && s2 < 4 && j2 >= 0 && j2 < a.depths[s2]) { p = T.blk[s2][j2].dp; n = 2 * (size_t)B; }
    }
    else if (k == "seg_keep") { p = reinterpret_cast<const float*>(T.keep); n = M1 * F; }   // uint8
    else if (k.compare(0, 3, "hy.") == 0 && a.hybrid) {
        const HyTape& Y = T.hy;
        const int H2 = a.img / 4;
        if (k == "hy.stem_pool") { p = Y.pool; n = (size_t)B * H2 * H2 * a.stem_ch; }
        else if (k == "hy.pool_idx") { p = reinterpret_cast<const float*>(Y.pool_idx); n = (size_t)B * H2 * H2 * a.stem_ch; }   // uint8
        else if (k.compare(0, 6, "hy.blk") == 0) {                    // "hy.blk<i>.t1" / ".t2" / ".out", i in HyTape::blk order
            int i = -1, used = 0;
            if (sscanf(k.c_str() + 6, "%d%n", &i, &used) == 1 && i >= 0 && i < (int)Y.blk.size()) {
                const RnBlkT& b = Y.blk[i];
                const RnBlockP& g = h.params.hy.rn[i];
                const std::string part = k.substr(6 + used);
                if (part == ".t1") { p = b.t1; n = (size_t)B * (g.rin + 2) * (g.rin + 2) * g.mid; }
                else if (part == ".t2") { p = b.t2; n = (size_t)B * g.rout * g.rout * g.mid; }
                else if (part == ".out") { p = b.out; n = (size_t)B * g.rout * g.rout * g.cout; }
            }
        }
    }
    else {
        for (int l = 0; l < 4 && !p; ++l) {
            const int r = a.fres(l);
            const size_t M = (size_t)B * r * r, Mh = (size_t)B * (r + 2) * (r + 2);
            const std::string sl = std::to_string(l);
            if (k == "lrn_raw" + sl) { p = T.lrn_raw[l]; n = M * F; }
            else if (k == "fusion_out" + sl) { p = T.oc[l]; n = M * F; }
            else if (k == "rcu2_out" + sl) { p = T.u[l]; n = M * F; }
            else if (k == "fused_raw" + sl && l < 3) { p = T.out_raw[l]; n = M * F; }
            else if (k == "d_feat" + sl) { p = T.DF[l]; n = M * a.fdim(l); }
            // zero-halo images [B][r+2][r+2][C]
            else if (k == "feat" + sl) { p = T.feat[l]; n = Mh * a.fdim(l); }
            else if (k == "lrn_relu" + sl) { p = T.lrn_relu[l]; n = Mh * F; }
            else if (k == "rcu1_mid" + sl && l < 3) { p = T.t1[l]; n = Mh * F; }
            else if (k == "fused_relu" + sl && l < 3) { p = T.out_relu[l]; n = Mh * F; }
            else if (k == "rcu2_mid" + sl) { p = T.t2[l]; n = Mh * F; }
        }
    }
    if (!p) return 1;
    *byte_offset = (size_t)(reinterpret_cast<const char*>(p) - base);
    *elems = n;
    return 0;
}

size_t train_workspace_bytes(Handle& h, int B) {
    if (!train_backbone_ok(h)) return 0;   // no training step for this model: nothing to size (check_train names the reason)
    TArena ar(nullptr);
    Tape T;
    carve(h, B, ar, T);
    return ar.off + 256;
}

int train_forward(Handle& h, const float* x, int B, float* inv, float* seg, void* ws, size_t ws_bytes, float dropout_p, unsigned seed, hipStream_t st, std::string& err) {
    if (check_train(h, B, ws, ws_bytes, err)) return 1;
    const Arch& a = h.arch;
    TArena ar(ws);
    Tape T;
    carve(h, B, ar, T);
    T.dropout_p = dropout_p;
    Ctx c{h, T, B, st, err};
    const ModelP& P = h.params;
    const int F = h.cfg.features;
    {
        hipError_t e = hipMemsetAsync(static_cast<char*>(ws) + T.halo_lo, 0, T.halo_hi - T.halo_lo, st);
        if (e != hipSuccess) { err = std::string("train_forward memset: ") + hipGetErrorString(e); return 1; }
    }
    if (a.hybrid) { TRY(hy_forward(c, x)); } else {
    // ---------------- encoder ----------------
    const int G = a.grid(), C0 = a.embed;
    const size_t M0 = (size_t)B * G * G;
    TRY(tr_patch_im2col(x, T.patches, B, a.img, st, err));
    TRY(tr_pad_cols(c.W(P.swin.patch.w), T.pe_wpad, C0, 48, 64, st, err));
    {
        IgemmDesc d;
        d.X = T.patches; d.Wt = T.pe_wpad; d.M = (int)M0; d.N = C0; d.Cin = 64; d.ldx = 64; d.bias = c.W(P.swin.patch.b); d.out_f32 = T.pe_pre;
        TRY(gemm_fwd(c, d, M0 * 64, (size_t)C0 * 64));
        TRY(launch_ln_residual(T.pe_pre, c.W(P.swin.patch_norm.g), c.W(P.swin.patch_norm.b), T.x0, nullptr, nullptr, nullptr, 0, (int)M0, C0, 0, G, 0,
                               st, err));
    }
    const float* xcur = T.x0;
    int blk_index = 0;
    const int nblk_total = a.depths[0] + a.depths[1] + a.depths[2] + a.depths[3];
    for (int s = 0; s < 4; ++s) {
        const int C = a.dim(s), res = a.res(s), M = B * res * res, wsz = a.ws(s), H = a.heads[s];
        for (int j = 0; j < a.depths[s]; ++j) {
            BlkT& b = T.blk[s][j];
            const SwinBlockP& p = P.swin.blk[s][j];
            b.xin = xcur;
            // stochastic depth (timm DropPath on both residual branches; rate rising linearly over the blocks): per-sample scales for this block
            const float dp_p = nblk_total > 1 ? h.train_drop_path * (float)blk_index / (float)(nblk_total - 1) : 0.f;
            const bool dp_on = h.train_drop_path > 0.f;
            if (dp_on) {
                TRY(tr_drop_path_fill(b.dp, B, dp_p, seed, 2u * (unsigned)blk_index, st, err));
                TRY(tr_drop_path_fill(b.dp + B, B, dp_p, seed, 2u * (unsigned)blk_index + 1u, st, err));
            }
            ++blk_index;
            TRY(launch_qkv_bias(c.W(p.q_bias), c.W(p.v_bias), b.qkv_bias, C, st, err));
            TRY(launch_logit_scale(c.W(p.logit_scale), b.scale, H, st, err));
            TRY(launch_cpb_table(c.W(p.cpb0_w), c.W(p.cpb0_b), c.W(p.cpb2_w), b.table, wsz, a.pretrained_window[s], H,
                                 st, err));
            TRY(launch_attn_bias(b.table, b.bias_acc, wsz, H, st, err));
            IgemmDesc d;
            d.X = b.xin; d.Wt = c.W(p.qkv_w); d.M = M; d.N = 3 * C; d.Cin = C; d.ldx = C; d.bias = b.qkv_bias; d.out_f32 = b.qkv;
            TRY(gemm_fwd(c, d, (size_t)M * C, (size_t)3 * C * C));
            TRY(launch_window_attention_f32(b.qkv, b.bias_acc, b.table, b.scale, b.attn, B, res, wsz, a.shift(s, j), H, st, err));
            d = IgemmDesc();
            d.X = b.attn; d.Wt = c.W(p.proj.w); d.M = M; d.N = C; d.Cin = C; d.ldx = C; d.bias = c.W(p.proj.b); d.out_f32 = b.a_pre;
            TRY(gemm_fwd(c, d, (size_t)M * C, (size_t)C * C));
            TRY(copy_d2d(c, b.x1, b.xin, (size_t)M * C * 4, "train_forward copy"));
            TRY(launch_ln_residual(b.a_pre, c.W(p.n1.g), c.W(p.n1.b), b.x1, nullptr, nullptr, nullptr, 0, M, C, 1, res, 0, st, err,
                                   dp_on ? b.dp : nullptr, res * res));
            d = IgemmDesc();
            d.X = b.x1; d.Wt = c.W(p.fc1.w); d.M = M; d.N = 4 * C; d.Cin = C; d.ldx = C; d.bias = c.W(p.fc1.b); d.act = ACT_GELU;
            d.out_f32 = b.hpre; d.out_op = b.hact;
            TRY(gemm_fwd(c, d, (size_t)M * C, (size_t)4 * C * C));
            d = IgemmDesc();
            d.X = b.hact; d.Wt = c.W(p.fc2.w); d.M = M; d.N = C; d.Cin = 4 * C; d.ldx = 4 * C; d.bias = c.W(p.fc2.b); d.out_f32 = b.m_pre;
            TRY(gemm_fwd(c, d, (size_t)M * 4 * C, (size_t)4 * C * C));
            TRY(copy_d2d(c, b.xout, b.x1, (size_t)M * C * 4, "train_forward copy"));
            TRY(launch_ln_residual(b.m_pre, c.W(p.n2.g), c.W(p.n2.b), b.xout, nullptr, nullptr, j == a.hooks[s] ? T.feat[s] : nullptr, 0, M, C, 1, res, 0,
                                   st, err, dp_on ? b.dp + B : nullptr, res * res));
            xcur = b.xout;
        }
        if (s < 3) {
            const MergeP& mp = P.swin.merge[s];
            TRY(launch_merge_gather(xcur, T.mg[s], B, res, C, 4, st, err));
            IgemmDesc d;
            d.X = T.mg[s]; d.Wt = c.W(mp.red_w); d.M = M / 4; d.N = 2 * C; d.Cin = 4 * C; d.ldx = 4 * C; d.out_f32 = T.mr_pre[s];
            TRY(gemm_fwd(c, d, (size_t)M * C, (size_t)8 * C * C));
            TRY(launch_ln_residual(T.mr_pre[s], c.W(mp.norm.g), c.W(mp.norm.b), T.mx[s], nullptr, nullptr, nullptr, 0, M / 4, 2 * C, 0, res / 2, 0, st, err));
            xcur = T.mx[s];
        }
    }
    }
    // ---------------- decoder ----------------
    for (int l = 0; l < 4; ++l) {
        TRY(launch_conv_w(c.W(P.layer_rn[l]), nullptr, T.w_lrn[l], 1, 0, F, a.fdim(l), st, err));
        for (int u = 0; u < 2; ++u) {
            if (l == 3 && u == 0) continue;
            TRY(launch_conv_w(c.W(P.refine[l].rcu[u].c1.w), nullptr, T.w_rcu[l][u][0], 1, 0, F, F, st, err));
            TRY(launch_conv_w(c.W(P.refine[l].rcu[u].c2.w), nullptr, T.w_rcu[l][u][1], 1, 0, F, F, st, err));
        }
    }
    for (int l = 3; l >= 0; --l) {
        const int r = a.fres(l), M = B * r * r;
        const RefineP& R = P.refine[l];
        {
            IgemmDesc d = conv_desc(T.feat[l], a.fdim(l), T.w_lrn[l], F, r, B);
            d.out_f32 = T.lrn_raw[l]; d.out_op = T.lrn_relu[l]; d.out_halo = 1; d.act = ACT_RELU;
            TRY(gemm_fwd(c, d, Halo{r, r, a.fdim(l)}.elems(B), (size_t)F * 9 * a.fdim(l)));
        }
        const float* fused_raw = T.lrn_raw[l];
        const float* fused_relu = T.lrn_relu[l];
        if (l < 3) {
            const RcuP& ub = R.rcu[0];
            IgemmDesc d = conv_desc(T.lrn_relu[l], F, T.w_rcu[l][0][0], F, r, B);
            d.bias = c.W(ub.c1.b); d.act = ACT_RELU; d.out_op = T.t1[l]; d.out_halo = 1;
            TRY(gemm_fwd(c, d, Halo{r, r, F}.elems(B), (size_t)F * 9 * F));
            d = conv_desc(T.t1[l], F, T.w_rcu[l][0][1], F, r, B);
            d.bias = c.W(ub.c2.b); d.res1 = T.lrn_raw[l];
            d.res2 = T.oc[l + 1]; d.res2_h = a.fres(l + 1); d.res2_w = a.fres(l + 1);
            d.out_f32 = T.out_raw[l]; d.out_op = T.out_relu[l]; d.out_halo = 1; d.act = ACT_RELU;
            TRY(gemm_fwd(c, d, Halo{r, r, F}.elems(B), (size_t)F * 9 * F));
            fused_raw = T.out_raw[l];
            fused_relu = T.out_relu[l];
        }
        {
            const RcuP& ub = R.rcu[1];
            IgemmDesc d = conv_desc(fused_relu, F, T.w_rcu[l][1][0], F, r, B);
            d.bias = c.W(ub.c1.b); d.act = ACT_RELU; d.out_op = T.t2[l]; d.out_halo = 1;
            TRY(gemm_fwd(c, d, Halo{r, r, F}.elems(B), (size_t)F * 9 * F));
            d = conv_desc(T.t2[l], F, T.w_rcu[l][1][1], F, r, B);
            d.bias = c.W(ub.c2.b); d.res1 = fused_raw; d.out_f32 = T.u[l];
            TRY(gemm_fwd(c, d, Halo{r, r, F}.elems(B), (size_t)F * 9 * F));
        }
        {
            IgemmDesc d;
            d.X = T.u[l]; d.Wt = c.W(R.out_conv.w); d.M = M; d.N = F; d.Cin = F; d.ldx = F; d.bias = c.W(R.out_conv.b); d.out_f32 = T.oc[l];
            TRY(gemm_fwd(c, d, (size_t)M * F, (size_t)F * F));
        }
        if (l == 0) TRY(launch_bilinear(T.oc[0], 0, nullptr, nullptr, T.path1, 1, 0, B, r, r, 2 * r, 2 * r, F, st, err));
    }
    // ---------------- heads ----------------
    const int r1 = 2 * a.fres(0), r0 = 4 * a.fres(0);
    const size_t M1 = (size_t)B * r1 * r1, M0p = (size_t)B * r0 * r0;
    TRY(launch_conv_w(c.W(P.depth.c0.w), nullptr, T.w_d0, 1, 0, F / 2, F, st, err));
    TRY(launch_conv_w(c.W(P.depth.c2.w), nullptr, T.w_d2, 1, 0, 32, F / 2, st, err));
    TRY(launch_conv_w(c.W(P.seg.c0_w), nullptr, T.w_s0, 1, 0, F, F, st, err));
    {
        IgemmDesc d = conv_desc(T.path1, F, T.w_d0, F / 2, r1, B);
        d.bias = c.W(P.depth.c0.b); d.out_f32 = T.d1;
        TRY(gemm_fwd(c, d, Halo{r1, r1, F}.elems(B), (size_t)(F / 2) * 9 * F));
        TRY(launch_bilinear(T.d1, 0, nullptr, nullptr, T.d1u, 1, 0, B, r1, r1, r0, r0, F / 2, st, err));
        d = conv_desc(T.d1u, F / 2, T.w_d2, 32, r0, B);
        d.bias = c.W(P.depth.c2.b); d.out_f32 = T.e;
        TRY(gemm_fwd(c, d, Halo{r0, r0, F / 2}.elems(B), (size_t)32 * 9 * (F / 2)));
        TRY(tr_depth_tail_fwd(T.e, c.W(P.depth.c4.w), c.W(P.depth.c4.b), T.inv, M0p, 32, st, err));
        TRY(copy_d2d(c, inv, T.inv, M0p * 4, "train_forward inv"));
    }
    {
        IgemmDesc d = conv_desc(T.path1, F, T.w_s0, F, r1, B);
        d.out_f32 = T.c_raw;
        TRY(gemm_fwd(c, d, Halo{r1, r1, F}.elems(B), (size_t)F * 9 * F));
        TRY(tr_bn_stats(T.c_raw, T.bn_stats, const_cast<float*>(c.W(P.seg.bn_mean)), const_cast<float*>(c.W(P.seg.bn_var)), T.S_col, F, M1, 1e-5f,
                        0.1f, st, err));
        TRY(tr_bn_relu_dropout_fwd(T.c_raw, T.bn_stats, c.W(P.seg.bn.g), c.W(P.seg.bn.b), T.r, T.keep, M1, F, dropout_p, seed, st, err));
        TRY(launch_seg_tail(T.r, 1, 0, c.W(P.seg.c4.w), c.W(P.seg.c4.b), T.logits, T.seg, B, r1, r1, h.cfg.sigmoid, st, err));
        TRY(copy_d2d(c, seg, T.seg, M0p * 3 * 4, "train_forward seg"));
    }
    return 0;
}

// Encoder part of the backward: consumes the gradients of the four hooked feature maps (T.DF[l], [pixels][channels]) left by the decoder pass.
static int encoder_backward(Ctx& c) {
    Handle& h = c.h;
    const Arch& a = h.arch;
    Tape& T = c.T;
    const int B = c.B;
    hipStream_t st = c.st;
    std::string& err = c.err;
    float** G = T.G;
    if (a.hybrid) return hy_backward(c);
    const ModelP& P = h.params;
    {
        const float* xcur = T.x0;
        for (int s = 0; s < 4; ++s) {
            for (auto& b : T.blk[s]) { b.xin = xcur; xcur = b.xout; }
            if (s < 3) xcur = T.mx[s];
        }
    }
    // ---------------- encoder, last stage -> first ----------------
    bool have = false;   // GX holds a gradient
    for (int s = 3; s >= 0; --s) {
        const int C = a.dim(s), res = a.res(s), wsz = a.ws(s), H = a.heads[s];
        const size_t M = (size_t)B * res * res;
        for (int j = a.depths[s] - 1; j >= 0; --j) {
            BlkT& b = T.blk[s][j];
            const SwinBlockP& p = P.swin.blk[s][j];
            if (j == a.hooks[s]) {
                if (have) TRY(tr_axpy(T.GX, T.DF[s], M * C, st, err));
                else TRY(copy_d2d(c, T.GX, T.DF[s], M * C * 4, "train_backward"));
                have = true;
            }
            if (!have) continue;   // blocks after the last hooked one do not reach the outputs
            if (!any_grad(h, p.upto)) return 0;   // nothing trainable at or before this block in forward order: the walk ends below the earliest trainable tensor
            // xout = x1 + dp2 * LN2(m_pre)      (dp: the forward's per-sample DropPath scales; the gradient entering the branch is scaled alike)
            const bool dp_on = h.train_drop_path > 0.f;
            const float* g_mlp = T.GX;
            if (dp_on) { TRY(tr_scale_rows(T.GX, G[4], b.dp + B, M, C, res * res, st, err)); g_mlp = G[4]; }
            TRY(ln_bwd(c, b.m_pre, c.W(p.n2.g), g_mlp, G[0], G[1], M, C, c.Gd(p.n2.g), c.Gd(p.n2.b)));
            TRY(linear_bwd(c, G[0], b.hact, c.W(p.fc2.w), M, C, 4 * C, G[2], nullptr, c.Gd(p.fc2.w), c.Gd(p.fc2.b)));
            TRY(tr_gelu_bwd(G[2], b.hpre, G[2], M * 4 * C, st, err));
            TRY(linear_bwd(c, G[2], b.x1, c.W(p.fc1.w), M, 4 * C, C, G[3], T.GX, c.Gd(p.fc1.w), c.Gd(p.fc1.b)));   // G3 = d x1
            // x1 = xin + dp1 * LN1(a_pre)
            const float* g_att = G[3];
            if (dp_on) { TRY(tr_scale_rows(G[3], G[4], b.dp, M, C, res * res, st, err)); g_att = G[4]; }
            TRY(ln_bwd(c, b.a_pre, c.W(p.n1.g), g_att, G[0], G[1], M, C, c.Gd(p.n1.g), c.Gd(p.n1.b)));
            TRY(linear_bwd(c, G[0], b.attn, c.W(p.proj.w), M, C, C, G[2], nullptr, c.Gd(p.proj.w), c.Gd(p.proj.b)));
            // train_attn.hip.  amp modes: the four products of the attention backward on 16-bit MFMAs too (autocast semantics); exact f32 and x3: exact products
            const OpFmt attn_fmt = op_is16(amp_fmt(c)) ? amp_fmt(c) : OpFmt::F32;
            TRY(tr_attention_bwd_mfma(b.qkv, b.attn, G[2], b.table, b.scale, T.dS, T.rowstat, T.dscale_part, G[4], B, res, wsz, a.shift(s, j), H, st, err, attn_fmt));
            {
                float* dls = c.Gd(p.logit_scale);
                float* dw0 = c.Gd(p.cpb0_w);
                float* db0 = c.Gd(p.cpb0_b);
                float* dw2 = c.Gd(p.cpb2_w);
                if (dls || dw0 || db0 || dw2)
                    TRY(tr_attn_param_grads(T.dS, T.dscale_part, b.table, c.W(p.logit_scale), c.W(p.cpb0_w), c.W(p.cpb0_b),
                                            c.W(p.cpb2_w), T.dtable, T.dt, T.S_cpb, dls, dw0, db0, dw2, B * (res / wsz) * (res / wsz), wsz,
                                            a.pretrained_window[s], H, tr_attention_bwd_mfma_slots(wsz), st, err));
            }
            {
                float* dq = c.Gd(p.q_bias);
                float* dv = c.Gd(p.v_bias);
                float* dbias = (dq || dv) ? T.S_vec : nullptr;
                TRY(linear_bwd(c, G[4], b.xin, c.W(p.qkv_w), M, 3 * C, C, T.GX, G[3], c.Gd(p.qkv_w), dbias));
                if (dbias) TRY(tr_qv_bias_grad(dbias, dq, dv, C, st, err));
            }
        }
        if (!have) continue;
        if (!any_grad(h, P.swin.below[s])) return 0;   // nothing trainable in patch_embed or stages < s (their blocks and PatchMerging)
        if (s > 0) {
            // x_s = LN(reduction(gather(x_{s-1})))   (timm PatchMerging of Swin-V2: reduction then norm)
            const int Cp = a.dim(s - 1);
            const MergeP& mp = P.swin.merge[s - 1];
            TRY(ln_bwd(c, T.mr_pre[s - 1], c.W(mp.norm.g), T.GX, G[0], G[1], M, C, c.Gd(mp.norm.g), c.Gd(mp.norm.b)));
            TRY(linear_bwd(c, G[0], T.mg[s - 1], c.W(mp.red_w), M, C, 4 * Cp, G[2], nullptr, c.Gd(mp.red_w), nullptr));
            TRY(tr_merge_scatter(G[2], T.GX, B, a.res(s - 1), Cp, st, err));
        } else {
            const int C0 = a.embed;
            TRY(ln_bwd(c, T.pe_pre, c.W(P.swin.patch_norm.g), T.GX, G[0], G[1], M, C0, c.Gd(P.swin.patch_norm.g), c.Gd(P.swin.patch_norm.b)));
            float* dw = c.Gd(P.swin.patch.w);
            TRY(linear_bwd(c, G[0], T.patches, T.pe_wpad, M, C0, 64, nullptr, nullptr, dw ? T.S_dw + kPeGradOffset : nullptr, c.Gd(P.swin.patch.b)));
            if (dw) TRY(tr_pad_cols(T.S_dw + kPeGradOffset, dw, C0, 64, 48, st, err));
        }
    }
    return 0;
}

// Test entry: the encoder backward alone, from caller-supplied gradients of the hooked feature maps (d_feat[l]: [B * fres(l)^2][fdim(l)] f32).
int train_backward_encoder(Handle& h, int B, const float* const* d_feat, void* ws, size_t ws_bytes, hipStream_t st, std::string& err) {
    if (check_train(h, B, ws, ws_bytes, err)) return 1;
    TArena ar(ws);
    Tape T;
    carve(h, B, ar, T);
    Ctx c{h, T, B, st, err};
    c.arm_defer(T.tn_arena, kTrainTnArenaFloats);
    for (int l = 0; l < 4; ++l) {
        if (!d_feat || !d_feat[l]) { err = "soccdpt_train_backward_encoder: null feature gradient"; return 1; }
        const size_t n = (size_t)B * h.arch.fres(l) * h.arch.fres(l) * h.arch.fdim(l);
        TRY(copy_d2d(c, T.DF[l], d_feat[l], n * 4, "train_backward_encoder"));
    }
    TRY(stage_weights(c));
    TRY(encoder_backward(c));
    return tn_flush(c.tn, st, err);   // the deferred weight-gradient sums of this pass
}

int train_backward(Handle& h, const float* x, int B, const float* d_inv, const float* d_seg, void* ws, size_t ws_bytes, hipStream_t st, std::string& err) {
    if (check_train(h, B, ws, ws_bytes, err)) return 1;
    (void)x;
    const Arch& a = h.arch;
    TArena ar(ws);
    Tape T;
    carve(h, B, ar, T);
    T.dropout_p = h.train_key.dropout_p;
    Ctx c{h, T, B, st, err};
    const ModelP& P = h.params;
    c.arm_defer(T.tn_arena, kTrainTnArenaFloats);   // weight-gradient partials wait for ONE batched sum at the end of the pass (train.h TnDefer)
    TRY(stage_weights(c));
    auto pass = [&]() -> int {
    const int F = h.cfg.features;
    float** G = T.G;
    const int r1 = 2 * a.fres(0), r0 = 4 * a.fres(0);
    const size_t M1 = (size_t)B * r1 * r1, M0p = (size_t)B * r0 * r0;
    const bool enc_train = any_grad(h, P.encoder);   // depth_net.pretrained.*: the timm model and, for the hybrid, the act_postprocess read-outs
    // Frozen prefixes (freeze helpers of model/loss.py, PatchWiseInplace): the gradient stops flowing where nothing upstream is trainable
    bool lvl_own[4], lvl_side[4];   // level l: RCU2 / out_conv / anything coarser  |  RCU1 + layer_rn + encoder hook
    for (int l = 0; l < 4; ++l) {
        const RefineP& R = P.refine[l];
        lvl_own[l] = any_grad(h, R.out_conv_span) || any_grad(h, R.rcu_span[1]);
        lvl_side[l] = enc_train || any_grad(h, R.rcu_span[0]) || any_grad(h, span_of(P.layer_rn[l]));
    }
    bool need_level[5];             // the gradient has to reach level l's out_conv output
    need_level[4] = false;
    for (int l = 3; l >= 0; --l) need_level[l] = lvl_own[l] || lvl_side[l] || need_level[l + 1];
    // ---------------- depth head ----------------
    {
        TRY(tr_depth_tail_bwd(d_inv, T.inv, T.e, c.W(P.depth.c4.w), G[0], G[1], M0p, 32, st, err));
        float* dw4 = c.Gd(P.depth.c4.w);
        float* db4 = c.Gd(P.depth.c4.b);
        if (dw4 || db4) {
            TRY(tr_colsum(G[1], nullptr, T.S_vec, T.S_col, M0p, 33, 0, st, err));
            if (dw4) TRY(copy_d2d(c, dw4, T.S_vec, 32 * 4, "train_backward"));
            if (db4) TRY(copy_d2d(c, db4, T.S_vec + 32, 4, "train_backward"));
        }
        TRY(conv3_bwd(c, G[0], T.d1u, c.W(P.depth.c2.w), r0, 32, F / 2, G[2], nullptr, c.Gd(P.depth.c2.w), c.Gd(P.depth.c2.b)));
        TRY(tr_bilinear_bwd(G[2], G[3], B, r1, r1, r0, r0, F / 2, 0, st, err));
        TRY(conv3_bwd(c, G[3], T.path1, c.W(P.depth.c0.w), r1, F / 2, F, need_level[0] ? T.GP : nullptr, nullptr, c.Gd(P.depth.c0.w),
                      c.Gd(P.depth.c0.b)));
    }
    // ---------------- seg head ----------------
    {
        TRY(tr_seg_act_bwd(d_seg, T.seg, G[0], B, 3, r0, h.cfg.sigmoid, st, err));
        TRY(tr_bilinear_bwd(G[0], G[1], B, r1, r1, r0, r0, 3, 0, st, err));   // d logits [M1][3]
        if (float* dw = c.Gd(P.seg.c4.w)) TRY(tr_smallk_wgrad(G[1], T.r, dw, T.S_col, M1, F, 3, st, err));
        if (float* db = c.Gd(P.seg.c4.b)) {
            // colsum needs N >= 1: three columns
            TRY(tr_colsum(G[1], nullptr, db, T.S_col, M1, 3, 0, st, err));
        }
        TRY(tr_smallk_dgrad(G[1], c.W(P.seg.c4.w), G[2], M1, F, 3, st, err));
        TRY(tr_bn_relu_dropout_bwd_pre(G[2], T.r, T.keep, G[0], M1 * F, T.dropout_p, st, err));
        TRY(tr_bn_xhat(T.c_raw, T.bn_stats, G[3], M1, F, st, err));
        float* dbeta = T.S_vec;
        float* dgamma = T.S_vec + F;
        TRY(tr_colsum(G[0], nullptr, dbeta, T.S_col, M1, F, 0, st, err));
        TRY(tr_colsum(G[0], G[3], dgamma, T.S_col, M1, F, 0, st, err));
        if (float* p = c.Gd(P.seg.bn.b)) TRY(copy_d2d(c, p, dbeta, F * 4, "train_backward"));
        if (float* p = c.Gd(P.seg.bn.g)) TRY(copy_d2d(c, p, dgamma, F * 4, "train_backward"));
        TRY(tr_bn_bwd(G[0], T.c_raw, T.bn_stats, c.W(P.seg.bn.g), dbeta, dgamma, G[2], M1, F, st, err));
        // path_1's im2col^T is still in S_T2 from output_conv.0's weight gradient (same input image, nothing in between writes S_T2)
        const bool xt_ready = c.Gd(P.depth.c0.w) != nullptr;
        TRY(conv3_bwd(c, G[2], T.path1, c.W(P.seg.c0_w), r1, F, F, need_level[0] ? T.GP : nullptr, T.GP, c.Gd(P.seg.c0_w), nullptr, xt_ready));
    }
    if (!need_level[0]) return 0;
    TRY(tr_bilinear_bwd(T.GP, T.DOC, B, a.fres(0), a.fres(0), r1, r1, F, 0, st, err));
    // ---------------- decoder, fine -> coarse ----------------
    for (int l = 0; l < 4; ++l) {
        const int r = a.fres(l);
        const size_t M = (size_t)B * r * r;
        const RefineP& R = P.refine[l];
        TRY(linear_bwd(c, T.DOC, T.u[l], c.W(R.out_conv.w), M, F, F, G[0], nullptr, c.Gd(R.out_conv.w), c.Gd(R.out_conv.b)));
        const float* fused_raw = l < 3 ? T.out_raw[l] : T.lrn_raw[l];
        const float* fused_relu = l < 3 ? T.out_relu[l] : T.lrn_relu[l];
        {
            const RcuP& ub = R.rcu[1];
            TRY(conv3_bwd(c, G[0], T.t2[l], c.W(ub.c2.w), r, F, F, G[1], nullptr, c.Gd(ub.c2.w), c.Gd(ub.c2.b)));
            TRY(tr_relu_bwd_halo(G[1], T.t2[l], nullptr, G[1], B, r, r, F, st, err));
            TRY(conv3_bwd(c, G[1], fused_relu, c.W(ub.c1.w), r, F, F, G[2], nullptr, c.Gd(ub.c1.w), c.Gd(ub.c1.b)));
            TRY(tr_relu_bwd(G[2], fused_raw, G[0], G[3], M * F, st, err));   // d fused_raw
        }
        const float* d_lrn = G[3];
        if (l < 3 && need_level[l + 1])
            TRY(tr_bilinear_bwd(G[3], T.DOC, B, a.fres(l + 1), a.fres(l + 1), r, r, F, 0, st, err));   // gradient of the coarser level's out_conv output
        if (!lvl_side[l]) {
            if (!need_level[l + 1]) return 0;
            continue;
        }
        if (l < 3) {
            const RcuP& ub = R.rcu[0];
            TRY(conv3_bwd(c, G[3], T.t1[l], c.W(ub.c2.w), r, F, F, G[1], nullptr, c.Gd(ub.c2.w), c.Gd(ub.c2.b)));
            TRY(tr_relu_bwd_halo(G[1], T.t1[l], nullptr, G[1], B, r, r, F, st, err));
            TRY(conv3_bwd(c, G[1], T.lrn_relu[l], c.W(ub.c1.w), r, F, F, G[2], nullptr, c.Gd(ub.c1.w), c.Gd(ub.c1.b)));
            TRY(tr_relu_bwd(G[2], T.lrn_raw[l], G[3], G[0], M * F, st, err));
            d_lrn = G[0];
        }
        const PRef lk = P.layer_rn[l];
        TRY(conv3_bwd(c, d_lrn, T.feat[l], c.W(lk), r, F, a.fdim(l), enc_train ? T.DF[l] : nullptr, nullptr, c.Gd(lk), nullptr));
    }
    if (!enc_train) return 0;
    return encoder_backward(c);
    };
    TRY(pass());
    return tn_flush(c.tn, st, err);
}

}  // namespace soccdpt
