// Training step, ViT-hybrid encoder (dpt_hybrid_384): train-mode forward with saved activations and the backward of
// timm vit_base_resnet50_384 as the reference wires it (/root/reference/SOccDPT/model/backbones/vit.py:147-258: ResNetV2 stem + stages (3, 4, 9)
// with weight-standardised 'SAME' convolutions and GroupNorm, HybridEmbed projection, class token + position embedding, 12 pre-norm ViT-B
// blocks, hooks on stages[0], stages[1], blocks[8], blocks[11]; backbones/utils.py:27-133: ProjectReadout + reassemble convolutions).
// The forward is launch for launch the eval path of model.cpp in exact f32, with every intermediate kept; kernels: train_hybrid.hip, train.hip,
// hybrid.hip, igemm.hip.
#include "train_internal.h"

namespace soccdpt {
namespace trn {
namespace {

const float kWsEps = 1e-8f;    // timm StdConv2dSame
const float kLnEps = 1e-6f;    // timm VisionTransformer norm_layer

}  // namespace

// Backward of a 3x3 convolution with tap-major weights Wtap [N][9][C] over a zero-haloed input [B][Hi+2][Hi+2][C], output Ho x Ho.
// stride 1 / pad 1: dgrad as the same conv over the rotated filter; otherwise dcol = dY Wtap, then col2im.  dWtap_out [N][9][C].
int conv_gen_bwd(Ctx& c, const float* dY, const float* Xhalo, const float* Wtap, int Hi, int Ho, int N, int C, int stride, int pad, float* dX_out, float* dWtap_out,
                 float* db) {
    Tape& T = c.T;
    const int B = c.B;
    const size_t Mo = (size_t)B * Ho * Ho;
    // 16-bit amp modes, un-strided convolutions of the wide stages (N, C multiples of 128): the path the decoder convolutions take in conv3_bwd -- dgrad on the
    // 16-bit igemm over the zero-bordered dY image, weight gradient from the operands as stored in halo pixel order (train_wgrad_tn.hip) -- with the tap-major
    // standardised weights of this encoder on both ends.  Everything else takes the f32 path below.
    const ConvPlan p = plan_conv_gen(B, Hi, Ho, N, C, stride, pad, amp_fmt(c), PlanReq{dX_out != nullptr, dWtap_out != nullptr, false, false});
    TRY(check_fit(c, "conv_gen_bwd", with_dw_target(T, p.need, dWtap_out, (size_t)9 * N * C)));
    const OpFmt fmt = p.fmt;
    c.path |= route_fmt_bit(fmt) | route_wgrad_bit(p.wgrad);
    if (fmt != OpFmt::F32) {
        TRY(conv3_dy_halo(c, dY, Ho, N, fmt));
        if (dX_out) {
            c.path |= SOCCDPT_ROUTE_W_FALLBACK;
            TRY(th_conv_w_dgrad_tap(Wtap, T.S_dw, N, C, c.st, c.err));                         // [C][9][N] f32, rotated
            TRY(cvt_op(c, T.S_dw, T.S_wt, (size_t)C * 9 * N, fmt));
            TRY(conv3_dgrad_s1(c, T.S_wt, Ho, N, C, fmt, dX_out, nullptr));
        }
        if (dWtap_out) {
            c.path |= SOCCDPT_ROUTE_SUM_IMMEDIATE;
            TRY(conv3_wgrad_tn(c, p, Xhalo, N, C, false, dWtap_out, nullptr, false));
        }
        if (db) TRY(tr_colsum(dY, nullptr, db, T.S_col, Mo, N, 0, c.st, c.err));
        return 0;
    }
    if (dX_out) {
        c.path |= SOCCDPT_ROUTE_W_FALLBACK;
        if (!p.col2im) {
            hipError_t e = hipMemsetAsync(T.S_halo, 0, p.Kh * N * sizeof(float), c.st);
            if (e != hipSuccess) { c.err = std::string("conv_gen_bwd memset: ") + hipGetErrorString(e); return 1; }
            TRY(tr_to_halo(dY, T.S_halo, B, Ho, Ho, N, c.st, c.err));
            TRY(th_conv_w_dgrad_tap(Wtap, T.S_wt, N, C, c.st, c.err));
            TRY(conv3_dgrad_s1(c, T.S_wt, Ho, N, C, OpFmt::F32, dX_out, nullptr));
        } else {
            TRY(tr_transpose(Wtap, T.S_wt, OpFmt::F32, N, 9 * C, N, c.st, c.err));   // [9C][N]
            IgemmDesc d;
            d.X = dY; d.Wt = T.S_wt; d.M = (int)Mo; d.N = 9 * C; d.Cin = N; d.ldx = N; d.out_f32 = T.S_T2;   // dcol [Mo][9][C]
            TRY(gemm(c, d));
            TRY(th_col2im(T.S_T2, dX_out, B, Hi, Ho, C, stride, pad, 0, c.st, c.err));
        }
    }
    if (dWtap_out) {
        const int Mp = p.Mp;
        TRY(tr_transpose(dY, T.S_T1, OpFmt::F32, (int)Mo, N, Mp, c.st, c.err));
        TRY(th_im2colT_gen(Xhalo, T.S_T2, B, Hi, Ho, C, stride, pad, (size_t)Mp, c.st, c.err));
        IgemmDesc d;
        d.X = T.S_T1; d.Wt = T.S_T2; d.M = N; d.N = 9 * C; d.Cin = Mp; d.ldx = Mp; d.out_f32 = dWtap_out;
        TRY(gemm_wgrad(c, d, OpFmt::F32));   // f32 staging (the strided / weight-standardised convolutions do not take the amp path)
    }
    if (db) TRY(tr_colsum(dY, nullptr, db, T.S_col, Mo, N, 0, c.st, c.err));
    return 0;
}

namespace {

// GroupNorm statistics ride on the producing convolution as per-tile partials; its reader (gn_apply, gn_finish for the stem) adds them up and leaves
// {mean, rstd} in `stats` for the backward pass (model.cpp's forward does the same: DESIGN.md 11.5)
void with_stats(Ctx& c, IgemmDesc& d, float* stats, int cout, int hw, int slot = 0) {
    HyTape& Y = c.T.hy;
    d.gn_stats = stats; d.gn_part = Y.gn_part[slot]; d.gn_bm_out = &Y.gn_bm[slot]; d.gn_cpg = cout / 32; d.gn_hw = hw; d.gn_eps = 1e-5f;
    d.gn_part_floats = Y.gn_part_floats;
}
void from_partials(Ctx& c, GnApplyArgs& g, int slot, int slot2 = -1) {
    HyTape& Y = c.T.hy;
    g.part = Y.gn_part[slot]; g.tps = g.HW / Y.gn_bm[slot];
    if (slot2 >= 0) { g.part2 = Y.gn_part[slot2]; g.tps2 = g.HW / Y.gn_bm[slot2]; }
}

}  // namespace

void hy_carve_halo(const Handle& h, int B, TArena& ar, Tape& T) {
    HyTape& Y = T.hy;
    const std::vector<RnBlockP>& rn = h.params.hy.rn;
    Y.blk.assign(rn.size(), RnBlkT{});
    for (size_t i = 0; i < rn.size(); ++i) Y.blk[i].t1 = ar.f((size_t)B * (rn[i].rin + 2) * (rn[i].rin + 2) * rn[i].mid);
    const int G = h.arch.grid();
    Y.pp4_in = ar.f((size_t)B * (G + 2) * (G + 2) * h.arch.fdim(3));
}

void hy_carve(const Handle& h, int B, TArena& ar, Tape& T, size_t& maxAct) {
    const Arch& a = h.arch;
    HyTape& Y = T.hy;
    const int S = a.img, H1 = S / 2, H2 = S / 4, E = a.vit_dim, G = a.grid(), NT = G * G + 1;
    const size_t M1s = (size_t)B * H1 * H1, Mt = (size_t)B * NT, Mp = (size_t)B * G * G;
    Y.a0 = ar.f(M1s * 160);
    Y.w_stem = ar.f((size_t)a.stem_ch * 160);
    Y.stem_raw = ar.f(M1s * a.stem_ch);
    Y.stem_stats = ar.f((size_t)B * 32 * 2);
    Y.pool = ar.f((size_t)B * H2 * H2 * a.stem_ch);
    Y.pool_idx = reinterpret_cast<uint8_t*>(ar.f(((size_t)B * H2 * H2 * a.stem_ch + 3) / 4));
    maxAct = std::max(maxAct, M1s * 160);
    for (size_t i = 0; i < Y.blk.size(); ++i) {
        RnBlkT& b = Y.blk[i];
        const RnBlockP& p = h.params.hy.rn[i];
        const size_t Min = (size_t)B * p.rin * p.rin, Mout = (size_t)B * p.rout * p.rout;
        b.w_ds = p.proj ? ar.f((size_t)p.cout * p.cin) : nullptr;
        b.w_c1 = ar.f((size_t)p.mid * p.cin);
        b.w_c2 = ar.f((size_t)p.mid * 9 * p.mid);
        b.w_c3 = ar.f((size_t)p.cout * p.mid);
        b.ds_raw = p.proj ? ar.f(Mout * p.cout) : nullptr;
        b.ds_stats = p.proj ? ar.f((size_t)B * 64) : nullptr;
        b.c1_raw = ar.f(Min * p.mid);
        b.c1_stats = ar.f((size_t)B * 64);
        b.c2_raw = ar.f(Mout * p.mid);
        b.c2_stats = ar.f((size_t)B * 64);
        b.t2 = ar.f(Mout * p.mid);
        b.c3_raw = ar.f(Mout * p.cout);
        b.c3_stats = ar.f((size_t)B * 64);
        b.out = ar.f(Mout * p.cout);
        maxAct = std::max(maxAct, std::max(Min * (size_t)std::max(p.cin, p.mid), Mout * (size_t)p.cout));
        maxAct = std::max(maxAct, Mout * 9 * (size_t)p.mid);   // dcol of the strided 3x3
    }
    Y.gn_part_floats = M1s * 2;   // (M / 32 tiles) x 32 groups x 2 at the stem's M
    for (int i = 0; i < 2; ++i) Y.gn_part[i] = ar.f(Y.gn_part_floats);
    Y.pe_y = ar.f(Mp * E);
    Y.x0 = ar.f(Mt * E);
    Y.vb.assign(a.vit_depth, VitBlkT{});
    for (auto& v : Y.vb) {
        v.ln1 = ar.f(Mt * E);
        v.qkv = ar.f(Mt * 3 * E);
        v.attn = ar.f(Mt * E);
        v.x1 = ar.f(Mt * E);
        v.ln2 = ar.f(Mt * E);
        v.hpre = ar.f(Mt * 4 * E);
        v.hact = ar.f(Mt * 4 * E);
        v.xout = ar.f(Mt * E);
        v.rowstat = ar.f((size_t)B * a.vit_heads * NT * 2);
    }
    for (int k = 0; k < 2; ++k) {
        Y.cat[k] = ar.f(Mp * 2 * E);
        Y.ro_pre[k] = ar.f(Mp * E);
        Y.ro_act[k] = ar.f(Mp * E);
    }
    Y.w_pp4 = ar.f((size_t)a.fdim(3) * 9 * a.fdim(3));
    maxAct = std::max(maxAct, std::max(Mt * 4 * E, Mp * 9 * (size_t)a.fdim(3)));
    Y.GT = ar.f(Mt * E);
    Y.GR = ar.f((size_t)B * H2 * H2 * 256);
    Y.xg = ar.f((size_t)B * (H2 / 2) * (H2 / 2) * 256);
}

int hy_forward(Ctx& c, const float* x) {
    Handle& h = c.h;
    const Arch& a = h.arch;
    Tape& T = c.T;
    HyTape& Y = T.hy;
    const int B = c.B;
    hipStream_t st = c.st;
    std::string& err = c.err;
    const int S = a.img, H1 = S / 2, H2 = S / 4;
    const HybridP& P = h.params.hy;
    // ---- stem: Conv 7x7 / 2 'SAME' (im2col + GEMM) -> GroupNorm + ReLU -> MaxPool 3x3 / 2 'SAME' ----
    TRY(launch_stem_im2col(x, Y.a0, 2, B, S, st, err));
    TRY(launch_ws_conv_w(c.W(P.stem_w), Y.w_stem, 2, a.stem_ch, 3, 7, 160, kWsEps, st, err));
    {
        IgemmDesc d;
        d.X = Y.a0; d.Wt = Y.w_stem; d.M = B * H1 * H1; d.N = a.stem_ch; d.Cin = 160; d.ldx = 160; d.out_f32 = Y.stem_raw;
        with_stats(c, d, Y.stem_stats, a.stem_ch, H1 * H1);
        TRY(gemm(c, d));
        TRY(launch_gn_finish(Y.gn_part[0], Y.stem_stats, B, H1 * H1 / Y.gn_bm[0], 32, H1 * H1, a.stem_ch / 32, 1e-5f, st, err));
        TRY(launch_gn_relu_maxpool(Y.stem_raw, Y.stem_stats, c.W(P.stem_n.g), c.W(P.stem_n.b), Y.pool, 2, B, H1, a.stem_ch, a.stem_ch / 32, st, err));
    }
    const float* xcur = Y.pool;
    int hook = 0, cnt = 0, stage = 0;
    for (size_t bi = 0; bi < Y.blk.size(); ++bi) {
        RnBlkT& b = Y.blk[bi];
        const RnBlockP& p = P.rn[bi];
        const int Min = B * p.rin * p.rin, Mout = B * p.rout * p.rout;
        b.xin = xcur;
        if (p.proj) {
            TRY(launch_ws_conv_w(c.W(p.ds_w), b.w_ds, 2, p.cout, p.cin, 1, p.cin, kWsEps, st, err));
            IgemmDesc d;
            d.X = b.xin; d.Wt = b.w_ds; d.M = Mout; d.N = p.cout; d.Cin = p.cin; d.out_f32 = b.ds_raw;
            if (p.stride == 1) d.ldx = p.cin;
            else { d.gather1 = 1; d.stride = p.stride; d.pad = 0; d.in_halo = 0; d.Hi = p.rin; d.Wi = p.rin; d.H = p.rout; d.W = p.rout; }
            with_stats(c, d, b.ds_stats, p.cout, p.rout * p.rout, 1);
            TRY(gemm_fwd(c, d, (size_t)Min * p.cin, (size_t)p.cout * p.cin));   // (x3 only for the un-strided form: gemm_fwd checks)
        }
        {
            TRY(launch_ws_conv_w(c.W(p.c1_w), b.w_c1, 2, p.mid, p.cin, 1, p.cin, kWsEps, st, err));
            IgemmDesc d;
            d.X = b.xin; d.Wt = b.w_c1; d.M = Min; d.N = p.mid; d.Cin = p.cin; d.ldx = p.cin; d.out_f32 = b.c1_raw;
            with_stats(c, d, b.c1_stats, p.mid, p.rin * p.rin);
            TRY(gemm_fwd(c, d, (size_t)Min * p.cin, (size_t)p.mid * p.cin));
            GnApplyArgs g;
            g.raw = b.c1_raw; g.stats = b.c1_stats; g.gamma = c.W(p.n1.g); g.beta = c.W(p.n1.b); g.out_halo = b.t1;
            g.M = (size_t)Min; g.HW = p.rin * p.rin; g.W = p.rin; g.C = p.mid; g.cpg = p.mid / 32;
            from_partials(c, g, 0);
            TRY(launch_gn_apply(g, 2, st, err));
        }
        {
            TRY(launch_ws_conv_w(c.W(p.c2_w), b.w_c2, 2, p.mid, p.mid, 3, 9 * p.mid, kWsEps, st, err));
            IgemmDesc d;
            d.X = b.t1; d.Wt = b.w_c2; d.M = Mout; d.N = p.mid; d.Cin = p.mid; d.taps = 9; d.H = p.rout; d.W = p.rout; d.Hi = p.rin; d.Wi = p.rin;
            d.stride = p.stride; d.pad = p.stride == 1 ? 1 : 0; d.in_halo = 1; d.out_f32 = b.c2_raw;
            with_stats(c, d, b.c2_stats, p.mid, p.rout * p.rout);
            TRY(gemm_fwd(c, d, (size_t)B * (p.rin + 2) * (p.rin + 2) * p.mid, (size_t)9 * p.mid * p.mid));
            GnApplyArgs g;
            g.raw = b.c2_raw; g.stats = b.c2_stats; g.gamma = c.W(p.n2.g); g.beta = c.W(p.n2.b); g.out_op = b.t2;
            g.M = (size_t)Mout; g.HW = p.rout * p.rout; g.W = p.rout; g.C = p.mid; g.cpg = p.mid / 32;
            from_partials(c, g, 0);
            TRY(launch_gn_apply(g, 2, st, err));
        }
        {
            TRY(launch_ws_conv_w(c.W(p.c3_w), b.w_c3, 2, p.cout, p.mid, 1, p.mid, kWsEps, st, err));
            IgemmDesc d;
            d.X = b.t2; d.Wt = b.w_c3; d.M = Mout; d.N = p.cout; d.Cin = p.mid; d.ldx = p.mid; d.out_f32 = b.c3_raw;
            with_stats(c, d, b.c3_stats, p.cout, p.rout * p.rout);
            TRY(gemm_fwd(c, d, (size_t)Mout * p.mid, (size_t)p.cout * p.mid));
            GnApplyArgs g;
            g.raw = b.c3_raw; g.stats = b.c3_stats; g.gamma = c.W(p.n3.g); g.beta = c.W(p.n3.b);
            if (p.proj) { g.raw2 = b.ds_raw; g.stats2 = b.ds_stats; g.gamma2 = c.W(p.ds_n.g); g.beta2 = c.W(p.ds_n.b); }
            else g.res = b.xin;
            g.out_f32 = b.out;
            ++cnt;
            if (stage < 2 && cnt == a.rn_layers[stage]) g.out_halo = T.feat[hook++];   // hooks on stages[0], stages[1] (vit.py:164-167)
            g.M = (size_t)Mout; g.HW = p.rout * p.rout; g.W = p.rout; g.C = p.cout; g.cpg = p.cout / 32;
            from_partials(c, g, 0, p.proj ? 1 : -1);
            TRY(launch_gn_apply(g, 2, st, err));
            if (cnt == a.rn_layers[stage]) { ++stage; cnt = 0; }
        }
        xcur = b.out;
    }
    (void)H2;
    // ---- ViT-B over g*g + 1 tokens ----
    const int E = a.vit_dim, G = a.grid(), NT = G * G + 1, Mt = B * NT, Mp = B * G * G;
    {
        IgemmDesc d;
        d.X = xcur; d.Wt = c.W(P.pe.w); d.M = Mp; d.N = E; d.Cin = 1024; d.ldx = 1024; d.bias = c.W(P.pe.b); d.out_f32 = Y.pe_y;
        TRY(gemm(c, d));
        TRY(launch_vit_tokens_ln(Y.pe_y, c.W(P.cls), c.W(P.pos), Y.x0, c.W(P.vit[0].n1.g), c.W(P.vit[0].n1.b), Y.vb[0].ln1, 2,
                                 B, NT, E, kLnEps, st, err));
    }
    const float* tcur = Y.x0;
    for (int i = 0; i < a.vit_depth; ++i) {
        VitBlkT& v = Y.vb[i];
        const VitBlockP& p = P.vit[i];
        v.xin = tcur;
        if (i > 0) TRY(launch_ln_rows(const_cast<float*>(v.xin), c.W(p.n1.g), c.W(p.n1.b), v.ln1, 2, Mt, E, kLnEps, st, err));
        IgemmDesc d;
        d.X = v.ln1; d.Wt = c.W(p.qkv.w); d.M = Mt; d.N = 3 * E; d.Cin = E; d.ldx = E; d.bias = c.W(p.qkv.b); d.out_f32 = v.qkv;
        TRY(gemm_fwd(c, d, (size_t)Mt * E, (size_t)3 * E * E));   // x3 operands in the amp modes (train_step.cpp: gemm_fwd), exact f32 otherwise
        TRY(launch_vit_attention(v.qkv, v.attn, SOCCDPT_PREC_F32, B, NT, a.vit_heads, st, err));   // the exact-f32 MFMA kernel of the inference path (vit_attention.hip)
        d = IgemmDesc();
        d.X = v.attn; d.Wt = c.W(p.proj.w); d.M = Mt; d.N = E; d.Cin = E; d.ldx = E; d.bias = c.W(p.proj.b); d.res1 = v.xin; d.out_f32 = v.x1;
        TRY(gemm_fwd(c, d, (size_t)Mt * E, (size_t)E * E));
        TRY(launch_ln_rows(v.x1, c.W(p.n2.g), c.W(p.n2.b), v.ln2, 2, Mt, E, kLnEps, st, err));
        d = IgemmDesc();
        d.X = v.ln2; d.Wt = c.W(p.fc1.w); d.M = Mt; d.N = 4 * E; d.Cin = E; d.ldx = E; d.bias = c.W(p.fc1.b); d.act = ACT_GELU;
        d.out_f32 = v.hpre; d.out_op = v.hact;
        TRY(gemm_fwd(c, d, (size_t)Mt * E, (size_t)4 * E * E));
        d = IgemmDesc();
        d.X = v.hact; d.Wt = c.W(p.fc2.w); d.M = Mt; d.N = E; d.Cin = 4 * E; d.ldx = 4 * E; d.bias = c.W(p.fc2.b); d.res1 = v.x1; d.out_f32 = v.xout;
        TRY(gemm_fwd(c, d, (size_t)Mt * 4 * E, (size_t)4 * E * E));
        tcur = v.xout;
    }
    // ---- act_postprocess3 / 4: ProjectReadout -> Conv1x1 (-> Conv3x3 / 2) ----
    for (int k = 0; k < 2; ++k) {
        const ReadoutP& ro = P.ro[k];
        TRY(th_readout_cat(Y.vb[a.vit_hooks[k]].xout, Y.cat[k], B, NT, E, st, err));
        IgemmDesc d;
        d.X = Y.cat[k]; d.Wt = c.W(ro.project.w); d.M = Mp; d.N = E; d.Cin = 2 * E; d.ldx = 2 * E; d.bias = c.W(ro.project.b); d.act = ACT_GELU;
        d.out_f32 = Y.ro_pre[k]; d.out_op = Y.ro_act[k];
        TRY(gemm(c, d));
        d = IgemmDesc();
        d.X = Y.ro_act[k]; d.Wt = c.W(ro.conv.w); d.M = Mp; d.N = a.fdim(2 + k); d.Cin = E; d.ldx = E; d.bias = c.W(ro.conv.b); d.H = G; d.W = G;
        d.out_op = k == 0 ? T.feat[2] : Y.pp4_in; d.out_halo = 1;
        TRY(gemm(c, d));
        if (k == 1) {
            TRY(launch_conv_w(c.W(P.pp4.w), nullptr, Y.w_pp4, 1, 0, a.fdim(3), a.fdim(3), st, err));
            d = IgemmDesc();
            d.X = Y.pp4_in; d.Wt = Y.w_pp4; d.M = B * (G / 2) * (G / 2); d.N = a.fdim(3); d.Cin = a.fdim(3); d.taps = 9; d.H = G / 2; d.W = G / 2; d.Hi = G; d.Wi = G;
            d.stride = 2; d.pad = 1; d.in_halo = 1; d.bias = c.W(P.pp4.b); d.out_op = T.feat[3]; d.out_halo = 1;
            TRY(gemm(c, d));
        }
    }
    return 0;
}

int hy_backward(Ctx& c) {
    Handle& h = c.h;
    const Arch& a = h.arch;
    Tape& T = c.T;
    HyTape& Y = T.hy;
    const int B = c.B;
    hipStream_t st = c.st;
    std::string& err = c.err;
    float** G = T.G;
    const HybridP& P = h.params.hy;
    const int E = a.vit_dim, Gd = a.grid(), NT = Gd * Gd + 1;
    const size_t Mt = (size_t)B * NT, Mp = (size_t)B * Gd * Gd;
    // re-derive the input pointers of the forward walk
    {
        const float* xcur = Y.pool;
        for (auto& b : Y.blk) { b.xin = xcur; xcur = b.out; }
        const float* tcur = Y.x0;
        for (auto& v : Y.vb) { v.xin = tcur; tcur = v.xout; }
    }
    // weight-standardised convolution: gradient of the standardised weights (tap-major, in S_dw) -> parameter gradient
    auto ws_grad = [&](PRef key, const float* wh, int Cout, int Cin, int k, int Kpad) -> int {
        float* dw = c.Gd(key);
        if (!dw) return 0;
        return th_ws_bwd(T.S_dw, wh, c.W(key), dw, Cout, Cin, k, Kpad, kWsEps, st, err);
    };
    // ---- read-outs: gradient of a hooked token stream from the gradient of its reassembled map ----
    auto readout_bwd = [&](int k, int accumulate) -> int {
        const ReadoutP& ro = P.ro[k];
        const float* dmap = T.DF[2 + k];
        if (k == 1) {   // Conv2d(768, 768, 3, stride 2, padding 1)
            TRY(conv_gen_bwd(c, dmap, Y.pp4_in, Y.w_pp4, Gd, Gd / 2, a.fdim(3), a.fdim(3), 2, 1, G[0], c.Gd(P.pp4.w) ? T.S_dw : nullptr, c.Gd(P.pp4.b)));
            if (float* dw = c.Gd(P.pp4.w)) TRY(tr_wgrad_permute(T.S_dw, dw, a.fdim(3), a.fdim(3), st, err));
            dmap = G[0];
        }
        TRY(linear_bwd(c, dmap, Y.ro_act[k], c.W(ro.conv.w), Mp, a.fdim(2 + k), E, G[1], nullptr, c.Gd(ro.conv.w), c.Gd(ro.conv.b)));
        TRY(tr_gelu_bwd(G[1], Y.ro_pre[k], G[1], Mp * E, st, err));
        TRY(linear_bwd(c, G[1], Y.cat[k], c.W(ro.project.w), Mp, E, 2 * E, G[2], nullptr, c.Gd(ro.project.w), c.Gd(ro.project.b)));
        TRY(th_readout_cat_bwd(G[2], Y.GT, B, NT, E, accumulate, st, err));
        return 0;
    };
    // ---- ViT blocks, last -> first ----
    for (int i = a.vit_depth - 1; i >= 0; --i) {
        if (i == a.vit_hooks[1]) TRY(readout_bwd(1, 0));     // blocks[11] is the last block: its output reaches the outputs through the read-out only
        if (i == a.vit_hooks[0]) TRY(readout_bwd(0, 1));
        if (i > a.vit_hooks[1]) continue;
        VitBlkT& v = Y.vb[i];
        const VitBlockP& p = P.vit[i];
        // xout = x1 + fc2(gelu(fc1(LN2(x1))))
        TRY(linear_bwd(c, Y.GT, v.hact, c.W(p.fc2.w), Mt, E, 4 * E, G[0], nullptr, c.Gd(p.fc2.w), c.Gd(p.fc2.b)));
        TRY(tr_gelu_bwd(G[0], v.hpre, G[0], Mt * 4 * E, st, err));
        TRY(linear_bwd(c, G[0], v.ln2, c.W(p.fc1.w), Mt, 4 * E, E, G[1], nullptr, c.Gd(p.fc1.w), c.Gd(p.fc1.b)));
        TRY(ln_bwd(c, v.x1, c.W(p.n2.g), G[1], G[2], G[3], Mt, E, c.Gd(p.n2.g), c.Gd(p.n2.b), kLnEps));
        TRY(tr_axpy(G[2], Y.GT, Mt * E, st, err));                                   // G2 = d x1
        // x1 = xin + proj(attn(qkv(LN1(xin))))
        TRY(linear_bwd(c, G[2], v.attn, c.W(p.proj.w), Mt, E, E, G[0], nullptr, c.Gd(p.proj.w), c.Gd(p.proj.b)));
        // 16-bit products in the 16-bit amp modes (autocast semantics), exact ones otherwise; v.rowstat is this launch's scratch ({m + ln l, delta} per query)
        const OpFmt attn_fmt = op_is16(amp_fmt(c)) ? amp_fmt(c) : OpFmt::F32;
        TRY(th_vit_attention_bwd_mfma(v.qkv, v.attn, G[0], v.rowstat, G[4], B, NT, a.vit_heads, st, err, attn_fmt));
        TRY(linear_bwd(c, G[4], v.ln1, c.W(p.qkv.w), Mt, 3 * E, E, G[1], nullptr, c.Gd(p.qkv.w), c.Gd(p.qkv.b)));
        TRY(ln_bwd(c, v.xin, c.W(p.n1.g), G[1], G[0], G[3], Mt, E, c.Gd(p.n1.g), c.Gd(p.n1.b), kLnEps));
        TRY(copy_d2d(c, Y.GT, G[2], Mt * E * 4, "hy_backward"));
        TRY(tr_axpy(Y.GT, G[0], Mt * E, st, err));                                   // GT = d xin
    }
    // ---- tokens = cat(cls, proj(features)) + pos_embed ----
    {
        float* dpos = c.Gd(P.pos);
        float* dcls = c.Gd(P.cls);
        if (dpos || dcls) {
            // sum over the batch of the token-stream gradient: [B][NT*E] -> [NT*E]  (tr_colsum: rows = samples)
            float* tmp = dpos ? dpos : G[3];
            TRY(tr_colsum(Y.GT, nullptr, tmp, T.S_col, (size_t)B, NT * E, 0, st, err));
            if (dcls) TRY(copy_d2d(c, dcls, tmp, (size_t)E * 4, "hy_backward"));
        }
        TRY(th_tokens_to_patches(Y.GT, G[0], B, NT, E, st, err));
        TRY(linear_bwd(c, G[0], Y.blk.back().out, c.W(P.pe.w), Mp, E, 1024, Y.GR, nullptr, c.Gd(P.pe.w),
                       c.Gd(P.pe.b)));
    }
    // ---- ResNetV2 stages, last block -> first ----
    int stage = 2, cnt = a.rn_layers[2];
    for (int bi = (int)Y.blk.size() - 1; bi >= 0; --bi) {
        RnBlkT& b = Y.blk[bi];
        const RnBlockP& p = P.rn[bi];
        const size_t Min = (size_t)B * p.rin * p.rin, Mout = (size_t)B * p.rout * p.rout;
        if (stage < 2 && cnt == a.rn_layers[stage]) TRY(tr_axpy(Y.GR, T.DF[stage], Mout * p.cout, st, err));   // hooked stage output
        // out = relu(GN3(conv3(t2)) + shortcut)
        TRY(tr_relu_bwd(Y.GR, b.out, nullptr, G[0], Mout * p.cout, st, err));                       // G0 = d (sum)
        TRY(th_gn_bwd(G[0], b.c3_raw, b.c3_stats, c.W(p.n3.g), c.W(p.n3.b), G[1], c.Gd(p.n3.g), c.Gd(p.n3.b), T.S_col, B,
                      p.rout * p.rout, p.cout, p.cout / 32, 0, st, err));
        TRY(linear_bwd(c, G[1], b.t2, b.w_c3, Mout, p.cout, p.mid, G[2], nullptr, c.Gd(p.c3_w) ? T.S_dw : nullptr, nullptr));
        TRY(ws_grad(p.c3_w, b.w_c3, p.cout, p.mid, 1, p.mid));
        TRY(th_gn_bwd(G[2], b.c2_raw, b.c2_stats, c.W(p.n2.g), c.W(p.n2.b), G[2], c.Gd(p.n2.g), c.Gd(p.n2.b), T.S_col, B,
                      p.rout * p.rout, p.mid, p.mid / 32, 1, st, err));
        TRY(conv_gen_bwd(c, G[2], b.t1, b.w_c2, p.rin, p.rout, p.mid, p.mid, p.stride, p.stride == 1 ? 1 : 0, G[1], c.Gd(p.c2_w) ? T.S_dw : nullptr, nullptr));
        TRY(ws_grad(p.c2_w, b.w_c2, p.mid, p.mid, 3, 9 * p.mid));
        TRY(th_gn_bwd(G[1], b.c1_raw, b.c1_stats, c.W(p.n1.g), c.W(p.n1.b), G[1], c.Gd(p.n1.g), c.Gd(p.n1.b), T.S_col, B,
                      p.rin * p.rin, p.mid, p.mid / 32, 1, st, err));
        TRY(linear_bwd(c, G[1], b.xin, b.w_c1, Min, p.mid, p.cin, G[3], nullptr, c.Gd(p.c1_w) ? T.S_dw : nullptr, nullptr));   // G3 = d xin (conv path)
        TRY(ws_grad(p.c1_w, b.w_c1, p.mid, p.cin, 1, p.cin));
        if (!p.proj) {
            TRY(tr_axpy(G[3], G[0], Min * p.cin, st, err));                                        // identity shortcut
        } else {
            TRY(th_gn_bwd(G[0], b.ds_raw, b.ds_stats, c.W(p.ds_n.g), c.W(p.ds_n.b), G[2], c.Gd(p.ds_n.g),
                          c.Gd(p.ds_n.b), T.S_col, B, p.rout * p.rout, p.cout, p.cout / 32, 0, st, err));
            const float* xs = b.xin;
            if (p.stride != 1) { TRY(th_stride_gather(b.xin, Y.xg, B, p.rin, p.rout, p.cin, p.stride, st, err)); xs = Y.xg; }
            TRY(linear_bwd(c, G[2], xs, b.w_ds, Mout, p.cout, p.cin, G[1], nullptr, c.Gd(p.ds_w) ? T.S_dw : nullptr, nullptr));
            TRY(ws_grad(p.ds_w, b.w_ds, p.cout, p.cin, 1, p.cin));
            if (p.stride == 1) TRY(tr_axpy(G[3], G[1], Min * p.cin, st, err));
            else TRY(th_stride_scatter_add(G[1], G[3], B, p.rin, p.rout, p.cin, p.stride, st, err));
        }
        TRY(copy_d2d(c, Y.GR, G[3], Min * p.cin * 4, "hy_backward"));
        if (--cnt == 0 && stage > 0) { --stage; cnt = a.rn_layers[stage]; }
    }
    // ---- stem ----
    {
        const int H1 = a.img / 2;
        const size_t M1s = (size_t)B * H1 * H1;
        float* dwk = c.Gd(P.stem_w);
        float* dg = c.Gd(P.stem_n.g);
        float* dbt = c.Gd(P.stem_n.b);
        if (dwk || dg || dbt) {
            TRY(th_maxpool_bwd(Y.GR, Y.stem_raw, Y.stem_stats, c.W(P.stem_n.g), c.W(P.stem_n.b), Y.pool_idx, G[0], B, H1, a.stem_ch, a.stem_ch / 32, st,
                               err));
            TRY(th_gn_bwd(G[0], Y.stem_raw, Y.stem_stats, c.W(P.stem_n.g), c.W(P.stem_n.b), G[0], dg, dbt, T.S_col, B, H1 * H1, a.stem_ch,
                          a.stem_ch / 32, 1, st, err));
            if (dwk) {
                TRY(linear_bwd(c, G[0], Y.a0, nullptr, M1s, a.stem_ch, 160, nullptr, nullptr, T.S_dw, nullptr));
                TRY(th_ws_bwd(T.S_dw, Y.w_stem, c.W(P.stem_w), dwk, a.stem_ch, 3, 7, 160, kWsEps, st, err));
            }
        }
    }
    return 0;
}

}  // namespace trn
}  // namespace soccdpt
