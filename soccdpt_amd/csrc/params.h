// The parameter table of SOccDPT_V3, stated once (host-only: no HIP header).  build_params() walks the architecture a single time and registers
// every state-dict key with its shape AND the typed reference its consumers read it through, so a tensor is named in one place; the forward
// (model.cpp), the training step (train_step.cpp, train_hybrid_step.cpp) and the calibration fingerprint read Handle::weights through the
// references of ModelP.  Only the by-name entry points of the API (soccdpt_bind_weight, soccdpt_bind_grad) look a key up.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace soccdpt {

// Swin-V2 geometry (timm swinv2_* as created by /root/reference/SOccDPT/model/backbones/swin2.py:15-30;
// hooks from /root/reference/SOccDPT/model/dpt.py:67-72).
struct Arch {
    int img = 256, patch = 4, embed = 96, window = 16;
    int depths[4] = {2, 2, 6, 2};
    int heads[4] = {3, 6, 12, 24};
    int pretrained_window[4] = {0, 0, 0, 0};
    int hooks[4] = {1, 1, 5, 1};
    // ViT-hybrid (vitb_rn50_384; /root/reference/SOccDPT/model/backbones/vit.py:147-258, model/blocks.py:103-112): ResNetV2 (3, 4, 9) stem +
    // 12 ViT-B blocks; the reassembled pyramid is [256, 512, 768, 768] channels at 1/4, 1/8, 1/16, 1/32 of the input
    // Swin-V1 block (swinl12_384, timm swin_large_patch4_window12_384; hooks /root/reference/SOccDPT/model/dpt.py:73-78): pre-norm, scaled dot-product
    // attention with a learned relative-position-bias table and a full qkv bias, PatchMerging = gather, LayerNorm(4C), reduction.  pretrained_window is unused.
    bool swin1 = false;
    bool hybrid = false;
    int vit_depth = 12, vit_heads = 12, vit_dim = 768, stem_ch = 64;
    int rn_layers[3] = {3, 4, 9};
    int vit_hooks[2] = {8, 11};
    int grid() const { return img / patch; }
    int dim(int s) const { return embed << s; }
    int res(int s) const { return grid() >> s; }
    // feature pyramid handed to scratch.layerN_rn (level l = 0 finest)
    int fdim(int l) const { return hybrid ? (l == 0 ? 256 : l == 1 ? 512 : 768) : dim(l); }
    int fres(int l) const { return hybrid ? (img / 4) >> l : res(l); }
    int out_res() const { return img; }   // network output resolution (4 * fres(0))
    int ws(int s) const { return res(s) < window ? res(s) : window; }
    int shift(int s, int j) const { return (j % 2 == 0 || res(s) <= window) ? 0 : window / 2; }
};
inline Arch arch_swin2t16_256() { return Arch{}; }
inline Arch arch_swin2b24_384() {
    Arch a;
    a.img = 384; a.embed = 128; a.window = 24;
    const int d[4] = {2, 2, 18, 2}, hd[4] = {4, 8, 16, 32}, pw[4] = {12, 12, 12, 6}, hk[4] = {1, 1, 17, 1};
    for (int i = 0; i < 4; ++i) { a.depths[i] = d[i]; a.heads[i] = hd[i]; a.pretrained_window[i] = pw[i]; a.hooks[i] = hk[i]; }
    return a;
}
// swinv2_large_window12to24_192to384_22kft1k: base's depths, windows and hooks at embed 192, heads (6, 12, 24, 48); stage 3 is 1536 wide
inline Arch arch_swin2l24_384() {
    Arch a = arch_swin2b24_384();
    a.embed = 192;
    const int hd[4] = {6, 12, 24, 48};
    for (int i = 0; i < 4; ++i) a.heads[i] = hd[i];
    return a;
}
// swin_large_patch4_window12_384: Swin-V2-L's widths, depths, heads and hooks with 12 x 12 windows at every stage (stage 3: res == window, unshifted)
inline Arch arch_swinl12_384() {
    Arch a = arch_swin2l24_384();
    a.swin1 = true; a.window = 12;
    for (int i = 0; i < 4; ++i) a.pretrained_window[i] = 0;
    return a;
}
inline Arch arch_vitb_rn50_384() {
    Arch a;
    a.hybrid = true; a.img = 384; a.patch = 16;
    return a;
}

struct WeightSlot {
    std::string key;
    std::vector<int64_t> shape;
    const float* ptr = nullptr;
    float* grad = nullptr;   // gradient destination of the training step (soccdpt_bind_grad); nullptr = frozen
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};

// A tensor of the model: index into Handle::weights, -1 = this model has no such tensor
struct PRef { int i = -1; };
// Registration order is module order, so "the tensors of this module" is a run of indices [lo, hi); lo == hi (the default) is the empty span
struct Span { int lo = 0, hi = 0; };
inline Span span_of(PRef r) { return r.i < 0 ? Span{} : Span{r.i, r.i + 1}; }

struct WB { PRef w, b; };   // <module>.weight, <module>.bias
struct GB { PRef g, b; };   // the same pair of a normalisation layer: gamma, beta
struct SwinBlockP {          // timm SwinTransformerV2Block; Swin-V1 (Arch::swin1): rpb_table, qkv_w, qkv_b instead of the first six
    PRef logit_scale, q_bias, v_bias, cpb0_w, cpb0_b, cpb2_w, qkv_w;
    PRef rpb_table, qkv_b;   // attn.relative_position_bias_table [(2 ws - 1)^2][H], attn.qkv.bias [3C]
    WB proj;
    GB n1;
    WB fc1, fc2;
    GB n2;
    Span upto;               // everything of the encoder at or before this block in forward order
};
struct MergeP { PRef red_w; GB norm; };   // PatchMerging of Swin-V2: reduction, then norm [2C]; of Swin-V1: norm [4C], then reduction
struct RnBlockP {            // ResNetV2 bottleneck (weight-standardised convolutions + GroupNorm) and its geometry
    int cin = 0, cout = 0, mid = 0, stride = 1, rin = 0, rout = 0;
    bool proj = false;       // the first block of a stage: shortcut projection ds_w / ds_n
    PRef ds_w, c1_w, c2_w, c3_w;
    GB ds_n, n1, n2, n3;
};
struct VitBlockP { GB n1; WB qkv, proj; GB n2; WB fc1, fc2; };
struct ReadoutP { WB project, conv; };    // act_postprocess<n>: ProjectReadout Linear, Conv1x1
struct RcuP { WB c1, c2; };               // ResidualConvUnit
struct SwinP {
    WB patch;
    GB patch_norm;
    std::vector<SwinBlockP> blk[4];
    MergeP merge[3];         // downsample of stage s: registered after stage s's blocks
    Span below[4];           // patch_embed and every stage before s
};
struct HybridP {
    PRef cls, pos, stem_w;
    GB stem_n;
    std::vector<RnBlockP> rn;   // the bottlenecks of the three stages in forward order (Arch::rn_layers of each)
    WB pe;
    std::vector<VitBlockP> vit;
    ReadoutP ro[2];
    WB pp4;                  // act_postprocess4.4: Conv3x3 / 2
};
struct RefineP {             // scratch.refinenet<l + 1>; level 3 (refinenet4) has a single input and no rcu[0]
    WB out_conv;
    RcuP rcu[2];
    Span out_conv_span, rcu_span[2];
};
struct DepthHeadP { WB c0, c2, c4; };                        // scratch.output_conv.{0, 2, 4}
struct SegHeadP { PRef c0_w; GB bn; PRef bn_mean, bn_var; WB c4; };
struct ModelP {
    SwinP swin;              // one of the two encoders: Arch::hybrid says which
    HybridP hy;
    Span encoder;            // depth_net.pretrained.*
    PRef layer_rn[4];
    RefineP refine[4];
    DepthHeadP depth;
    SegHeadP seg;
};

// The one walk over the architecture: appends every consumed tensor to `out` in state-dict order (soccdpt_num_weights / soccdpt_weight_key
// iterate it) and returns the references.  No other function of the library spells a state-dict key.
inline ModelP build_params(const Arch& a, int features, int num_classes, std::vector<WeightSlot>& out) {
    typedef std::vector<int64_t> Shape;
    ModelP P;
    auto n = [](int v) { return std::to_string(v); };
    auto here = [&]() { return (int)out.size(); };
    auto add = [&](const std::string& key, Shape shape) {
        out.push_back(WeightSlot{key, std::move(shape)});
        return PRef{here() - 1};
    };
    auto wb = [&](const std::string& m, Shape w, int64_t nb) { WB r; r.w = add(m + ".weight", std::move(w)); r.b = add(m + ".bias", {nb}); return r; };
    auto gb = [&](const std::string& m, int64_t c) { GB r; r.g = add(m + ".weight", {c}); r.b = add(m + ".bias", {c}); return r; };
    const std::string PRE = "depth_net.pretrained.", ENC = PRE + "model.", SCR = "depth_net.scratch.";
    P.encoder.lo = here();
    if (a.hybrid) {
        // timm 0.6.12 vit_base_resnet50_384 + the reference's act_postprocess3/4 (backbones/vit.py:183-229): SURVEY.md 8a row a4-H
        HybridP& Y = P.hy;
        const int64_t E = a.vit_dim, NT = (int64_t)a.grid() * a.grid() + 1;
        Y.cls = add(ENC + "cls_token", {1, 1, E});
        Y.pos = add(ENC + "pos_embed", {1, NT, E});
        const std::string bb = ENC + "patch_embed.backbone.";
        Y.stem_w = add(bb + "stem.conv.weight", {a.stem_ch, 3, 7, 7});
        Y.stem_n = gb(bb + "stem.norm", a.stem_ch);
        int prev = a.stem_ch, r = a.img / 4;
        for (int s = 0; s < 3; ++s) {
            const int cout = 256 << s, mid = cout / 4;
            for (int j = 0; j < a.rn_layers[s]; ++j) {
                const std::string b = bb + "stages." + n(s) + ".blocks." + n(j) + ".";
                RnBlockP p;
                p.cin = prev; p.cout = cout; p.mid = mid; p.proj = j == 0; p.stride = (j == 0 && s > 0) ? 2 : 1;
                p.rin = r; p.rout = r / p.stride;
                if (p.proj) {
                    p.ds_w = add(b + "downsample.conv.weight", {cout, prev, 1, 1});
                    p.ds_n = gb(b + "downsample.norm", cout);
                }
                p.c1_w = add(b + "conv1.weight", {mid, prev, 1, 1});
                p.n1 = gb(b + "norm1", mid);
                p.c2_w = add(b + "conv2.weight", {mid, mid, 3, 3});
                p.n2 = gb(b + "norm2", mid);
                p.c3_w = add(b + "conv3.weight", {cout, mid, 1, 1});
                p.n3 = gb(b + "norm3", cout);
                Y.rn.push_back(p);
                prev = cout;
                r = p.rout;
            }
        }
        Y.pe = wb(ENC + "patch_embed.proj", {E, prev, 1, 1}, E);
        for (int i = 0; i < a.vit_depth; ++i) {
            const std::string b = ENC + "blocks." + n(i) + ".";
            VitBlockP v;
            v.n1 = gb(b + "norm1", E);
            v.qkv = wb(b + "attn.qkv", {3 * E, E}, 3 * E);
            v.proj = wb(b + "attn.proj", {E, E}, E);
            v.n2 = gb(b + "norm2", E);
            v.fc1 = wb(b + "mlp.fc1", {4 * E, E}, 4 * E);
            v.fc2 = wb(b + "mlp.fc2", {E, 4 * E}, E);
            Y.vit.push_back(v);
        }
        for (int k = 0; k < 2; ++k) {
            const std::string ap = PRE + "act_postprocess" + n(3 + k) + ".";
            Y.ro[k].project = wb(ap + "0.project.0", {E, 2 * E}, E);
            Y.ro[k].conv = wb(ap + "3", {a.fdim(2 + k), E, 1, 1}, a.fdim(2 + k));
        }
        Y.pp4 = wb(PRE + "act_postprocess4.4", {a.fdim(3), a.fdim(3), 3, 3}, a.fdim(3));
    } else {
        SwinP& S = P.swin;
        const int64_t C0 = a.embed;
        S.patch = wb(ENC + "patch_embed.proj", {C0, 3, a.patch, a.patch}, C0);
        S.patch_norm = gb(ENC + "patch_embed.norm", C0);
        for (int s = 0; s < 4; ++s) {
            const int64_t C = a.dim(s), H = a.heads[s];
            S.below[s] = Span{P.encoder.lo, here()};
            for (int j = 0; j < a.depths[s]; ++j) {
                const std::string b = ENC + "layers." + n(s) + ".blocks." + n(j) + ".";
                SwinBlockP p;
                if (a.swin1) {   // timm 0.6.12 SwinTransformerBlock; the buffers (attn.relative_position_index, attn_mask) are never consumed
                    const int64_t T = (int64_t)(2 * a.ws(s) - 1) * (2 * a.ws(s) - 1);
                    p.n1 = gb(b + "norm1", C);
                    p.rpb_table = add(b + "attn.relative_position_bias_table", {T, H});
                    p.qkv_w = add(b + "attn.qkv.weight", {3 * C, C});
                    p.qkv_b = add(b + "attn.qkv.bias", {3 * C});
                    p.proj = wb(b + "attn.proj", {C, C}, C);
                    p.n2 = gb(b + "norm2", C);
                    p.fc1 = wb(b + "mlp.fc1", {4 * C, C}, 4 * C);
                    p.fc2 = wb(b + "mlp.fc2", {C, 4 * C}, C);
                    p.upto = Span{P.encoder.lo, here()};
                    S.blk[s].push_back(p);
                    continue;
                }
                p.logit_scale = add(b + "attn.logit_scale", {H, 1, 1});
                p.q_bias = add(b + "attn.q_bias", {C});
                p.v_bias = add(b + "attn.v_bias", {C});
                p.cpb0_w = add(b + "attn.cpb_mlp.0.weight", {512, 2});
                p.cpb0_b = add(b + "attn.cpb_mlp.0.bias", {512});
                p.cpb2_w = add(b + "attn.cpb_mlp.2.weight", {H, 512});
                p.qkv_w = add(b + "attn.qkv.weight", {3 * C, C});
                p.proj = wb(b + "attn.proj", {C, C}, C);
                p.n1 = gb(b + "norm1", C);
                p.fc1 = wb(b + "mlp.fc1", {4 * C, C}, 4 * C);
                p.fc2 = wb(b + "mlp.fc2", {C, 4 * C}, C);
                p.n2 = gb(b + "norm2", C);
                p.upto = Span{P.encoder.lo, here()};
                S.blk[s].push_back(p);
            }
            if (s < 3) {
                const std::string d = ENC + "layers." + n(s) + ".downsample.";
                S.merge[s].red_w = add(d + "reduction.weight", {2 * C, 4 * C});
                S.merge[s].norm = gb(d + "norm", a.swin1 ? 4 * C : 2 * C);
            }
        }
    }
    P.encoder.hi = here();
    const int64_t F = features;
    for (int l = 0; l < 4; ++l) P.layer_rn[l] = add(SCR + "layer" + n(l + 1) + "_rn.weight", {F, a.fdim(l), 3, 3});
    for (int l = 0; l < 4; ++l) {
        const std::string b = SCR + "refinenet" + n(l + 1) + ".";
        RefineP& R = P.refine[l];
        R.out_conv_span.lo = here();
        R.out_conv = wb(b + "out_conv", {F, F, 1, 1}, F);
        R.out_conv_span.hi = here();
        for (int u = 0; u < 2; ++u) {
            R.rcu_span[u].lo = R.rcu_span[u].hi = here();
            if (l == 3 && u == 0) continue;  // refinenet4 gets one input: its RCU1 never runs (model/dpt.py:163-165)
            R.rcu[u].c1 = wb(b + "resConfUnit" + n(u + 1) + ".conv1", {F, F, 3, 3}, F);
            R.rcu[u].c2 = wb(b + "resConfUnit" + n(u + 1) + ".conv2", {F, F, 3, 3}, F);
            R.rcu_span[u].hi = here();
        }
    }
    P.depth.c0 = wb(SCR + "output_conv.0", {F / 2, F, 3, 3}, F / 2);
    P.depth.c2 = wb(SCR + "output_conv.2", {32, F / 2, 3, 3}, 32);
    P.depth.c4 = wb(SCR + "output_conv.4", {1, 32, 1, 1}, 1);
    P.seg.c0_w = add("seg_head.0.weight", {F, F, 3, 3});
    P.seg.bn = gb("seg_head.1", F);
    P.seg.bn_mean = add("seg_head.1.running_mean", {F});
    P.seg.bn_var = add("seg_head.1.running_var", {F});
    P.seg.c4 = wb("seg_head.4", {num_classes, F, 1, 1}, num_classes);
    return P;
}

}  // namespace soccdpt
