// Stand-alone driver of soccdpt_amd/csrc/params.h for tests/test_params_cpu.py (host compiler, address + undefined sanitizers): the parameter table
// of the three backbones without a GPU.
//
//   params_main      features 256, 3 classes; one JSON line per backbone:
//     keys   [[key, [shape]], ...]        in registration order
//     refs   {"<field path>": index, ...}   every reference of ModelP (-1: the model has no such tensor)
//     spans  {"<field path>": [lo, hi], ...}
//     rn     [[cin, cout, mid, stride, rin, rout, proj], ...]   geometry of the ResNetV2 bottlenecks (hybrid only)
#include <cstdio>
#include <string>
#include <vector>

#include "../soccdpt_amd/csrc/params.h"

using namespace soccdpt;

namespace {

struct Emit {
    std::string refs, spans;
    void ref(const std::string& name, PRef r) { refs += (refs.empty() ? "\"" : ", \"") + name + "\": " + std::to_string(r.i); }
    void span(const std::string& name, Span s) {
        spans += (spans.empty() ? "\"" : ", \"") + name + "\": [" + std::to_string(s.lo) + ", " + std::to_string(s.hi) + "]";
    }
    void wb(const std::string& name, const WB& p) { ref(name + ".w", p.w); ref(name + ".b", p.b); }
    void gb(const std::string& name, const GB& p) { ref(name + ".g", p.g); ref(name + ".b", p.b); }
};

void dump(const char* backbone, const Arch& a) {
    std::vector<WeightSlot> w;
    const ModelP P = build_params(a, 256, 3, w);
    Emit e;
    auto n = [](size_t v) { return std::to_string(v); };
    const SwinP& S = P.swin;
    e.wb("swin.patch", S.patch);
    e.gb("swin.patch_norm", S.patch_norm);
    for (int s = 0; s < 4; ++s) {
        for (size_t j = 0; j < S.blk[s].size(); ++j) {
            const SwinBlockP& b = S.blk[s][j];
            const std::string k = "swin.blk." + n(s) + "." + n(j);
            e.ref(k + ".logit_scale", b.logit_scale); e.ref(k + ".q_bias", b.q_bias); e.ref(k + ".v_bias", b.v_bias);
            e.ref(k + ".cpb0_w", b.cpb0_w); e.ref(k + ".cpb0_b", b.cpb0_b); e.ref(k + ".cpb2_w", b.cpb2_w); e.ref(k + ".qkv_w", b.qkv_w);
            e.wb(k + ".proj", b.proj); e.gb(k + ".n1", b.n1); e.wb(k + ".fc1", b.fc1); e.wb(k + ".fc2", b.fc2); e.gb(k + ".n2", b.n2);
            e.span(k + ".upto", b.upto);
        }
        e.span("swin.below." + n(s), S.below[s]);
        if (s < 3) { e.ref("swin.merge." + n(s) + ".red_w", S.merge[s].red_w); e.gb("swin.merge." + n(s) + ".norm", S.merge[s].norm); }
    }
    const HybridP& Y = P.hy;
    e.ref("hy.cls", Y.cls); e.ref("hy.pos", Y.pos); e.ref("hy.stem_w", Y.stem_w); e.gb("hy.stem_n", Y.stem_n);
    std::string rn;
    for (size_t i = 0; i < Y.rn.size(); ++i) {
        const RnBlockP& b = Y.rn[i];
        const std::string k = "hy.rn." + n(i);
        e.ref(k + ".ds_w", b.ds_w); e.gb(k + ".ds_n", b.ds_n);
        e.ref(k + ".c1_w", b.c1_w); e.gb(k + ".n1", b.n1); e.ref(k + ".c2_w", b.c2_w); e.gb(k + ".n2", b.n2); e.ref(k + ".c3_w", b.c3_w); e.gb(k + ".n3", b.n3);
        char buf[128];
        snprintf(buf, sizeof(buf), "%s[%d, %d, %d, %d, %d, %d, %d]", i ? ", " : "", b.cin, b.cout, b.mid, b.stride, b.rin, b.rout, b.proj ? 1 : 0);
        rn += buf;
    }
    e.wb("hy.pe", Y.pe);
    for (size_t i = 0; i < Y.vit.size(); ++i) {
        const VitBlockP& b = Y.vit[i];
        const std::string k = "hy.vit." + n(i);
        e.gb(k + ".n1", b.n1); e.wb(k + ".qkv", b.qkv); e.wb(k + ".proj", b.proj); e.gb(k + ".n2", b.n2); e.wb(k + ".fc1", b.fc1); e.wb(k + ".fc2", b.fc2);
    }
    for (int k = 0; k < 2; ++k) { e.wb("hy.ro." + n(k) + ".project", Y.ro[k].project); e.wb("hy.ro." + n(k) + ".conv", Y.ro[k].conv); }
    e.wb("hy.pp4", Y.pp4);
    e.span("encoder", P.encoder);
    for (int l = 0; l < 4; ++l) {
        const RefineP& R = P.refine[l];
        const std::string k = "refine." + n(l);
        e.ref("layer_rn." + n(l), P.layer_rn[l]);
        e.wb(k + ".out_conv", R.out_conv);
        e.span(k + ".out_conv", R.out_conv_span);
        for (int u = 0; u < 2; ++u) {
            e.wb(k + ".rcu." + n(u) + ".c1", R.rcu[u].c1); e.wb(k + ".rcu." + n(u) + ".c2", R.rcu[u].c2);
            e.span(k + ".rcu." + n(u), R.rcu_span[u]);
        }
    }
    e.wb("depth.c0", P.depth.c0); e.wb("depth.c2", P.depth.c2); e.wb("depth.c4", P.depth.c4);
    e.ref("seg.c0_w", P.seg.c0_w); e.gb("seg.bn", P.seg.bn); e.ref("seg.bn_mean", P.seg.bn_mean); e.ref("seg.bn_var", P.seg.bn_var); e.wb("seg.c4", P.seg.c4);

    printf("{\"backbone\": \"%s\", \"keys\": [", backbone);
    for (size_t i = 0; i < w.size(); ++i) {
        printf("%s[\"%s\", [", i ? ", " : "", w[i].key.c_str());
        for (size_t d = 0; d < w[i].shape.size(); ++d) printf("%s%lld", d ? ", " : "", (long long)w[i].shape[d]);
        printf("]]");
    }
    printf("], \"refs\": {%s}, \"spans\": {%s}, \"rn\": [%s]}\n", e.refs.c_str(), e.spans.c_str(), rn.c_str());
}

}  // namespace

int main() {
    dump("swin2t16_256", arch_swin2t16_256());
    dump("swin2b24_384", arch_swin2b24_384());
    dump("vitb_rn50_384", arch_vitb_rn50_384());
    return 0;
}
