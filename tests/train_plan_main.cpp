// Stand-alone driver of soccdpt_amd/csrc/train_plan.h for tests/test_train_plan_cpu.py (host compiler, address + undefined sanitizers): the scratch plans
// of the training backward without a GPU.
//
//   train_plan_main FILE      FILE holds one shape per line:  L M N K  |  C B r N C  |  G B Hi Ho N C stride pad
//
// Every shape is planned in the four operand formats and for every request (dX only, dW only, both; with and without a staged weight; sum deferred or
// not).  One JSON line per plan: the decisions, every layout number, the need, and what the helper that executes the plan (train_step.cpp,
// train_hybrid_step.cpp) does with the numbers:
//   spans  [region, label, first byte, end byte]   what it writes (zero fills separately) and the allowance its kernels may read behind that
//   views  [first element, end element]            S_T2 in elements of the operand format: what each tap of a shifted-view GEMM reads (igemm.h wt_*)
//   short  per region: fits() of the need against itself with that region one float short (null where the need is 0); fits: against itself
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../soccdpt_amd/csrc/train_plan.h"

using namespace soccdpt;
using namespace soccdpt::trn;

namespace {

const char* const kFmt[4] = {"f32", "bf16", "f16", "x3"};
const char* const kPath[7] = {"none", "tn", "transpose", "x3shift", "im2colT", "haloshift", "im2colT"};

struct Span { int region; const char* label; size_t lo, hi; };   // bytes
struct Out {
    std::vector<Span> spans;
    std::vector<std::pair<long long, long long>> views;
    size_t es;
    void add(int region, const char* label, size_t lo_elems, size_t n_elems, size_t es_ = 0) {
        const size_t e = es_ ? es_ : es;
        if (n_elems) spans.push_back(Span{region, label, lo_elems * e, (lo_elems + n_elems) * e});
    }
};
enum { T1 = 0, T2 = 1, HALO = 2, WT = 3, DW = 4 };

void emit_common(const char* kind, const long long* in, int nin, OpFmt mode, PlanReq q, OpFmt fmt, WgradPath wg, const ScratchNeed& need, const Out& o,
                 const std::string& extra) {
    printf("{\"kind\":\"%s\",\"in\":[", kind);
    for (int i = 0; i < nin; ++i) printf("%s%lld", i ? "," : "", in[i]);
    printf("],\"mode\":\"%s\",\"dX\":%d,\"dW\":%d,\"staged\":%d,\"defer\":%d,\"fmt\":\"%s\",\"wgrad\":\"%s\",%s", kFmt[(int)mode], q.dX, q.dW, q.staged_w, q.defer,
           kFmt[(int)fmt], kPath[(int)wg], extra.c_str());
    printf("\"need\":[%zu,%zu,%zu,%zu,%zu],\"spans\":[", need.t1, need.t2, need.halo, need.wt, need.dw);
    for (size_t i = 0; i < o.spans.size(); ++i)
        printf("%s[%d,\"%s\",%zu,%zu]", i ? "," : "", o.spans[i].region, o.spans[i].label, o.spans[i].lo, o.spans[i].hi);
    printf("],\"views\":[");
    for (size_t i = 0; i < o.views.size(); ++i) printf("%s[%lld,%lld]", i ? "," : "", o.views[i].first, o.views[i].second);
    printf("],\"fits\":%d,\"short\":[", need.fits(need) ? 1 : 0);
    for (int i = 0; i < 5; ++i) {
        ScratchNeed cap = need;
        if (need.*kRegion[i] == 0) { printf("%snull", i ? "," : ""); continue; }
        cap.*kRegion[i] -= 1;
        printf("%s%d", i ? "," : "", need.fits(cap) ? 1 : 0);
        if (need.misfit(cap).find(kRegionName[i]) != 0) fprintf(stderr, "misfit() does not name %s\n", kRegionName[i]);
    }
    printf("]}\n");
}

std::string kv(const char* k, long long v) { return std::string("\"") + k + "\":" + std::to_string(v) + ","; }

void linear(long long M, int N, int K, OpFmt mode, PlanReq q) {
    const LinearPlan p = plan_linear((size_t)M, N, K, mode, q);
    Out o;
    o.es = op_size(p.fmt);
    if (p.wgrad == WgradPath::TN) {   // linear_bwd: tr_cvt_pair, the zero rows, the kernel's over-read
        o.add(T1, "dY", 0, (size_t)M * N);
        o.add(T1, "zero rows", (size_t)M * N, (p.Mtn - M) * N);
        o.add(T1, "over-read", p.Mtn * N, kTnOverread);
        o.add(T2, "X", 0, (size_t)M * K);
        o.add(T2, "zero rows", (size_t)M * K, (p.Mtn - M) * K);
        o.add(T2, "over-read", p.Mtn * K, kTnOverread);
    } else {
        if (q.dX && p.fmt != OpFmt::F32 && !q.dW) o.add(T1, "dY", 0, (size_t)M * N);   // (with dW: overwritten by the transpose afterwards)
        if (q.dW) {
            o.add(T1, "dY^T", 0, (size_t)N * p.Mp);
            o.add(T2, "X^T", 0, (size_t)K * p.Mp);
        }
    }
    if (q.dX && !q.staged_w) o.add(WT, "W^T", 0, (size_t)N * K);
    const long long in[3] = {M, N, K};
    emit_common("linear", in, 3, mode, q, p.fmt, p.wgrad, p.need, o, kv("Mtn", (long long)p.Mtn) + kv("Mp", p.Mp) + kv("ldA", N) + kv("ldB", K));
}

std::string conv_fields(const ConvPlan& p, int N, int C) {
    return kv("col2im", p.col2im) + kv("rp", p.rp) + kv("Kh", (long long)p.Kh) + kv("Kp", (long long)p.Kp) + kv("mrg", (long long)p.mrg) + kv("rpp", p.rpp) + kv("Mh", p.Mh) +
           kv("margin", p.margin) + kv("ld", p.ld) + kv("head", (long long)p.head) + kv("copy", (long long)p.copy) + kv("ncopies", p.ncopies) + kv("Mp", p.Mp) + kv("ldA", N) +
           kv("ldB", C) + kv("wt_grp_rows", C);
}

void conv_tn_spans(const ConvPlan& p, int N, int C, Out& o) {   // conv3_dy_halo + conv3_wgrad_tn
    o.add(HALO, "dY image", 0, p.Kh * N);
    o.add(HALO, "zero rows", p.Kh * N, (p.Kp - p.Kh) * N);
    o.add(T2, "zero margin", 0, p.mrg * C);
    o.add(T2, "X image", p.mrg * C, p.Kh * C);
    o.add(T2, "zero tail", (p.mrg + p.Kh) * C, (p.Kp - p.Kh + p.mrg) * C);
    // tap (ky, kx) reads rows (ky - 1) rp + (kx - 1) .. + Kp of the image: the views, in elements from the start of S_T2
    for (int g = 0; g < 9; ++g) {
        const long long first = ((long long)p.mrg + (g / 3 - 1) * p.rp + (g % 3 - 1)) * C;
        o.views.push_back({first, first + (long long)p.Kp * C});
    }
}

void conv3(int B, int r, int N, int C, OpFmt mode, PlanReq q) {
    const ConvPlan p = plan_conv3(B, r, N, C, mode, q);
    Out o;
    o.es = op_size(p.fmt);
    const size_t M = (size_t)B * r * r, w = (size_t)9 * N * C;
    if (q.dX) {
        if (p.wgrad != WgradPath::TN) o.add(HALO, "dY image", 0, p.Kh * N);
        if (!q.staged_w) o.add(WT, "rotated filter", 0, w);
    }
    if (p.wgrad == WgradPath::TN) {
        conv_tn_spans(p, N, C, o);
        if (!q.defer) o.add(DW, "tap-major dW", 0, w, 4);
    } else if (p.wgrad == WgradPath::Im2colT) {
        o.add(T1, "dY^T", 0, (size_t)N * p.Mp);
        o.add(T2, "im2col^T", 0, (size_t)9 * C * p.Mp);
        o.add(DW, "tap-major dW", 0, w, 4);
        (void)M;
    } else if (p.wgrad != WgradPath::None) {
        const bool x3 = p.wgrad == WgradPath::X3Shift;
        o.add(T1, "dY^T", 0, (size_t)N * p.ld);
        for (int cp = 0; cp < p.ncopies; ++cp) {   // conv3_bwd's loop over the copies
            const size_t base = cp * p.copy;
            if (x3) {
                o.add(T2, "zero head", base, p.head);
                o.add(T2, "X^T copy", base + p.head, (size_t)C * p.ld);
                o.add(T2, "zero tail", base + p.head + (size_t)C * p.ld, p.head);
            } else {
                o.add(T2, "zero head", base, p.head + p.margin - cp);   // (the memset's last element is overwritten by copy 1's image)
                o.add(T2, "X^T copy", base + p.head + p.margin - cp, (size_t)C * p.ld);
            }
        }
        for (int g = 0; g < 9; ++g) {   // igemm.h: shift(g), then C rows of ld elements
            const int ky = g / 3, kx = g % 3;
            const long long odd = op_is16(p.fmt) ? (long long)p.copy - 1 : 0;
            const long long shift = x3 ? (long long)p.head + (ky - 1) * p.rpp + kx * (long long)p.copy
                                       : (long long)p.head + (ky - 1) * p.rp + (kx - 1) + (kx != 1 ? odd : 0);
            o.views.push_back({shift, shift + (long long)C * p.ld});
        }
        o.add(DW, "tap-major dW", 0, w, 4);
    }
    const long long in[4] = {B, r, N, C};
    emit_common("conv3", in, 4, mode, q, p.fmt, p.wgrad, p.need, o, conv_fields(p, N, C));
}

void conv_gen(int B, int Hi, int Ho, int N, int C, int stride, int pad, OpFmt mode, PlanReq q) {
    const ConvPlan p = plan_conv_gen(B, Hi, Ho, N, C, stride, pad, mode, q);
    Out o;
    o.es = op_size(p.fmt);
    const size_t Mo = (size_t)B * Ho * Ho, w = (size_t)9 * N * C;
    if (p.fmt != OpFmt::F32) {
        if (q.dX) { o.add(DW, "rotated filter f32", 0, w, 4); o.add(WT, "rotated filter", 0, w); }
        if (q.dW) conv_tn_spans(p, N, C, o);
        else o.add(HALO, "dY image", 0, p.Kh * N);
    } else {
        if (q.dX) {
            o.add(WT, "filter operand", 0, w);
            if (!p.col2im) o.add(HALO, "dY image", 0, p.Kh * N);
            else if (!q.dW) o.add(T2, "dcol", 0, Mo * 9 * C);   // (with dW: overwritten by the im2col^T afterwards)
        }
        if (q.dW) {
            o.add(T1, "dY^T", 0, (size_t)N * p.Mp);
            o.add(T2, "im2col^T", 0, (size_t)9 * C * p.Mp);
        }
    }
    const long long in[7] = {B, Hi, Ho, N, C, stride, pad};
    emit_common("conv_gen", in, 7, mode, q, p.fmt, p.wgrad, p.need, o, conv_fields(p, N, C) + kv("dcol", p.col2im && q.dX ? (long long)(Mo * 9 * C) : 0));
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: train_plan_main FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[256];
    while (fgets(line, sizeof line, f)) {
        long long v[7] = {0, 0, 0, 0, 0, 0, 0};
        char k = 0;
        const int n = sscanf(line, " %c %lld %lld %lld %lld %lld %lld %lld", &k, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6]);
        if (n < 1) continue;
        if ((k == 'L' && n != 4) || (k == 'C' && n != 5) || (k == 'G' && n != 8) || !strchr("LCG", k)) { fprintf(stderr, "bad line: %s", line); fclose(f); return 2; }
        for (int mode = 0; mode < 4; ++mode)
            for (int out = 1; out <= 3; ++out)
                for (int staged = 0; staged < 2; ++staged)
                    for (int defer = 0; defer < 2; ++defer) {
                        const PlanReq q{(out & 1) != 0, (out & 2) != 0, staged != 0, defer != 0};
                        const OpFmt m = static_cast<OpFmt>(mode);
                        if (k == 'L') linear(v[0], (int)v[1], (int)v[2], m, q);
                        else if (k == 'C') conv3((int)v[0], (int)v[1], (int)v[2], (int)v[3], m, q);
                        else conv_gen((int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], (int)v[6], m, q);
                    }
    }
    fclose(f);
    return 0;
}
