// Device code of the Swin-V1 block (dpt_swin_large_384: timm swin_large_patch4_window12_384), where it differs from Swin-V2's:
//
//  * scaled dot-product window attention: S = (q 32^-0.5) k^T + table[relative position index] [+ shift mask], O = softmax(S) V.  The 12 x 12
//    online-softmax kernels of attention.hip without the cosine normalisation at staging: the 16-bit form stages q scaled, k and v as they are, and
//    runs attention_body.h's window_attention_flash_core on them (same LDS layout, same bias tile as the initial accumulator, same x3 store); the f32
//    form is window_attention_f32_flash_kernel's loop with the plain k tile.  A second body in a translation unit of its own: nothing attention.hip
//    instantiates is touched.
//  * pre-norm LayerNorm rows: operand = LN(xf) g + beta, xf read only (Swin-V2 normalises the branch and writes the stream: ln_residual).
//  * merge-LN: PatchMerging of Swin-V1 normalises the gathered 4C row BEFORE the reduction; one kernel gathers the 2 x 2 neighbourhood in timm's
//    order (0::2, 0::2), (1::2, 0::2), (0::2, 1::2), (1::2, 1::2) from the f32 stream and writes the normalised operand row.
//
// Both LayerNorm kernels: one wave per row, float4 loads, the whole row in registers, ln_body.h's wave_sum.  Compiler's report (gfx950): ln_prenorm_kernel
// <1 / 2 / 3 / 6> 23 / 27 / 31 / 50 VGPRs, merge_ln_kernel<192 / 384 / 768> 34 / 50 / 76 VGPRs; the attention kernels 108 (fp16) / 104 (bf16) / 104 (f32).  No scratch in any of them.
// Operand format codes as in kernels.h: 0 bf16, 1 fp16, 2 f32, 3 x3.
#include "../../include/soccdpt_swin1.h"

#include "attention_body.h"
#include "ln_body.h"

namespace soccdpt {

void set_last_error(const std::string& msg);   // what soccdpt_last_error(NULL) returns (capi.cpp)

namespace {

constexpr int SDP_WKS = 36;   // floats per K row in LDS, as attention.hip's WKS

template <int WS, bool F16>
__global__ __launch_bounds__(AttnGenCfg<WS>::THREADS) void window_attention_sdp_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias_acc,
                                                                                        float qscale, bf16_t* __restrict__ out, int res, int shift, int heads,
                                                                                        int out_x3) {
    using A = AttnGenCfg<WS>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;
    char* Ks = smem + A::KS_OFF;
    char* Vt = smem + A::VT_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = heads * 32;
    const int nw = res / WS;
    int bid = blockIdx.x;
    const int head = bid % heads;
    bid /= heads;
    const int wx = bid % nw;
    bid /= nw;
    const int wy = bid % nw;
    const int b = bid / nw;
    auto token_row = [&](int p) -> size_t {
        const int r = p / WS, c = p % WS;
        int sy = wy * WS + r + shift, sx = wx * WS + c + shift;
        sy = sy >= res ? sy - res : sy;
        sx = sx >= res ? sx - res : sx;
        return (size_t)(b * res + sy) * res + sx;
    };
    // staging: 4 lanes per token, 16-byte loads; q is scaled (one more 16-bit rounding of q), k and v keep their bits; padded tokens are zero rows
    for (int idx = tid; idx < A::NPAD * 4; idx += A::THREADS) {
        const int p = idx >> 2, c = idx & 3;
        uint4 qv = make_uint4(0, 0, 0, 0), kv = qv, vv = qv;
        if (p < A::N) {
            const bf16_t* src = qkv + token_row(p) * (size_t)(3 * C) + head * 32 + c * 8;
            qv = *reinterpret_cast<const uint4*>(src);
            kv = *reinterpret_cast<const uint4*>(src + C);
            vv = *reinterpret_cast<const uint4*>(src + 2 * C);
        }
        const uint32_t qu[4] = {qv.x, qv.y, qv.z, qv.w}, vu[4] = {vv.x, vv.y, vv.z, vv.w};
        uint4 qo;
        qo.x = pack_h2<F16>(h_lo<F16>(qu[0]) * qscale, h_hi<F16>(qu[0]) * qscale);
        qo.y = pack_h2<F16>(h_lo<F16>(qu[1]) * qscale, h_hi<F16>(qu[1]) * qscale);
        qo.z = pack_h2<F16>(h_lo<F16>(qu[2]) * qscale, h_hi<F16>(qu[2]) * qscale);
        qo.w = pack_h2<F16>(h_lo<F16>(qu[3]) * qscale, h_hi<F16>(qu[3]) * qscale);
        const int sw = (c ^ ((p >> 2) & 3)) * 16;
        *reinterpret_cast<uint4*>(Qs + p * 64 + sw) = qo;
        *reinterpret_cast<uint4*>(Ks + p * 64 + sw) = kv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<uint16_t*>(Vt + (c * 8 + 2 * j) * A::VT_STRIDE + p * 2) = (uint16_t)(vu[j] & 0xffffu);
            *reinterpret_cast<uint16_t*>(Vt + (c * 8 + 2 * j + 1) * A::VT_STRIDE + p * 2) = (uint16_t)(vu[j] >> 16);
        }
    }
    __syncthreads();
    window_attention_flash_core<WS, F16>(Qs, Ks, Vt, bias_acc, out, res, shift, heads, out_x3, head, b, wy, wx, 0, A::NT, wave, lane, A::THREADS / 64);
}

// The exact-f32 form: window_attention_f32_flash_kernel (attention.hip) with q scaled by qscale and k as stored.  One workgroup = 4 waves = 4 blocks of 32
// queries of one (sample, window, head); key / value tiles of 32 tokens stream through a double-buffered LDS ring, one barrier per tile.
template <int WS>
__global__ __launch_bounds__(256) void window_attention_sdp_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ bias_acc, float qscale,
                                                                       float* __restrict__ out, int res, int shift, int heads, int x3) {
    constexpr int N = WS * WS, NT = (N + 31) / 32, NQB = (NT + 3) / 4, HALF = WS / 2;
    __shared__ __attribute__((aligned(16))) float Ks[2][32 * SDP_WKS];
    __shared__ __attribute__((aligned(16))) float Vs[2][32 * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = heads * 32;
    const int nw = res / WS;
    int bid = blockIdx.x;
    const int part = bid % NQB;
    bid /= NQB;
    const int head = bid % heads;
    bid /= heads;
    const int wx = bid % nw;
    bid /= nw;
    const int wy = bid % nw;
    const int b = bid / nw;
    auto token_row = [&](int p) -> size_t {
        const int r = p / WS, c = p % WS;
        int sy = wy * WS + r + shift, sx = wx * WS + c + shift;
        sy = sy >= res ? sy - res : sy;
        sx = sx >= res ? sx - res : sx;
        return (size_t)(b * res + sy) * res + sx;
    };
    const int r32 = lane & 31, h = lane >> 5;
    const int qb = part * 4 + wave;
    const bool active = qb < NT;             // wave-uniform
    const int qrow = qb * 32 + r32;
    const int qcl = qrow < N ? qrow : N - 1;
    const bool qr_hi = (qcl / WS) >= HALF, qc_hi = (qcl % WS) >= HALF;
    const bool lastrow = (shift > 0) && (wy == nw - 1), lastcol = (shift > 0) && (wx == nw - 1);

    // staging: thread -> (token of the tile = tid >> 3, 16-byte chunk c = tid & 7)
    float4 kr, vr;
    auto gload = [&](int t) {
        const int p = t * 32 + (tid >> 3), c = tid & 7;
        kr = make_float4(0.f, 0.f, 0.f, 0.f);
        vr = kr;
        if (p < N) {
            const float* src = qkv + token_row(p) * (size_t)(3 * C) + head * 32 + c * 4;
            kr = *reinterpret_cast<const float4*>(src + C);
            vr = *reinterpret_cast<const float4*>(src + 2 * C);
        }
    };
    auto lstore = [&](int buf) {
        const int kt = tid >> 3, c = tid & 7;
        *reinterpret_cast<float4*>(&Ks[buf][kt * SDP_WKS + c * 4]) = kr;
        *reinterpret_cast<float4*>(&Vs[buf][kt * 32 + c * 4]) = vr;
    };
    // scaled q fragment (B operand): lane (query r32, half h), step st <-> d = 16 h + st
    float qf[16];
    {
        const float* src = qkv + token_row(qcl) * (size_t)(3 * C) + head * 32 + 16 * h;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float4 q4 = *reinterpret_cast<const float4*>(src + 4 * j);
            qf[4 * j] = q4.x * qscale; qf[4 * j + 1] = q4.y * qscale; qf[4 * j + 2] = q4.z * qscale; qf[4 * j + 3] = q4.w * qscale;
        }
    }
    gload(0);
    lstore(0);
    __syncthreads();
    constexpr float LOG2E = 1.4426950408889634f;
    float m = -3.0e38f, l = 0.f;
    f32x16 o;
#pragma unroll
    for (int rg = 0; rg < 16; ++rg) o[rg] = 0.f;
    const float* bp = bias_acc + ((size_t)(head * NT + (active ? qb : 0)) * NT) * 1024 + lane * 16;
    float4 nb0, nb1, nb2, nb3;
    {
        const float4* b4 = reinterpret_cast<const float4*>(bp);
        nb0 = b4[0]; nb1 = b4[1]; nb2 = b4[2]; nb3 = b4[3];
    }
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
        const int buf = t & 1;
        if (t + 1 < NT) gload(t + 1);
        if (active) {
            const float4 b0 = nb0, b1 = nb1, b2 = nb2, b3 = nb3;
            if (t + 1 < NT) {
                const float4* b4 = reinterpret_cast<const float4*>(bp + (size_t)(t + 1) * 1024);
                nb0 = b4[0]; nb1 = b4[1]; nb2 = b4[2]; nb3 = b4[3];
            }
            f32x16 acc = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w, b2.x, b2.y, b2.z, b2.w, b3.x, b3.y, b3.z, b3.w};
            if (lastrow || lastcol) {
#pragma unroll
                for (int rg = 0; rg < 16; ++rg) {
                    int key = t * 32 + (rg & 3) + 8 * (rg >> 2) + 4 * h;
                    key = key < N ? key : N - 1;
                    const bool kr_hi = (key / WS) >= HALF, kc_hi = (key % WS) >= HALF;
                    if ((lastrow && (kr_hi != qr_hi)) || (lastcol && (kc_hi != qc_hi))) acc[rg] += -100.0f;
                }
            }
            const float* krow = &Ks[buf][r32 * SDP_WKS + 16 * h];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 k4 = *reinterpret_cast<const float4*>(krow + 4 * j);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qf[4 * j], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qf[4 * j + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qf[4 * j + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qf[4 * j + 3], acc, 0, 0, 0);
            }
            float mt = acc[0];
#pragma unroll
            for (int rg = 1; rg < 16; ++rg) mt = fmaxf(mt, acc[rg]);
            mt = fmaxf(mt, __shfl_xor(mt, 32));
            const float mn = fmaxf(m, mt);
            const float mnl = mn * LOG2E;
            const float alpha = __builtin_amdgcn_exp2f(fmaf(m, LOG2E, -mnl));
            float psum = 0.f;
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) {
                acc[rg] = __builtin_amdgcn_exp2f(fmaf(acc[rg], LOG2E, -mnl));
                psum += acc[rg];
                o[rg] *= alpha;
            }
            l = l * alpha + psum;
            m = mn;
            const float* vcol = &Vs[buf][(4 * h) * 32 + r32];
#pragma unroll
            for (int rg = 0; rg < 16; ++rg) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vcol[((rg & 3) + 8 * (rg >> 2)) * 32], acc[rg], o, 0, 0, 0);
        }
        if (t + 1 < NT) lstore(buf ^ 1);
        __syncthreads();
    }
    if (!active) return;
    l += __shfl_xor(l, 32);
    if (qrow < N) {
        const float inv = 1.0f / l;
        const size_t e0 = token_row(qrow) * (size_t)C + head * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (x3) x3_store4(out, e0 + 8 * g + 4 * h, o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
            else *reinterpret_cast<float4*>(out + e0 + 8 * g + 4 * h) = make_float4(o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
        }
    }
}

// 4 consecutive elements e .. e + 3 of an operand tensor in format fmt (wave-uniform)
__device__ __forceinline__ void store_op4(void* out, int fmt, size_t e, float4 o) {
    if (fmt == 2) *reinterpret_cast<float4*>(static_cast<float*>(out) + e) = o;
    else if (fmt == 3) x3_store4(out, e, o.x, o.y, o.z, o.w);
    else {
        uint2 ob;
        if (fmt == 1) { ob.x = pack_h2<true>(o.x, o.y); ob.y = pack_h2<true>(o.z, o.w); }
        else { ob.x = pack_h2<false>(o.x, o.y); ob.y = pack_h2<false>(o.z, o.w); }
        *reinterpret_cast<uint2*>(static_cast<bf16_t*>(out) + e) = ob;
    }
}

// mean and 1 / sqrt(var + eps) of a row of K values held as V4 float4 groups per lane (absent groups are zero and `valid` false); v becomes v - mean
template <int V4>
__device__ __forceinline__ float center_and_rstd(float4 (&v)[V4], const bool (&valid)[V4], int K, float eps) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < V4; ++t) s += (v[t].x + v[t].y) + (v[t].z + v[t].w);
    const float mean = wave_sum(s) / (float)K;
    float q = 0.f;
#pragma unroll
    for (int t = 0; t < V4; ++t) {
        if (valid[t]) { v[t].x -= mean; v[t].y -= mean; v[t].z -= mean; v[t].w -= mean; }
        q += (v[t].x * v[t].x + v[t].y * v[t].y) + (v[t].z * v[t].z + v[t].w * v[t].w);
    }
    return rsqrtf(wave_sum(q) / (float)K + eps);
}

__device__ __forceinline__ float4 affine4(float4 d, float rstd, float4 g, float4 b) {
    return make_float4(d.x * rstd * g.x + b.x, d.y * rstd * g.y + b.y, d.z * rstd * g.z + b.z, d.w * rstd * g.w + b.w);
}

template <int V4>   // float4 groups per lane = ceil(C / 256)
__global__ __launch_bounds__(256) void ln_prenorm_kernel(const float* __restrict__ xf, const float* __restrict__ g, const float* __restrict__ beta,
                                                         void* __restrict__ out, int fmt, int rows, int C, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;   // wave-uniform
    const int n4 = C >> 2;
    const float4* xr = reinterpret_cast<const float4*>(xf + (size_t)row * C);
    float4 v[V4];
    bool valid[V4];
#pragma unroll
    for (int t = 0; t < V4; ++t) {
        const int c4 = lane + 64 * t;
        valid[t] = c4 < n4;
        v[t] = valid[t] ? xr[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float rstd = center_and_rstd<V4>(v, valid, C, eps);
#pragma unroll
    for (int t = 0; t < V4; ++t) {
        const int c4 = lane + 64 * t;
        if (!valid[t]) continue;
        const float4 o = affine4(v[t], rstd, reinterpret_cast<const float4*>(g)[c4], reinterpret_cast<const float4*>(beta)[c4]);
        store_op4(out, fmt, (size_t)row * C + 4 * c4, o);
    }
}

template <int C>   // source width; the normalised row is 4C = 64 lanes x (C / 64) float4 groups
__global__ __launch_bounds__(256) void merge_ln_kernel(const float* __restrict__ xf, const float* __restrict__ g, const float* __restrict__ beta,
                                                       void* __restrict__ out, int fmt, int rows, int R, float eps) {
    constexpr int V4 = C / 64, N4 = C / 4;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;   // wave-uniform
    const int Ro = R >> 1;
    const int b = row / (Ro * Ro), r = row - b * (Ro * Ro), oy = r / Ro, ox = r - oy * Ro;
    float4 v[V4];
    bool valid[V4];
#pragma unroll
    for (int t = 0; t < V4; ++t) {
        const int c4 = lane + 64 * t;
        const int k = c4 / N4, o4 = c4 - k * N4;   // channel block k of the 4C row = source pixel (2 oy + (k & 1), 2 ox + (k >> 1))
        const float* src = xf + (((size_t)b * R + 2 * oy + (k & 1)) * R + 2 * ox + (k >> 1)) * C;
        valid[t] = true;
        v[t] = reinterpret_cast<const float4*>(src)[o4];
    }
    const float rstd = center_and_rstd<V4>(v, valid, 4 * C, eps);
#pragma unroll
    for (int t = 0; t < V4; ++t) {
        const int c4 = lane + 64 * t;
        const float4 o = affine4(v[t], rstd, reinterpret_cast<const float4*>(g)[c4], reinterpret_cast<const float4*>(beta)[c4]);
        store_op4(out, fmt, (size_t)row * (4 * C) + 4 * c4, o);
    }
}

int failed(const std::string& err) {
    set_last_error("soccdpt_swin1_" + err);
    return 1;
}

}  // namespace

static int sdp_geometry(const char* who, int B, int res, int ws, int shift, int heads, std::string& err) {
    if (window_attention_geometry(who, B, res, ws, shift, heads, err)) return 1;
    if (ws != 12) { err = std::string(who) + ": window size not instantiated (12 is)"; return 1; }
    if ((long long)B * (res / ws) * (res / ws) * heads * 2 > 0x7fffffffLL) { err = std::string(who) + ": too many (window, head) pairs for one launch"; return 1; }
    return 0;
}

int launch_window_attention_sdp(const bf16_t* qkv, const float* bias_acc, bf16_t* out, int hf, int B, int res, int ws, int shift, int heads, hipStream_t st,
                                std::string& err, int out_x3) {
    if (!qkv || !bias_acc || !out) { err = "window_attention_sdp: null argument"; return 1; }
    if (sdp_geometry("window_attention_sdp", B, res, ws, shift, heads, err)) return 1;
    if (out_x3 && !hf) { err = "window_attention_sdp: the x3 output form belongs to the fp16 kernel"; return 1; }
    if (!ptr_aligned16(qkv) || !ptr_aligned16(bias_acc) || !ptr_aligned16(out)) { err = "window_attention_sdp: tensors must be 16-byte aligned"; return 1; }
    const int nw = res / ws;
    const unsigned blocks = (unsigned)(B * nw * nw * heads);
    const float qscale = 0.17677669529663687f;   // 32^-0.5: the head dimension is 32 at every stage
    using A = AttnGenCfg<12>;
    if (hf) SOCCDPT_LAUNCH((window_attention_sdp_kernel<12, true>), dim3(blocks), dim3(A::THREADS), A::LDS, st, qkv, bias_acc, qscale, out, res, shift, heads, out_x3);
    else SOCCDPT_LAUNCH((window_attention_sdp_kernel<12, false>), dim3(blocks), dim3(A::THREADS), A::LDS, st, qkv, bias_acc, qscale, out, res, shift, heads, out_x3);
    return check_launch("window_attention_sdp", err);
}

int launch_window_attention_sdp_f32(const float* qkv, const float* bias_acc, float* out, int B, int res, int ws, int shift, int heads, hipStream_t st,
                                    std::string& err, int x3) {
    if (!qkv || !bias_acc || !out) { err = "window_attention_sdp_f32: null argument"; return 1; }
    if (sdp_geometry("window_attention_sdp_f32", B, res, ws, shift, heads, err)) return 1;
    if (!ptr_aligned16(qkv) || !ptr_aligned16(bias_acc) || !ptr_aligned16(out)) { err = "window_attention_sdp_f32: tensors must be 16-byte aligned"; return 1; }
    const int nw = res / ws;
    constexpr int NT = (12 * 12 + 31) / 32, NQB = (NT + 3) / 4;
    const unsigned blocks = (unsigned)(B * nw * nw * heads * NQB);
    const float qscale = 0.17677669529663687f;
    SOCCDPT_LAUNCH((window_attention_sdp_f32_kernel<12>), dim3(blocks), dim3(256), 0, st, qkv, bias_acc, qscale, out, res, shift, heads, x3);
    return check_launch("window_attention_sdp_f32", err);
}

bool ln_prenorm_supported(int C) { return C == 192 || C == 384 || C == 768 || C == 1536; }

int launch_ln_prenorm(const float* xf, const float* g, const float* beta, void* out, int fmt, int rows, int C, float eps, hipStream_t st, std::string& err) {
    if (!xf || !g || !beta || !out) { err = "ln_prenorm: null argument"; return 1; }
    if (fmt < 0 || fmt > 3) { err = "ln_prenorm: unknown operand format"; return 1; }
    if (rows <= 0 || rows > 0x7ffffff0 / 4) { err = "ln_prenorm: rows must be positive"; return 1; }
    if (!ln_prenorm_supported(C)) { err = "ln_prenorm: C not instantiated (192, 384, 768, 1536 are)"; return 1; }
    if (!(eps > 0.f)) { err = "ln_prenorm: eps must be positive"; return 1; }
    if (!ptr_aligned16(xf) || !ptr_aligned16(g) || !ptr_aligned16(beta) || !ptr_aligned16(out)) { err = "ln_prenorm: tensors must be 16-byte aligned"; return 1; }
    if (static_cast<const void*>(xf) == out) { err = "ln_prenorm: the operand must not alias xf (the stream is read only)"; return 1; }
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (C) {
        case 192: SOCCDPT_LAUNCH((ln_prenorm_kernel<1>), grid, block, 0, st, xf, g, beta, out, fmt, rows, C, eps); break;
        case 384: SOCCDPT_LAUNCH((ln_prenorm_kernel<2>), grid, block, 0, st, xf, g, beta, out, fmt, rows, C, eps); break;
        case 768: SOCCDPT_LAUNCH((ln_prenorm_kernel<3>), grid, block, 0, st, xf, g, beta, out, fmt, rows, C, eps); break;
        default: SOCCDPT_LAUNCH((ln_prenorm_kernel<6>), grid, block, 0, st, xf, g, beta, out, fmt, rows, C, eps); break;
    }
    return check_launch("ln_prenorm", err);
}

int launch_merge_ln(const float* xf, const float* g, const float* beta, void* out, int fmt, int B, int R, int C, float eps, hipStream_t st, std::string& err) {
    if (!xf || !g || !beta || !out) { err = "merge_ln: null argument"; return 1; }
    if (fmt < 0 || fmt > 3) { err = "merge_ln: unknown operand format"; return 1; }
    if (B <= 0 || R <= 0) { err = "merge_ln: B and R must be positive"; return 1; }
    if (R % 2 != 0) { err = "merge_ln: R must be even"; return 1; }
    if (C != 192 && C != 384 && C != 768) { err = "merge_ln: C not instantiated (192, 384, 768 are)"; return 1; }
    if (!(eps > 0.f)) { err = "merge_ln: eps must be positive"; return 1; }
    if ((long long)B * (R / 2) * (R / 2) > 0x7ffffff0LL / 4) { err = "merge_ln: too many rows for one launch"; return 1; }
    if (!ptr_aligned16(xf) || !ptr_aligned16(g) || !ptr_aligned16(beta) || !ptr_aligned16(out)) { err = "merge_ln: tensors must be 16-byte aligned"; return 1; }
    if (static_cast<const void*>(xf) == out) { err = "merge_ln: the operand must not alias xf"; return 1; }
    const int rows = B * (R / 2) * (R / 2);
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    switch (C) {
        case 192: SOCCDPT_LAUNCH((merge_ln_kernel<192>), grid, block, 0, st, xf, g, beta, out, fmt, rows, R, eps); break;
        case 384: SOCCDPT_LAUNCH((merge_ln_kernel<384>), grid, block, 0, st, xf, g, beta, out, fmt, rows, R, eps); break;
        default: SOCCDPT_LAUNCH((merge_ln_kernel<768>), grid, block, 0, st, xf, g, beta, out, fmt, rows, R, eps); break;
    }
    return check_launch("merge_ln", err);
}

// SOCCDPT_PREC_* of the public header -> operand format code; -1 = none
static int fmt_of_precision(int precision) {
    switch (precision) {
        case SOCCDPT_PREC_BF16: return 0;
        case SOCCDPT_PREC_F16: return 1;
        case SOCCDPT_PREC_F32: return 2;
        case SOCCDPT_PREC_F16X3: return 3;
        default: return -1;
    }
}

}  // namespace soccdpt

extern "C" {

int soccdpt_swin1_window_attention(const void* dev_qkv, const float* dev_table, void* dev_out, float* dev_bias_scratch, int B, int res, int ws, int shift,
                                   int heads, int precision, int out_x3, void* stream) {
    using namespace soccdpt;
    std::string err;
    if (fmt_of_precision(precision) < 0) return failed("window_attention: unknown precision");
    if (!dev_qkv || !dev_table || !dev_out || !dev_bias_scratch) return failed("window_attention: null argument");
    if (sdp_geometry("window_attention", B, res, ws, shift, heads, err)) return failed(err);   // before the bias launch: nothing runs on a refusal
    if (out_x3 && precision != SOCCDPT_PREC_F16) return failed("window_attention: the x3 output form belongs to the fp16 kernel");
    if (!ptr_aligned16(dev_qkv) || !ptr_aligned16(dev_bias_scratch) || !ptr_aligned16(dev_out)) return failed("window_attention: tensors must be 16-byte aligned");
    if (launch_attn_bias(dev_table, dev_bias_scratch, ws, heads, (hipStream_t)stream, err)) return failed("window_attention: " + err);
    int rc;
    if (precision == SOCCDPT_PREC_F32 || precision == SOCCDPT_PREC_F16X3)   // F16X3: f32 qkv in, x3 operand out
        rc = launch_window_attention_sdp_f32(static_cast<const float*>(dev_qkv), dev_bias_scratch, static_cast<float*>(dev_out), B, res, ws, shift, heads,
                                             (hipStream_t)stream, err, precision == SOCCDPT_PREC_F16X3 ? 1 : 0);
    else
        rc = launch_window_attention_sdp(static_cast<const bf16_t*>(dev_qkv), dev_bias_scratch, static_cast<bf16_t*>(dev_out), precision == SOCCDPT_PREC_F16 ? 1 : 0,
                                         B, res, ws, shift, heads, (hipStream_t)stream, err, out_x3 ? 1 : 0);
    return rc ? failed(err) : 0;
}

int soccdpt_swin1_ln_rows(const float* dev_xf, const float* dev_g, const float* dev_beta, void* dev_out, int out_format, int rows, int C, float eps, void* stream) {
    using namespace soccdpt;
    std::string err;
    const int fmt = fmt_of_precision(out_format);
    if (fmt < 0) return failed("ln_rows: unknown operand format");
    return launch_ln_prenorm(dev_xf, dev_g, dev_beta, dev_out, fmt, rows, C, eps, (hipStream_t)stream, err) ? failed(err) : 0;
}

int soccdpt_swin1_merge_ln(const float* dev_xf, const float* dev_g, const float* dev_beta, void* dev_out, int out_format, int B, int R, int C, float eps,
                           void* stream) {
    using namespace soccdpt;
    std::string err;
    const int fmt = fmt_of_precision(out_format);
    if (fmt < 0) return failed("merge_ln: unknown operand format");
    return launch_merge_ln(dev_xf, dev_g, dev_beta, dev_out, fmt, B, R, C, eps, (hipStream_t)stream, err) ? failed(err) : 0;
}

}  // extern "C"
