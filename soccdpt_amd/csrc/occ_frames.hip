#pragma clang fp contract(off)
// Per-frame semantic occupancy grids for gfx950: row b of the packed output is the grid of frame b ALONE -- bit for bit what the reference's
// points_to_occupancy_grid (model/SOccDPT.py:374-463) computes when that one frame is handed to it as a batch of one -- where the fused kernel of
// projection.hip ORs every frame of the batch into one union grid.
//
//   voxelise_frames     inv_up [B,Hc,Wc] (the clamped inverse depth soccdpt_project wrote) + seg [B,C,h,w] (network resolution) -> bits [B][nwords]
//   occ_expand_frames   bits [B][nwords] -> dense f32 [B][ncell], row b from row b
//
// Float contract: this translation unit is NOT in the Makefile's EXACT_SRCS, so the pragma on its first line switches implicit contraction off for
// everything below, the included headers' inline functions as well: a * b + c rounds twice, as in projection.hip (-ffp-contract=off there); the
// explicit fmaf calls of rot3 stay fused; divisions are IEEE.  Per camera pixel the float32 sequence of project_rows*_kernel is redone from
// d = 1 / inv_up on, in its order, so every voxel index is the one the fused kernel derived from the same pixel.
//
// Algorithmic HBM bytes: read B * Hc * Wc * 4 (inv_up; a third of re-reading `points`), the class maps B * C * h * w * 4 once (gathered, cache
// resident), write B * nwords * 4 (the clear) + the OR traffic of ~1e4 voxels per frame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.h"
#include "resample.h"

namespace soccdpt {

namespace {

// o = p R, the k-ordered fma chain of a K = 3 sgemm row (the same expression as projection.hip's rot3)
__device__ __forceinline__ void rot3(const float p[3], const float* R, float o[3]) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = fmaf(p[2], R[6 + j], fmaf(p[1], R[3 + j], p[0] * R[j]));
}

struct FrameParams {
    const float* inv_up;   // [B,Hc,Wc]
    const float* seg;      // [B,C,h,w]
    uint32_t* bits;        // [B][nwords]
    size_t nwords;
    int B, h, w, Hc, Wc;
    float fx, fy, cx, cy;
    float pc_scale[3], pc_shift[3];
    float rot[27];
    float occ_shape[3];
    int grid[3];
};

// One workgroup = R consecutive camera rows x 1024 pixels of one frame, one thread = 4 consecutive pixels of each of the R rows (VEC4: one 16-byte
// load per row; otherwise -- camera width not a multiple of 4 -- four guarded scalar loads).  Marking is de-duplicated like project_rowsR_kernel:
// neighbouring pixels mostly fall into the same 0.5 m voxel, so a pixel only touches the grid when its (voxel, class set) is covered neither by
// its left neighbour's nor by the pixel's above it in the group; by induction along left / up chains every skipped pixel's bits are set by an
// acting pixel (the first pixel of each row segment and of the group's first row always act).  The OR is idempotent and integer: deterministic.
template <int C, int R, bool VEC4>
__global__ __launch_bounds__(256) void voxelise_frames_kernel(FrameParams P, int nseg, int rot_bc_identity) {
    __shared__ int s_lk[R][4];
    __shared__ uint32_t s_lc[R][4];
    int bid = blockIdx.x;
    const int seg = bid % nseg;
    bid /= nseg;
    const int ngrp = (P.Hc + R - 1) / R;
    const int u0 = (bid % ngrp) * R;
    const int b = bid / ngrp;
    const float sy = (float)P.h / (float)P.Hc;
    const float sx = (float)P.w / (float)P.Wc;
    const size_t npix = (size_t)P.Hc * P.Wc;
    const int vlo = seg * 1024;
    const int vhi = (vlo + 1024 < P.Wc) ? vlo + 1024 : P.Wc;
    const int v0 = vlo + (int)threadIdx.x * 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float* inv_b = P.inv_up + (size_t)b * npix;
    const float* seg_b = P.seg + (size_t)b * C * P.h * P.w;
    uint32_t* bits_b = P.bits + (size_t)b * P.nwords;

    int csv[4];
    float xt[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int v = v0 + e;
        csv[e] = nearest_src(v < P.Wc ? v : P.Wc - 1, P.w, sx);
        xt[e] = (float)v - P.cx;
    }
    int vkey[R][4];       // first cell index of the pixel's voxel (its C class bits are adjacent), -1 = not in the grid
    uint32_t vcm[R][4];   // classes with non-zero probability
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int u = u0 + r;
#pragma unroll
        for (int e = 0; e < 4; ++e) { vkey[r][e] = -1; vcm[r][e] = 0; }
        if (u >= P.Hc || v0 >= vhi) continue;
        const float* row = inv_b + (size_t)u * P.Wc;
        float iv[4];
        if constexpr (VEC4) {
            const float4 q = *reinterpret_cast<const float4*>(row + v0);   // Wc % 4 == 0: aligned, and all four pixels are inside the row
            iv[0] = q.x; iv[1] = q.y; iv[2] = q.z; iv[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) iv[e] = (v0 + e < vhi) ? row[v0 + e] : 0.0f;
        }
        const int su = nearest_src(u, P.h, sy);
        const float yterm = (float)u - P.cy;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int v = v0 + e;
            if (!VEC4 && v >= vhi) continue;
            float d = 1.0f / iv[e];
            if (isinf(d) || isnan(d)) d = __builtin_inff();
            float p[3];
            p[0] = (xt[e] * d) / P.fx;
            p[1] = (yterm * d) / P.fy;
            p[2] = d;
            const size_t n = (size_t)u * P.Wc + v;
            if (n < 3) {  // the reference scales/shifts flat pixels 0,1,2 of each image
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = p[k] * P.pc_scale[n] + P.pc_shift[n];
            }
            float a[3], cq[3];
            rot3(p, P.rot, a);
            if (rot_bc_identity) {   // fma(z, 0, fma(y, 0, x * 1)) == x for finite points; a non-finite one is left out either way (projection.hip)
                cq[0] = a[0]; cq[1] = a[1]; cq[2] = a[2];
            } else {
                float bq[3];
                rot3(a, P.rot + 9, bq);
                rot3(bq, P.rot + 18, cq);
            }
            const bool fin = isfinite(cq[0]) && isfinite(cq[1]) && isfinite(cq[2]);
            const float fi = (cq[0] / P.occ_shape[0]) * (float)P.grid[0];
            const float fj = (cq[1] / P.occ_shape[1]) * (float)P.grid[1];
            const float fk = (cq[2] / P.occ_shape[2]) * (float)P.grid[2];
            // trunc-toward-zero as the reference's .type(int64); window test in float first so the integer conversion is always in range
            const bool inr = fin && fi > -1.0f && fi < 65536.0f && fj > -1.0f && fj < 65536.0f && fk > -1.0f && fk < 65536.0f;
            if (inr) {
                const int i = (int)fi, j = (int)fj, k = (int)fk;
                if (0 < i && i < P.grid[0] && 0 < j && j < P.grid[1] && 0 < k && k < P.grid[2]) {
                    uint32_t cm = 0;   // the class maps are only read for pixels that land in the grid
#pragma unroll
                    for (int c = 0; c < C; ++c) cm |= (seg_b[((size_t)c * P.h + su) * P.w + csv[e]] != 0.0f) ? (1u << c) : 0u;
                    if (cm) {
                        vkey[r][e] = ((i * P.grid[1] + j) * P.grid[2] + k) * C;
                        vcm[r][e] = cm;
                    }
                }
            }
        }
    }
    // ---- marking with run-length de-duplication along each camera row and down the group's rows ----
    if (lane == 63) {
#pragma unroll
        for (int r = 0; r < R; ++r) { s_lk[r][wave] = vkey[r][3]; s_lc[r][wave] = vcm[r][3]; }
    }
    __syncthreads();
    uint32_t cur_lo[R][4], cur_hi[R][4];
    bool act[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        int pk = __shfl_up(vkey[r][3], 1);
        uint32_t pc = __shfl_up(vcm[r][3], 1);
        if (lane == 0) {
            if (wave == 0) { pk = -2; pc = 0; }
            else { pk = s_lk[r][wave - 1]; pc = s_lc[r][wave - 1]; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            act[r][e] = vkey[r][e] >= 0 && (vkey[r][e] != pk || (vcm[r][e] & ~pc));
            if (r > 0 && vkey[r][e] == vkey[r - 1][e] && !(vcm[r][e] & ~vcm[r - 1][e])) act[r][e] = false;
            cur_lo[r][e] = ~0u; cur_hi[r][e] = ~0u;
            if (act[r][e]) {   // all R x 4 check loads go out before the first result is needed
                const uint32_t bit = (uint32_t)vkey[r][e];
                const uint32_t* wp = bits_b + (bit >> 5);
                // idempotent OR: a stale read only costs a redundant atomic, so the check may be served by the nearest cache
                cur_lo[r][e] = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if ((bit & 31) + C > 32) cur_hi[r][e] = __hip_atomic_load(wp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            pk = vkey[r][e];
            pc = vcm[r][e];
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (act[r][e]) {
                const uint32_t bit = (uint32_t)vkey[r][e];
                const unsigned long long m = (unsigned long long)vcm[r][e] << (bit & 31);
                const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
                uint32_t* wp = bits_b + (bit >> 5);
                if ((cur_lo[r][e] & mlo) != mlo) atomicOr(wp, mlo);
                if (mhi && (cur_hi[r][e] & mhi) != mhi) atomicOr(wp + 1, mhi);
            }
        }
}

// bits [B][nwords] -> f32 [B][ncell].  ncell % 32 == 0, so the rows' words are contiguous in bit order and the batch is one flat array: one thread =
// 4 consecutive cells, written once and streamed past the caches (the same bytes per row as occ_expand_kernel stores).
__global__ __launch_bounds__(256) void occ_expand_frames_kernel(const uint32_t* __restrict__ bits, float* __restrict__ occ, size_t nq) {
    typedef __attribute__((ext_vector_type(4))) float v4f;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        const size_t n = q * 4;
        const uint32_t wv = bits[n >> 5] >> (n & 31);
        __builtin_nontemporal_store(v4f{(float)(wv & 1u), (float)((wv >> 1) & 1u), (float)((wv >> 2) & 1u), (float)((wv >> 3) & 1u)},
                                    reinterpret_cast<v4f*>(occ + n));
    }
}

}  // namespace

int launch_voxelise_frames(const soccdpt_config& cfg, const float* inv_up, const float* seg, int B, int in_h, int in_w, uint32_t* frame_bits,
                           int clear_bits, hipStream_t stream, std::string& err) {
    if (cfg.num_classes != 3) {
        err = "voxelise_frames kernel is instantiated for num_classes == 3 (the reference reshapes xyz with num_classes)";
        return 1;
    }
    if (B <= 0 || in_h <= 0 || in_w <= 0) {
        err = "soccdpt_voxelise_frames: empty input";
        return 1;
    }
    const size_t ncell = (size_t)cfg.grid[0] * cfg.grid[1] * cfg.grid[2] * cfg.num_classes;
    if (ncell >= (1ull << 31) || cfg.grid[0] > 65535 || cfg.grid[1] > 65535 || cfg.grid[2] > 65535) {
        err = "occupancy grid too large for 32-bit cell indices";
        return 1;
    }
    FrameParams P;
    P.inv_up = inv_up; P.seg = seg; P.bits = frame_bits;
    P.nwords = (ncell + 31) / 32;
    P.B = B; P.h = in_h; P.w = in_w; P.Hc = cfg.cam_height; P.Wc = cfg.cam_width;
    P.fx = cfg.fx; P.fy = cfg.fy; P.cx = cfg.cx; P.cy = cfg.cy;
    for (int i = 0; i < 3; ++i) {
        P.pc_scale[i] = cfg.pc_scale[i];
        P.pc_shift[i] = cfg.pc_shift[i];
        P.occ_shape[i] = cfg.occupancy_shape[i];
        P.grid[i] = cfg.grid[i];
    }
    for (int i = 0; i < 27; ++i) P.rot[i] = cfg.rot[i];
    if (clear_bits) {
        hipError_t e = hipMemsetAsync(frame_bits, 0, (size_t)B * P.nwords * sizeof(uint32_t), stream);
        if (e != hipSuccess) { err = hipGetErrorString(e); return 1; }
    }
    bool ident = true;   // Rb and Rc exactly the identity? (rotate_points with b = c = 0)
    for (int i = 0; i < 9; ++i) ident = ident && P.rot[9 + i] == ((i % 4 == 0) ? 1.0f : 0.0f) && P.rot[18 + i] == ((i % 4 == 0) ? 1.0f : 0.0f);
    constexpr int R = 4;
    const int nseg = (P.Wc + 1023) / 1024;
    const int ngrp = (P.Hc + R - 1) / R;
    const long long blocks = (long long)B * ngrp * nseg;
    if (blocks > 0x7fffffffLL) { err = "soccdpt_voxelise_frames: batch too large for one launch"; return 1; }
    if (P.Wc % 4 == 0)
        SOCCDPT_LAUNCH((voxelise_frames_kernel<3, R, true>), dim3((unsigned)blocks), dim3(256), 0, stream, P, nseg, ident ? 1 : 0);
    else
        SOCCDPT_LAUNCH((voxelise_frames_kernel<3, R, false>), dim3((unsigned)blocks), dim3(256), 0, stream, P, nseg, ident ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = hipGetErrorString(e); return 1; }
    return 0;
}

int launch_occ_expand_frames(const soccdpt_config& cfg, const uint32_t* frame_bits, int B, float* occ, hipStream_t stream, std::string& err) {
    const size_t ncell = (size_t)cfg.grid[0] * cfg.grid[1] * cfg.grid[2] * cfg.num_classes;
    if (ncell % 32 != 0) { err = "occupancy cell count must be a multiple of 32"; return 1; }
    const size_t nq = ncell / 4 * (size_t)B;
    size_t blocks = (nq + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride beyond 16 blocks per CU
    SOCCDPT_LAUNCH(occ_expand_frames_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, frame_bits, occ, nq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { err = hipGetErrorString(e); return 1; }
    return 0;
}

}  // namespace soccdpt
