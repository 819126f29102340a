// Observed space of a camera frame in the occupancy grid (include/soccdpt_occ_rays.h): what tells a voxel the camera saw from one nobody saw.
//   rays          one ray per cast pixel from z_near to the measured depth, walked voxel by voxel (occ_rays_core.h), every voxel entered set in a
//                 per-voxel bit mask [rows][nvw]: voxel m = (i0 g1 + i1) g2 + i2 is bit m & 31 of word m >> 5
//   iou_masked    per-class (intersection, union, pred, gt) counts of two packed cell grids over the voxels of such a mask
// The ray walk carries a bit-exact float64 contract with a numpy restatement (tests/occ_rays_refs.py); occ_rays_core.h turns contraction off for
// this file, and the pragma below says so again for whatever is added here.
#pragma clang fp contract(off)
#include "occ_rays.h"

#include "kernels.h"
#include "launch.h"
#include "occ_rays_core.h"

namespace soccdpt {

namespace {

// One lane per ray; a wave is an 8 x 8 tile of cast pixels, so that its rays run through the same columns of the grid near the camera.  A lane keeps
// the word it is in and the bits it set there in two registers and hands them over when the walk moves to another word (with g2 = 32: once per
// (i0, i1) column).  The hand-over is the idempotent OR of projection.hip: a relaxed load first, the atomic only when bits are missing -- a stale
// read costs a redundant atomic, nothing else.
__global__ __launch_bounds__(256) void occ_rays_kernel(const float* __restrict__ depth, int H, int W, OccRayCam cam, int step, int nu, int nv, int tiles_x,
                                                        int ntiles, uint32_t nvox, size_t nvw, uint32_t* __restrict__ mask) {
    const int tile = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const int a = (tile % tiles_x) * 8 + (lane & 7), b = (tile / tiles_x) * 8 + (lane >> 3);
    if (a >= nu || b >= nv) return;
    const int u = step / 2 + a * step, v = step / 2 + b * step;   // a < nu and b < nv: u < W and v < H
    const float d = depth[((size_t)blockIdx.y * H + v) * W + u];
    uint32_t* row = mask + (size_t)blockIdx.y * nvw;
    uint32_t cur = 0xffffffffu, acc = 0;
    auto flush = [&]() {
        if (acc != 0 && (size_t)cur < nvw) {
            uint32_t* wp = row + cur;
            if (~__hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & acc) atomicOr(wp, acc);
        }
    };
    occ_ray_walk(cam, u, v, d, [&](uint32_t m) {
        if (m >= nvox) return;
        const uint32_t w = m >> 5;
        if (w != cur) {
            flush();
            cur = w;
            acc = 0;
        }
        acc |= 1u << (m & 31);
    });
    flush();
}

// the C class bits of the voxel whose first bit is `bit` (bit + C <= ncell, so the second word exists whenever the voxel reaches into it)
__device__ __forceinline__ uint32_t voxel_bits(const uint32_t* __restrict__ row, size_t bit, int C) {
    const size_t w = bit >> 5;
    const uint32_t off = (uint32_t)(bit & 31);
    uint32_t m = row[w] >> off;
    if (off + (uint32_t)C > 32u) m |= row[w + 1] << (32u - off);   // off >= 25 here: the shift is 1 .. 7
    return m & ((1u << C) - 1u);
}

// One lane per voxel.  counts[r][c][4] += {|p & g|, |p | g|, |p|, |g|} over the voxels of the effective mask, observed[r] += their number;
// pred_stride / mask_stride 0 broadcast one row.
__global__ __launch_bounds__(256) void occ_iou_masked_kernel(const uint32_t* __restrict__ pred, size_t pred_stride, const uint32_t* __restrict__ gt, size_t nwords,
                                                              const uint32_t* __restrict__ mask, size_t mask_stride, size_t nvox, int C, int include_gt,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ observed) {
    __shared__ uint32_t sh[4][33];
    const size_t r = blockIdx.y;
    const uint32_t* prow = pred + r * pred_stride;
    const uint32_t* grow = gt + r * nwords;
    const uint32_t* mrow = mask + r * mask_stride;
    uint32_t cnt[33];
#pragma unroll
    for (int i = 0; i < 33; ++i) cnt[i] = 0;
    for (size_t vox = (size_t)blockIdx.x * 256 + threadIdx.x; vox < nvox; vox += (size_t)gridDim.x * 256) {
        const uint32_t g = voxel_bits(grow, vox * (size_t)C, C);
        const bool in = ((mrow[vox >> 5] >> (vox & 31)) & 1u) || (include_gt && g != 0);
        if (!in) continue;
        const uint32_t p = voxel_bits(prow, vox * (size_t)C, C);
        ++cnt[32];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t pb = (p >> c) & 1u, gb = (g >> c) & 1u;
            cnt[4 * c] += pb & gb;
            cnt[4 * c + 1] += pb | gb;
            cnt[4 * c + 2] += pb;
            cnt[4 * c + 3] += gb;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 33; ++i) {
        uint32_t v = cnt[i];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
        if (lane == 0) sh[wave][i] = v;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < C * 4 || t == 32) {
        const uint32_t v = sh[0][t] + sh[1][t] + sh[2][t] + sh[3][t];
        if (t == 32) {
            if (observed && v) atomicAdd(&observed[r], (unsigned long long)v);
        } else if (v) {
            atomicAdd(&counts[r * (size_t)(C * 4) + t], (unsigned long long)v);   // integer sums: the order does not matter
        }
    }
}

bool finite_all(const double* p, int n) {
    for (int i = 0; i < n; ++i)
        if (!(p[i] - p[i] == 0.0)) return false;
    return true;
}

}  // namespace

int launch_occ_rays_observed(const float* depth, int rows, int H, int W, const int* grid3, const double* camera_to_voxel, const double* intrinsics,
                             double z_near, double max_depth, int step, int clear, uint32_t* mask, hipStream_t st, std::string& err) {
    if (!depth || !grid3 || !camera_to_voxel || !intrinsics || !mask) { err = "occ_rays_observed: null argument"; return 1; }
    if (rows < 1 || rows > 65535 || H < 1 || W < 1 || step < 1) { err = "occ_rays_observed: need 1 <= rows <= 65535 and H, W, step >= 1"; return 1; }
    const size_t lim = (size_t)1 << 31;
    size_t nvox = 0;
    bool ok = grid3[0] >= 1 && grid3[1] >= 1 && grid3[2] >= 1;
    if (ok) {
        nvox = (size_t)grid3[0] * (size_t)grid3[1];   // < 2^62
        ok = nvox < lim && (nvox *= (size_t)grid3[2]) < lim;
    }
    if (!ok) { err = "occ_rays_observed: need a grid of positive sizes with g0 * g1 * g2 < 2^31"; return 1; }
    if (!finite_all(camera_to_voxel, 12) || !finite_all(intrinsics, 4) || !finite_all(&z_near, 1) || !finite_all(&max_depth, 1)) {
        err = "occ_rays_observed: camera_to_voxel, the intrinsics, z_near and max_depth must be finite";
        return 1;
    }
    if (intrinsics[0] == 0.0 || intrinsics[1] == 0.0 || z_near < 0.0) { err = "occ_rays_observed: need fx != 0, fy != 0 and z_near >= 0"; return 1; }
    const int nu = occ_rays_cast_count(W, step), nv = occ_rays_cast_count(H, step);
    const size_t tiles_x = ((size_t)nu + 7) / 8, ntiles = tiles_x * (((size_t)nv + 7) / 8);
    if (ntiles >= lim) { err = "occ_rays_observed: too many cast pixels (8 x 8 tiles of them must number below 2^31)"; return 1; }
    const size_t nvw = (nvox + 31) / 32;
    if (clear && hipMemsetAsync(mask, 0, (size_t)rows * nvw * sizeof(uint32_t), st) != hipSuccess) { err = "occ_rays_observed: memset failed"; return 1; }
    if (ntiles == 0) return 0;   // step / 2 is outside the frame: no pixel is cast
    OccRayCam cam;
    for (int i = 0; i < 12; ++i) cam.N[i] = camera_to_voxel[i];
    cam.fx = intrinsics[0]; cam.fy = intrinsics[1]; cam.cx = intrinsics[2]; cam.cy = intrinsics[3];
    cam.z_near = z_near; cam.max_depth = max_depth;
    cam.g[0] = grid3[0]; cam.g[1] = grid3[1]; cam.g[2] = grid3[2];
    SOCCDPT_LAUNCH(occ_rays_kernel, dim3((unsigned)((ntiles + 3) / 4), (unsigned)rows), dim3(256), 0, st, depth, H, W, cam, step, nu, nv, (int)tiles_x, (int)ntiles,
                   (uint32_t)nvox, nvw, mask);
    return check_launch("occ_rays_observed", err);
}

int launch_occ_iou_counts_masked(const uint32_t* pred_bits, int pred_rows, const uint32_t* gt_bits, int rows, size_t nvox, int C, const uint32_t* mask,
                                 int mask_rows, int include_gt, uint64_t* counts, uint64_t* observed, hipStream_t st, std::string& err) {
    if (!pred_bits || !gt_bits || !mask || !counts) { err = "occ_iou_counts_masked: null argument"; return 1; }
    if (rows < 1 || rows > 65535 || C < 1 || C > 8 || nvox == 0 || nvox >= ((size_t)1 << 31)) {
        err = "occ_iou_counts_masked: need 1 <= rows <= 65535, 1 <= C <= 8 and 1 <= nvox < 2^31";
        return 1;
    }
    if ((pred_rows != 1 && pred_rows != rows) || (mask_rows != 1 && mask_rows != rows)) {
        err = "occ_iou_counts_masked: pred_rows and mask_rows must be 1 or rows";
        return 1;
    }
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
    if (hipMemsetAsync(counts, 0, (size_t)rows * C * 4 * sizeof(uint64_t), st) != hipSuccess ||
        (observed && hipMemsetAsync(observed, 0, (size_t)rows * sizeof(uint64_t), st) != hipSuccess)) {
        err = "occ_iou_counts_masked: memset failed";
        return 1;
    }
    const size_t nwords = (nvox * (size_t)C + 31) / 32, nvw = (nvox + 31) / 32;
    size_t blocks = (nvox + 255) / 256;
    if (blocks > 1024) blocks = 1024;   // a lane then counts at most 2^31 / 2^18 voxels: its 32-bit counters cannot wrap
    SOCCDPT_LAUNCH(occ_iou_masked_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, st, pred_bits, pred_rows == 1 ? (size_t)0 : nwords, gt_bits, nwords,
                   mask, mask_rows == 1 ? (size_t)0 : nvw, nvox, C, include_gt ? 1 : 0, reinterpret_cast<unsigned long long*>(counts),
                   reinterpret_cast<unsigned long long*>(observed));
    return check_launch("occ_iou_counts_masked", err);
}

}  // namespace soccdpt
