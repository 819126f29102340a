// Pictures of the packed semantic occupancy grid (include/soccdpt_occ_view.h): the consumer the point lists and the 3-D IoU of occ_eval.hip leave out.
//   columns   reduce the grid along one axis: first occupied cell, its highest class, occupied cells and the OR of the class masks per column
//   paint     a column map -> u8 x 3 picture (class colour, shaded by the depth of the first cell), written into a destination rectangle
//   iou2d     per-class (intersection, union, pred, gt) counts of two `classes` maps
//   splat     every set bit -> its voxel centre in camera space -> a square of pixels, atomicMin of (f32 depth bits, cell index) into a z-buffer
//   resolve   z-buffer + camera frame -> the frame with the nearest voxel's class colour blended over it
// Bit layout (projection.hip occ_expand_kernel, occ_eval.hip): cell n = row-major index of [g0][g1][g2][C], class n % C, bit n & 31 of word n >> 5.
// Here a "voxel" is the C consecutive bits of one (i0, i1, i2); C need not divide 32, so a voxel's bits can lie in two words.  Every reader
// addresses bits below ncell only, so whatever the last word holds beyond them is never looked at.
//
// The splat carries a bit-exact contract with a numpy float64 restatement (tests/occ_view_refs.py): every product and sum below is rounded on its
// own, in the order written.  The pragma turns contraction off whatever -ffp-contract the file is compiled with; the f64 divisions are IEEE.
#pragma clang fp contract(off)
#include "occ_view.h"

#include "kernels.h"
#include "launch.h"

namespace soccdpt {

namespace {

// the C class bits of the voxel whose first bit is `bit` (bit + C <= ncell, so the second word exists whenever the voxel reaches into it)
__device__ __forceinline__ uint32_t voxel_mask(const uint32_t* __restrict__ row, size_t bit, int C) {
    const size_t w = bit >> 5;
    const uint32_t off = (uint32_t)(bit & 31);
    uint32_t m = row[w] >> off;
    if (off + (uint32_t)C > 32u) m |= row[w + 1] << (32u - off);   // off >= 25 here: the shift is 1 .. 7
    return m & ((1u << C) - 1u);
}

// One lane per column.  Column (a, b) holds the voxels a * sa + b * sb + k * sl, k < len (strides in voxels).
__global__ __launch_bounds__(256) void occ_view_columns_kernel(const uint32_t* __restrict__ bits, size_t nwords, int C, size_t ncol, uint32_t B, uint32_t len,
                                                                size_t sa, size_t sb, size_t sl, int from_high, uint8_t* __restrict__ top,
                                                                int32_t* __restrict__ first, int32_t* __restrict__ count, uint8_t* __restrict__ classes) {
    const size_t col = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncol) return;
    const uint32_t* row = bits + (size_t)blockIdx.y * nwords;
    const size_t base = (col / B) * sa + (col % B) * sb;
    int32_t f = -1, cnt = 0;
    uint32_t fm = 0, all = 0;
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t kk = from_high ? len - 1u - k : k;
        const uint32_t m = voxel_mask(row, (base + (size_t)kk * sl) * (size_t)C, C);
        if (m) {
            if (f < 0) { f = (int32_t)kk; fm = m; }
            ++cnt;
            all |= m;
        }
    }
    const size_t o = (size_t)blockIdx.y * ncol + col;
    if (top) top[o] = f < 0 ? (uint8_t)255 : (uint8_t)(31 - __clz((int)fm));   // the last matching class wins, as in color_masks
    if (first) first[o] = f;
    if (count) count[o] = cnt;
    if (classes) classes[o] = (uint8_t)all;
}

struct PaintArgs {
    int A, B, depth_len, from_high, C, shade, zoom, flip_a, flip_b, transpose, PH, PW;
    uint8_t background[3];
};

// One lane per picture pixel.  rank = distance of the first cell from the side the scan started at; w = 256 - shade * rank / max(depth_len - 1, 1).
__global__ __launch_bounds__(256) void occ_view_paint_kernel(const uint8_t* __restrict__ top, const int32_t* __restrict__ first,
                                                              const uint8_t* __restrict__ colors, PaintArgs p, uint8_t* __restrict__ dst, VisDst d) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)p.PH * p.PW) return;
    const int y = (int)(t / p.PW), x = (int)(t % p.PW);
    int a = (p.transpose ? x : y) / p.zoom, b = (p.transpose ? y : x) / p.zoom;
    if (p.flip_a) a = p.A - 1 - a;
    if (p.flip_b) b = p.B - 1 - b;
    const size_t col = ((size_t)blockIdx.y * p.A + a) * p.B + b;
    const int f = first[col];
    const int c = top[col];
    uint8_t* out = dst + 3 * ((size_t)blockIdx.y * d.frame_px + d.offset_px + (size_t)y * d.pitch_px + (size_t)x);
    if (f < 0 || c >= p.C) {   // an empty column (a class id outside the table is treated as one: nothing is read outside `colors`)
        out[0] = p.background[0]; out[1] = p.background[1]; out[2] = p.background[2];
        return;
    }
    int rank = p.from_high ? p.depth_len - 1 - f : f;
    rank = rank < 0 ? 0 : (rank > p.depth_len - 1 ? p.depth_len - 1 : rank);
    const int w = 256 - (p.shade * rank) / (p.depth_len - 1 > 1 ? p.depth_len - 1 : 1);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)(((int)colors[3 * c + ch] * w + 128) >> 8);
}

// counts[r][c][4] += {|p & g|, |p | g|, |p|, |g|} over the columns, bit c of a map's byte standing for class c; pred_stride 0 broadcasts one map
__global__ __launch_bounds__(256) void occ_view_iou2d_kernel(const uint8_t* __restrict__ pred, size_t pred_stride, const uint8_t* __restrict__ gt, size_t ncol,
                                                              int C, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t sh[4][32];
    const size_t r = blockIdx.y;
    const uint32_t keep = (1u << C) - 1u;
    uint32_t cnt[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) cnt[i] = 0;
    for (size_t col = (size_t)blockIdx.x * 256 + threadIdx.x; col < ncol; col += (size_t)gridDim.x * 256) {
        const uint32_t p = pred[r * pred_stride + col] & keep, g = gt[r * ncol + col] & keep;
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
    for (int i = 0; i < 32; ++i) {
        uint32_t v = cnt[i];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
        if (lane == 0) sh[wave][i] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < C * 4) {
        const uint32_t v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (v) atomicAdd(&counts[r * (size_t)(C * 4) + threadIdx.x], (unsigned long long)v);   // integer sums: the order does not matter
    }
}

struct SplatCam {
    double M[12], fx, fy, cx, cy, half_extent, z_near;
    int max_r;
};

// One lane per word; every set bit n projects its voxel centre and takes part in the atomicMin of the pixels of its square.  The key orders by the
// f32 depth first (positive, so its bit pattern orders like the value) and by the cell index second: the result does not depend on who comes first.
__global__ __launch_bounds__(256) void occ_view_splat_kernel(const uint32_t* __restrict__ bits, size_t nwords, size_t ncell, uint32_t C, uint32_t g1, uint32_t g2,
                                                              SplatCam cam, int H, int W, unsigned long long* __restrict__ zbuf) {
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= nwords) return;
    uint32_t w = bits[(size_t)blockIdx.y * nwords + wi];
    if (wi == nwords - 1 && (ncell & 31)) w &= (1u << (uint32_t)(ncell & 31)) - 1u;
    unsigned long long* zb = zbuf + (size_t)blockIdx.y * H * W;
    while (w) {
        const uint32_t n = (uint32_t)(wi * 32) + (uint32_t)__builtin_ctz(w);
        w &= w - 1;
        const uint32_t cell = n / C;
        const uint32_t i2 = cell % g2, ij = cell / g2;
        const uint32_t i1 = ij % g1, i0 = ij / g1;
        const double a = (double)i0 + 0.5, b = (double)i1 + 0.5, c = (double)i2 + 0.5;
        const double X = ((cam.M[0] * a + cam.M[1] * b) + cam.M[2] * c) + cam.M[3];
        const double Y = ((cam.M[4] * a + cam.M[5] * b) + cam.M[6] * c) + cam.M[7];
        const double Z = ((cam.M[8] * a + cam.M[9] * b) + cam.M[10] * c) + cam.M[11];
        if (!(Z > cam.z_near)) continue;   // behind or too close to the camera; NaN
        const double u = floor(((X / Z) * cam.fx + cam.cx) + 0.5);
        const double v = floor(((Y / Z) * cam.fy + cam.cy) + 0.5);
        const double rd = floor((cam.half_extent / Z) * cam.fx);
        // a centre this far out cannot reach the frame with r <= 256 (and NaN fails the comparison): nothing to convert to int that does not fit
        if (!(u >= -1073741824.0 && u <= 1073741824.0 && v >= -1073741824.0 && v <= 1073741824.0 && rd >= 0.0)) continue;
        const int r = rd >= (double)cam.max_r ? cam.max_r : (int)rd;
        const int ui = (int)u, vi = (int)v;
        const int x0 = ui - r > 0 ? ui - r : 0, x1 = ui + r < W - 1 ? ui + r : W - 1;
        const int y0 = vi - r > 0 ? vi - r : 0, y1 = vi + r < H - 1 ? vi + r : H - 1;
        const unsigned long long key = ((unsigned long long)__float_as_uint((float)Z) << 32) | (unsigned long long)n;
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) atomicMin(&zb[(size_t)y * W + x], key);
    }
}

// One lane per pixel: the frame where the z-buffer is untouched, else (frame * (256 - alpha) + colour * alpha + 128) >> 8
__global__ __launch_bounds__(256) void occ_view_resolve_kernel(const unsigned long long* __restrict__ zbuf, const uint8_t* __restrict__ frames, size_t frame_stride,
                                                                int H, int W, uint32_t C, const uint8_t* __restrict__ colors, int alpha,
                                                                uint8_t* __restrict__ dst, VisDst d) {
    const size_t npix = (size_t)H * W;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix) return;
    const size_t y = t / (size_t)W, x = t % (size_t)W;
    const unsigned long long key = zbuf[(size_t)blockIdx.y * npix + t];
    uint8_t* out = dst + 3 * ((size_t)blockIdx.y * d.frame_px + d.offset_px + y * d.pitch_px + x);
    int f[3] = {0, 0, 0};
    if (frames) {
        const uint8_t* p = frames + 3 * ((size_t)blockIdx.y * frame_stride + t);
        f[0] = p[0]; f[1] = p[1]; f[2] = p[2];
    }
    if (key == ~0ull) {
        out[0] = (uint8_t)f[0]; out[1] = (uint8_t)f[1]; out[2] = (uint8_t)f[2];
        return;
    }
    const uint32_t c = (uint32_t)(key & 0xffffffffull) % C;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[ch] = (uint8_t)((f[ch] * (256 - alpha) + (int)colors[3 * c + ch] * alpha + 128) >> 8);
}

struct GridGeom {
    size_t nvox, ncell, nwords;   // voxels (g0 g1 g2), cells (x C), words per row
};

// rows, grid and C of a packed grid: g0 * g1 * g2 * C < 2^32, checked without overflow
bool grid_ok(int rows, const int* g, int C, GridGeom& geo, const char* what, std::string& err) {
    const size_t lim = (size_t)1 << 32;
    bool ok = rows >= 1 && rows <= 65535 && g && C >= 1 && C <= 8 && g[0] >= 1 && g[1] >= 1 && g[2] >= 1;
    if (ok) {
        geo.nvox = (size_t)g[0] * (size_t)g[1];   // < 2^62
        ok = geo.nvox < lim && (geo.nvox *= (size_t)g[2]) < lim && (geo.ncell = geo.nvox * (size_t)C) < lim;
    }
    if (!ok) {
        err = std::string(what) + ": need 1 <= rows <= 65535, 1 <= C <= 8 and a grid of positive sizes with g0 * g1 * g2 * C < 2^32";
        return false;
    }
    geo.nwords = (geo.ncell + 31) / 32;
    return true;
}

dim3 lanes_grid(size_t lanes, int rows) { return dim3((unsigned)((lanes + 255) / 256), (unsigned)rows); }

}  // namespace

int launch_occ_view_columns(const uint32_t* bits, int rows, const int* grid3, int C, int axis, int from_high, uint8_t* top, int32_t* first, int32_t* count,
                            uint8_t* classes, hipStream_t st, std::string& err) {
    GridGeom geo;
    if (!grid_ok(rows, grid3, C, geo, "occ_view_columns", err)) return 1;
    if (axis < 0 || axis > 2) { err = "occ_view_columns: axis must be 0, 1 or 2"; return 1; }
    if (!bits) { err = "occ_view_columns: null bits"; return 1; }
    if (!top && !first && !count && !classes) return 0;
    const size_t stride[3] = {(size_t)grid3[1] * (size_t)grid3[2], (size_t)grid3[2], 1};
    const int ia = axis == 0 ? 1 : 0, ib = axis == 2 ? 1 : 2;   // the two remaining axes, ascending
    const size_t ncol = (size_t)grid3[ia] * (size_t)grid3[ib];
    SOCCDPT_LAUNCH(occ_view_columns_kernel, lanes_grid(ncol, rows), dim3(256), 0, st, bits, geo.nwords, C, ncol, (uint32_t)grid3[ib], (uint32_t)grid3[axis],
                   stride[ia], stride[ib], stride[axis], from_high ? 1 : 0, top, first, count, classes);
    return check_launch("occ_view_columns", err);
}

int launch_occ_view_paint(const uint8_t* top, const int32_t* first, int rows, int A, int B, int depth_len, int from_high, const uint8_t* class_colors, int C,
                          const uint8_t* background, int shade, int zoom, int flip_a, int flip_b, int transpose, uint8_t* dst, const VisDst& d,
                          hipStream_t st, std::string& err) {
    if (!top || !first || !class_colors || !background || !dst) { err = "occ_view_paint: null argument"; return 1; }
    if (C < 1 || C > 8 || zoom < 1 || shade < 0 || shade > 192 || depth_len < 1 || A < 1 || B < 1) {
        err = "occ_view_paint: need 1 <= C <= 8, zoom >= 1, 0 <= shade <= 192, depth_len >= 1 and A, B >= 1";
        return 1;
    }
    const size_t ha = (size_t)A * (size_t)zoom, wb = (size_t)B * (size_t)zoom;
    if (ha > ((size_t)1 << 24) || wb > ((size_t)1 << 24)) { err = "occ_view_paint: A * zoom and B * zoom may be at most 2^24"; return 1; }
    PaintArgs p{A, B, depth_len, from_high ? 1 : 0, C, shade, zoom, flip_a ? 1 : 0, flip_b ? 1 : 0, transpose ? 1 : 0, (int)(transpose ? wb : ha), (int)(transpose ? ha : wb),
                {background[0], background[1], background[2]}};
    if (!vis_image_ok(rows, p.PH, p.PW, "occ_view_paint", err) || !vis_dst_ok(rows, p.PH, p.PW, d, "occ_view_paint", err)) return 1;
    SOCCDPT_LAUNCH(occ_view_paint_kernel, lanes_grid((size_t)p.PH * p.PW, rows), dim3(256), 0, st, top, first, class_colors, p, dst, d);
    return check_launch("occ_view_paint", err);
}

int launch_occ_view_iou2d(const uint8_t* pred_classes, int pred_rows, const uint8_t* gt_classes, int rows, size_t ncol, int C, uint64_t* counts,
                          hipStream_t st, std::string& err) {
    if (rows < 1 || rows > 65535 || C < 1 || C > 8 || ncol == 0 || ncol > ((size_t)1 << 32)) {
        err = "occ_view_iou2d: need 1 <= rows <= 65535, 1 <= C <= 8 and 1 <= ncol <= 2^32";
        return 1;
    }
    if (!pred_classes || !gt_classes || !counts || (pred_rows != 1 && pred_rows != rows)) { err = "occ_view_iou2d: null argument, or pred_rows is neither 1 nor rows"; return 1; }
    if (hipMemsetAsync(counts, 0, (size_t)rows * C * 4 * sizeof(uint64_t), st) != hipSuccess) { err = "occ_view_iou2d: memset failed"; return 1; }
    size_t blocks = (ncol + 255) / 256;
    if (blocks > 1024) blocks = 1024;   // a lane then counts at most 2^32 / 2^18 columns: its 32-bit counters cannot wrap
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are 64-bit");
    SOCCDPT_LAUNCH(occ_view_iou2d_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, st, pred_classes, pred_rows == 1 ? (size_t)0 : ncol, gt_classes, ncol,
                   C, reinterpret_cast<unsigned long long*>(counts));
    return check_launch("occ_view_iou2d", err);
}

int launch_occ_view_splat(const uint32_t* bits, int rows, const int* grid3, int C, const double* voxel_to_camera, const double* intrinsics,
                          double half_extent_m, int max_radius_px, double z_near, int H, int W, uint64_t* zbuf, hipStream_t st, std::string& err) {
    GridGeom geo;
    if (!grid_ok(rows, grid3, C, geo, "occ_view_splat", err)) return 1;
    if (!bits || !voxel_to_camera || !intrinsics || !zbuf) { err = "occ_view_splat: null argument"; return 1; }
    if (!vis_image_ok(rows, H, W, "occ_view_splat", err)) return 1;
    if (max_radius_px < 0 || max_radius_px > kOccViewMaxRadiusPx) { err = "occ_view_splat: max_radius_px must be 0 .. 256"; return 1; }
    if (hipMemsetAsync(zbuf, 0xff, (size_t)rows * H * W * sizeof(uint64_t), st) != hipSuccess) { err = "occ_view_splat: memset failed"; return 1; }
    SplatCam cam;
    for (int i = 0; i < 12; ++i) cam.M[i] = voxel_to_camera[i];
    cam.fx = intrinsics[0]; cam.fy = intrinsics[1]; cam.cx = intrinsics[2]; cam.cy = intrinsics[3];
    cam.half_extent = half_extent_m; cam.z_near = z_near; cam.max_r = max_radius_px;
    SOCCDPT_LAUNCH(occ_view_splat_kernel, lanes_grid(geo.nwords, rows), dim3(256), 0, st, bits, geo.nwords, geo.ncell, (uint32_t)C, (uint32_t)grid3[1],
                   (uint32_t)grid3[2], cam, H, W, reinterpret_cast<unsigned long long*>(zbuf));
    return check_launch("occ_view_splat", err);
}

int launch_occ_view_resolve(const uint64_t* zbuf, const uint8_t* frames, int frame_rows, int rows, int H, int W, int C, const uint8_t* class_colors,
                            int alpha, uint8_t* dst, const VisDst& d, hipStream_t st, std::string& err) {
    if (!zbuf || !class_colors || !dst) { err = "occ_view_resolve: null argument"; return 1; }
    if (C < 1 || C > 8 || alpha < 0 || alpha > 256 || H < 1 || W < 1) { err = "occ_view_resolve: need 1 <= C <= 8, 0 <= alpha <= 256 and H, W >= 1"; return 1; }
    if (frames && frame_rows != 1 && frame_rows != rows) { err = "occ_view_resolve: frame_rows is neither 1 nor rows"; return 1; }
    if (!vis_image_ok(rows, H, W, "occ_view_resolve", err) || !vis_dst_ok(rows, H, W, d, "occ_view_resolve", err)) return 1;
    const size_t frame_stride = frame_rows == 1 ? 0 : (size_t)H * W;
    SOCCDPT_LAUNCH(occ_view_resolve_kernel, lanes_grid((size_t)H * W, rows), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(zbuf), frames, frame_stride,
                   H, W, (uint32_t)C, class_colors, alpha, dst, d);
    return check_launch("occ_view_resolve", err);
}

}  // namespace soccdpt
