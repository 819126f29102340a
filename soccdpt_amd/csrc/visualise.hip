// The evaluation pictures of the reference on the GPU (include/soccdpt_vis.h):
//   per-frame min / max + colour map   SOccDPT/utils/__init__.py:649-655   ((d - min) / (max - min) * 255).astype(np.uint8) -> cv2.applyColorMap
//   class maps -> class colours        SOccDPT/utils/__init__.py:35-43     color_segmentation: later classes overwrite earlier ones
//   bilinear resize of u8 x 3          cv2.resize(img, (W, H)): half-pixel centres, clamped borders, 11-bit integer weights
//   half-size shrink (+ B <-> R)       cv2.resize(img, (0, 0), fx=0.5, fy=0.5) after cv2.cvtColor(img, cv2.COLOR_BGR2RGB)
// Every kernel here is element-wise or a min / max reduction and bound by memory traffic.  A lane owns 4 consecutive pixels of one row: one 16-byte
// load of f32 inputs and three 4-byte stores of u8 x 3 output when the addresses allow it, guarded element accesses otherwise (any W, any pitch).
//
// The colouring carries a byte-exact contract with numpy: v = (d - mn) / (mx - mn) in f32 (one subtract, one IEEE divide), idx = (uint8)(v * 255.0f)
// truncated.  None of these is a multiply followed by an add, so there is nothing to contract; the pragma keeps it that way whatever -ffp-contract
// the file is compiled with.  The resize and the shrink are integer arithmetic.
#pragma clang fp contract(off)
#include "visualise.h"

#include <cmath>

#include "kernels.h"
#include "launch.h"

namespace soccdpt {

namespace {

typedef __attribute__((ext_vector_type(4))) float v4f;

constexpr int kPx = 4;   // pixels per lane

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) < __builtin_inff(); }   // NaN: false

// 4 floats from p (n of them valid): one 16-byte load when whole and aligned; elements past n read as `fill`.  kStream: the data is not read
// again (non-temporal load).  The min / max pass leaves it off: the colour-map pass reads the same frame right after it.
template <bool kStream>
__device__ __forceinline__ void load_f4(const float* __restrict__ p, int n, float fill, float (&v)[kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const v4f q = kStream ? __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p)) : *reinterpret_cast<const v4f*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j) v[j] = j < n ? p[j] : fill;
    }
}

// the 3 * n bytes of n <= 4 pixels to p: three 4-byte stores when whole and aligned
__device__ __forceinline__ void store_px(uint8_t* __restrict__ p, int n, const uint8_t (&c)[3 * kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int w = 0; w < 3; ++w)
            q[w] = (uint32_t)c[4 * w] | ((uint32_t)c[4 * w + 1] << 8) | ((uint32_t)c[4 * w + 2] << 16) | ((uint32_t)c[4 * w + 3] << 24);
    } else {
        for (int j = 0; j < 3 * n; ++j) p[j] = c[j];
    }
}

// the 3 * n bytes of n <= 4 pixels from p; bytes past them read as 0
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ p, int n, uint8_t (&c)[3 * kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const uint32_t u = q[w];
            c[4 * w] = (uint8_t)u; c[4 * w + 1] = (uint8_t)(u >> 8); c[4 * w + 2] = (uint8_t)(u >> 16); c[4 * w + 3] = (uint8_t)(u >> 24);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3 * kPx; ++j) c[j] = j < 3 * n ? p[j] : (uint8_t)0;
    }
}

// lane -> (row y, first column x0, valid pixels n) of an H x W image cut into groups of 4 pixels per row; false past the image
__device__ __forceinline__ bool lane_pixels(int H, int W, int& y, int& x0, int& n) {
    const unsigned gpr = (unsigned)(W + kPx - 1) / kPx;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)H * gpr) return false;
    y = (int)(t / gpr);
    x0 = (int)(t % gpr) * kPx;
    n = W - x0 < kPx ? W - x0 : kPx;
    return true;
}

__device__ __forceinline__ uint8_t* dst_px(uint8_t* dst, const VisDst& d, int b, int y, int x) {
    return dst + 3 * ((size_t)b * d.frame_px + d.offset_px + (size_t)y * d.pitch_px + (size_t)x);
}

// ---- min / max ----
// minmax[b] = {min, max} over the finite values of row b ({+inf, -inf} when there is none).  Two stages: every workgroup reduces its share in
// registers, across the wave and through LDS and writes one {lo, hi} pair to part[b][workgroup]; one workgroup per row reduces the pairs.  No
// atomics (a one-stage form whose workgroups ended in an atomic pair on minmax[b] took 1.8x as long: DESIGN.md section 12.2); min and max do not
// depend on the order anyway.  -0 is reported as +0.
__global__ __launch_bounds__(256) void vis_minmax_partial_kernel(const float* __restrict__ x, size_t npix, float* __restrict__ part) {
    __shared__ float sh[2][4];
    const float* row = x + (size_t)blockIdx.y * npix;
    const size_t ngroups = (npix + kPx - 1) / kPx;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t left = npix - g * kPx;
        float v[kPx];
        load_f4<false>(row + g * kPx, left < (size_t)kPx ? (int)left : kPx, __builtin_nanf(""), v);
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (finite_f32(v[j])) { lo = fminf(lo, v[j]); hi = fmaxf(hi, v[j]); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = lo; sh[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* p = part + 2 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        p[0] = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
        p[1] = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
    }
}
__global__ __launch_bounds__(256) void vis_minmax_finish_kernel(const float* __restrict__ part, int nblk, float* __restrict__ minmax) {
    __shared__ float sh[2][4];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int i = threadIdx.x; i < nblk; i += 256) {
        lo = fminf(lo, part[2 * ((size_t)blockIdx.x * nblk + i)]);
        hi = fmaxf(hi, part[2 * ((size_t)blockIdx.x * nblk + i) + 1]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = lo; sh[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = fminf(fminf(sh[0][0], sh[0][1]), fminf(sh[0][2], sh[0][3]));
        hi = fmaxf(fmaxf(sh[1][0], sh[1][1]), fmaxf(sh[1][2], sh[1][3]));
        if (lo == 0.0f) lo = 0.0f;
        if (hi == 0.0f) hi = 0.0f;
        minmax[2 * blockIdx.x] = lo;
        minmax[2 * blockIdx.x + 1] = hi;
    }
}

// ---- inverse depth -> colour map ----
__global__ __launch_bounds__(256) void vis_colorize_kernel(const float* __restrict__ x, const float* __restrict__ minmax, const uint8_t* __restrict__ lut,
                                                            int H, int W, uint8_t* __restrict__ dst, VisDst d) {
    __shared__ uint8_t sl[256 * 3];
    for (int i = threadIdx.x; i < 256 * 3; i += 256) sl[i] = lut[i];
    __syncthreads();
    int y, x0, n;
    if (!lane_pixels(H, W, y, x0, n)) return;
    const int b = blockIdx.y;
    const float mn = minmax[2 * b], mx = minmax[2 * b + 1];
    const float range = mx - mn;
    const bool usable = mx > mn;   // false for a constant frame and for a frame without a finite value
    float v[kPx];
    load_f4<true>(x + ((size_t)b * H + y) * W + x0, n, 0.0f, v);
    uint8_t c[3 * kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        const float u = (v[j] - mn) / range;
        // a finite pixel of a usable frame gives 0 <= u <= 1; everything the reference leaves undefined (NaN, +-inf, max == min) takes index 0
        const int idx = (usable && finite_f32(v[j]) && u >= 0.0f && u <= 1.0f) ? (int)(u * 255.0f) : 0;
        c[3 * j] = sl[3 * idx];
        c[3 * j + 1] = sl[3 * idx + 1];
        c[3 * j + 2] = sl[3 * idx + 2];
    }
    store_px(dst_px(dst, d, b, y, x0), n, c);
}

// ---- class maps -> class colours ----
// seg [B][C][H][W] (channels_last == 0) or [B][H][W][C]; colours [C][3], written as they are given.  The colour of the last class whose value is > 0.5.
__global__ __launch_bounds__(256) void vis_color_masks_kernel(const float* __restrict__ seg, int C, int H, int W, int channels_last,
                                                               const uint8_t* __restrict__ colors, uint8_t* __restrict__ dst, VisDst d) {
    int y, x0, n;
    if (!lane_pixels(H, W, y, x0, n)) return;
    const int b = blockIdx.y;
    uint8_t c[3 * kPx];
#pragma unroll
    for (int j = 0; j < 3 * kPx; ++j) c[j] = 0;
    const size_t hw = (size_t)H * W, px = (size_t)y * W + x0;
    for (int k = 0; k < C; ++k) {
        float v[kPx];
        if (channels_last) {
            const float* p = seg + ((size_t)b * hw + px) * C + k;
#pragma unroll
            for (int j = 0; j < kPx; ++j) v[j] = j < n ? p[(size_t)j * C] : 0.0f;
        } else {
            load_f4<true>(seg + ((size_t)b * C + k) * hw + px, n, 0.0f, v);
        }
        const uint8_t c0 = colors[3 * k], c1 = colors[3 * k + 1], c2 = colors[3 * k + 2];
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (v[j] > 0.5f) {   // 0.5 itself and NaN do not match
                c[3 * j] = c0;
                c[3 * j + 1] = c1;
                c[3 * j + 2] = c2;
            }
    }
    store_px(dst_px(dst, d, b, y, x0), n, c);
}

// ---- resize ----
__global__ __launch_bounds__(256) void vis_copy_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst, VisDst d) {
    int y, x0, n;
    if (!lane_pixels(H, W, y, x0, n)) return;
    const int b = blockIdx.y;
    uint8_t c[3 * kPx];
    load_px(src + 3 * (((size_t)b * H + y) * W + x0), n, c);
    store_px(dst_px(dst, d, b, y, x0), n, c);
}

// taps [len][3] = {i0, i1, w1}; the indices are clamped here as well, so a bad table cannot make the kernel read outside the source
__device__ __forceinline__ void read_taps(const int32_t* __restrict__ taps, int i, int src_len, int& i0, int& i1, uint32_t& w0, uint32_t& w1) {
    const int a = taps[3 * i], c = taps[3 * i + 1], w = taps[3 * i + 2];
    i0 = a < 0 ? 0 : (a > src_len - 1 ? src_len - 1 : a);
    i1 = c < 0 ? 0 : (c > src_len - 1 ? src_len - 1 : c);
    w1 = (uint32_t)(w < 0 ? 0 : (w > 2048 ? 2048 : w));
    w0 = 2048u - w1;
}

// out = (sum over the four taps of p * wx * wy + 2^21) >> 22, wx + wx' = wy + wy' = 2048: at most 255 * 2^22 + 2^21 < 2^31
__global__ __launch_bounds__(256) void vis_resize_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, const int32_t* __restrict__ ytaps,
                                                          const int32_t* __restrict__ xtaps, int Hd, int Wd, uint8_t* __restrict__ dst, VisDst d) {
    int y, x0, n;
    if (!lane_pixels(Hd, Wd, y, x0, n)) return;
    const int b = blockIdx.y;
    int ya, yb;
    uint32_t wy0, wy1;
    read_taps(ytaps, y, Hs, ya, yb, wy0, wy1);
    const uint8_t* ra = src + 3 * ((size_t)b * Hs + ya) * Ws;
    const uint8_t* rb = src + 3 * ((size_t)b * Hs + yb) * Ws;
    uint8_t c[3 * kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        int xa = 0, xb = 0;
        uint32_t wx0 = 2048u, wx1 = 0u;
        if (j < n) read_taps(xtaps, x0 + j, Ws, xa, xb, wx0, wx1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t s = (uint32_t)ra[3 * xa + k] * wx0 * wy0 + (uint32_t)ra[3 * xb + k] * wx1 * wy0 + (uint32_t)rb[3 * xa + k] * wx0 * wy1 +
                               (uint32_t)rb[3 * xb + k] * wx1 * wy1;
            c[3 * j + k] = (uint8_t)((s + (1u << 21)) >> 22);
        }
    }
    store_px(dst_px(dst, d, b, y, x0), n, c);
}

// ---- half-size shrink ----
// out(y, x) = (s(2y, 2x) + s(2y, 2x+1) + s(2y+1, 2x) + s(2y+1, 2x+1) + 2) >> 2, rows and columns clamped to the last; swap_rb exchanges channels 0 and 2
__global__ __launch_bounds__(256) void vis_shrink_half_kernel(const uint8_t* __restrict__ src, int H, int W, int Hd, int Wd, int swap_rb,
                                                               uint8_t* __restrict__ dst) {
    int y, x0, n;
    if (!lane_pixels(Hd, Wd, y, x0, n)) return;
    const int b = blockIdx.y;
    const int ya = 2 * y < H - 1 ? 2 * y : H - 1, yb = 2 * y + 1 < H - 1 ? 2 * y + 1 : H - 1;
    const uint8_t* ra = src + 3 * ((size_t)b * H + ya) * W;
    const uint8_t* rb = src + 3 * ((size_t)b * H + yb) * W;
    uint8_t a[2][3 * kPx], e[2][3 * kPx];   // 8 source columns of each of the two rows
    const int sx = 2 * x0;
    if (sx + 2 * kPx <= W) {
        load_px(ra + 3 * sx, kPx, a[0]);
        load_px(ra + 3 * (sx + kPx), kPx, a[1]);
        load_px(rb + 3 * sx, kPx, e[0]);
        load_px(rb + 3 * (sx + kPx), kPx, e[1]);
    } else {
#pragma unroll
        for (int i = 0; i < 2 * kPx; ++i) {
            const int xs = sx + i < W - 1 ? sx + i : W - 1;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a[i / kPx][3 * (i % kPx) + k] = ra[3 * xs + k];
                e[i / kPx][3 * (i % kPx) + k] = rb[3 * xs + k];
            }
        }
    }
    uint8_t c[3 * kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i0 = 2 * j, i1 = 2 * j + 1;
            const uint32_t s = (uint32_t)a[i0 / kPx][3 * (i0 % kPx) + k] + a[i1 / kPx][3 * (i1 % kPx) + k] + e[i0 / kPx][3 * (i0 % kPx) + k] +
                               e[i1 / kPx][3 * (i1 % kPx) + k];
            c[3 * j + (swap_rb ? 2 - k : k)] = (uint8_t)((s + 2u) >> 2);
        }
    store_px(dst + 3 * (((size_t)b * Hd + y) * Wd + x0), n, c);
}

bool image_ok(int B, int H, int W, const char* what, std::string& err) {
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24) || (size_t)H * (size_t)W > ((size_t)1 << 32)) {
        err = std::string(what) + ": need 1 <= B <= 65535, 1 <= H, W <= 2^24 and H * W <= 2^32";
        return false;
    }
    return true;
}

// every pixel (b, y, x), b < B, y < H, x < W, lies inside the destination buffer and rows / frames do not overlap
bool dst_ok(int B, int H, int W, const VisDst& d, const char* what, std::string& err) {
    const size_t last = d.offset_px + (size_t)(H - 1) * d.pitch_px + (size_t)W;   // one past the last pixel of a frame
    if (d.pitch_px < (size_t)W || d.pitch_px > ((size_t)1 << 32) || d.offset_px > ((size_t)1 << 40) || d.frame_px > ((size_t)1 << 40) ||
        (B > 1 && last > d.frame_px) || (size_t)(B - 1) * d.frame_px + last > d.total_px) {
        err = std::string(what) + ": the destination rectangle (pitch, offset, frame stride) does not fit the destination buffer";
        return false;
    }
    return true;
}

dim3 image_grid(int B, int H, int W) {
    const size_t lanes = (size_t)H * (((size_t)W + kPx - 1) / kPx);
    return dim3((unsigned)((lanes + 255) / 256), (unsigned)B);
}

}  // namespace

bool vis_image_ok(int B, int H, int W, const char* what, std::string& err) { return image_ok(B, H, W, what, err); }
bool vis_dst_ok(int B, int H, int W, const VisDst& d, const char* what, std::string& err) { return dst_ok(B, H, W, d, what, err); }

static size_t minmax_blocks(size_t npix) {
    const size_t blocks = ((npix + kPx - 1) / kPx + 255) / 256;
    return blocks > 1024 ? 1024 : blocks;
}

size_t vis_minmax_scratch_bytes(int B, size_t npix) {
    if (B <= 0 || B > 65535 || npix == 0) return 0;
    return (size_t)B * minmax_blocks(npix) * 2 * sizeof(float);
}

int launch_vis_minmax(const float* x, int B, size_t npix, float* minmax, void* scratch, size_t scratch_bytes, hipStream_t st, std::string& err) {
    if (!x || !minmax || !scratch || B <= 0 || B > 65535 || npix == 0) { err = "vis_minmax: null argument, or not 1 <= B <= 65535 and npix >= 1"; return 1; }
    if (scratch_bytes < vis_minmax_scratch_bytes(B, npix)) { err = "vis_minmax: scratch too small (soccdpt_vis_minmax_scratch_bytes)"; return 1; }
    const size_t blocks = minmax_blocks(npix);
    float* part = static_cast<float*>(scratch);
    SOCCDPT_LAUNCH(vis_minmax_partial_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, st, x, npix, part);
    SOCCDPT_LAUNCH(vis_minmax_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, part, (int)blocks, minmax);
    return check_launch("vis_minmax", err);
}

int launch_vis_colorize(const float* x, const float* minmax, const uint8_t* lut, int B, int H, int W, uint8_t* dst, const VisDst& d, hipStream_t st,
                        std::string& err) {
    if (!x || !minmax || !lut || !dst) { err = "vis_colorize: null argument"; return 1; }
    if (!image_ok(B, H, W, "vis_colorize", err) || !dst_ok(B, H, W, d, "vis_colorize", err)) return 1;
    SOCCDPT_LAUNCH(vis_colorize_kernel, image_grid(B, H, W), dim3(256), 0, st, x, minmax, lut, H, W, dst, d);
    return check_launch("vis_colorize", err);
}

int launch_vis_color_masks(const float* seg, int B, int C, int H, int W, int channels_last, const uint8_t* class_colors, uint8_t* dst, const VisDst& d,
                           hipStream_t st, std::string& err) {
    if (!seg || !class_colors || !dst || C < 1) { err = "vis_color_masks: null argument or C < 1"; return 1; }
    if (!image_ok(B, H, W, "vis_color_masks", err) || !dst_ok(B, H, W, d, "vis_color_masks", err)) return 1;
    SOCCDPT_LAUNCH(vis_color_masks_kernel, image_grid(B, H, W), dim3(256), 0, st, seg, C, H, W, channels_last ? 1 : 0, class_colors, dst, d);
    return check_launch("vis_color_masks", err);
}

int vis_resize_taps(int src, int dst, int32_t* taps, std::string& err) {
    if (src <= 0 || dst <= 0 || !taps) { err = "vis_resize_taps: null table or a size below 1"; return 1; }
    const double scale = (double)src / (double)dst;
    for (int i = 0; i < dst; ++i) {
        double f = ((double)i + 0.5) * scale - 0.5;
        int i0 = (int)std::floor(f);
        f -= (double)i0;
        if (i0 < 0) { i0 = 0; f = 0.0; }
        if (i0 >= src - 1) { i0 = src - 1; f = 0.0; }
        taps[3 * i] = i0;
        taps[3 * i + 1] = i0 + 1 < src ? i0 + 1 : src - 1;
        taps[3 * i + 2] = (int32_t)std::nearbyint(f * 2048.0);   // round half to even, as numpy's rint
    }
    return 0;
}

int launch_vis_resize(const uint8_t* src, int B, int Hs, int Ws, const int32_t* ytaps, const int32_t* xtaps, int Hd, int Wd, uint8_t* dst, const VisDst& d,
                      hipStream_t st, std::string& err) {
    if (!src || !dst) { err = "vis_resize: null argument"; return 1; }
    if (!image_ok(B, Hs, Ws, "vis_resize", err) || !image_ok(B, Hd, Wd, "vis_resize", err) || !dst_ok(B, Hd, Wd, d, "vis_resize", err)) return 1;
    if (Hs == Hd && Ws == Wd) {   // every tap has weight 2048 on the pixel itself
        SOCCDPT_LAUNCH(vis_copy_kernel, image_grid(B, Hd, Wd), dim3(256), 0, st, src, Hd, Wd, dst, d);
        return check_launch("vis_resize", err);
    }
    if (!ytaps || !xtaps) { err = "vis_resize: the row and column tap tables are needed when the sizes differ"; return 1; }
    SOCCDPT_LAUNCH(vis_resize_kernel, image_grid(B, Hd, Wd), dim3(256), 0, st, src, Hs, Ws, ytaps, xtaps, Hd, Wd, dst, d);
    return check_launch("vis_resize", err);
}

void vis_half_size(int H, int W, int* Hd, int* Wd) {
    // round-half-even of n / 2: n = 2k -> k; n = 2k + 1 -> k + 0.5 -> the even one of k, k + 1
    auto half = [](int n) { const int k = n >> 1; return (n & 1) ? k + (k & 1) : k; };
    *Hd = half(H);
    *Wd = half(W);
}

int launch_vis_shrink_half(const uint8_t* src, int B, int H, int W, int swap_rb, uint8_t* dst, hipStream_t st, std::string& err) {
    if (!src || !dst) { err = "vis_shrink_half: null argument"; return 1; }
    if (!image_ok(B, H, W, "vis_shrink_half", err)) return 1;
    int Hd, Wd;
    vis_half_size(H, W, &Hd, &Wd);
    if (Hd < 1 || Wd < 1) { err = "vis_shrink_half: the half-size image is empty (H and W must be at least 2)"; return 1; }
    SOCCDPT_LAUNCH(vis_shrink_half_kernel, image_grid(B, Hd, Wd), dim3(256), 0, st, src, H, W, Hd, Wd, swap_rb ? 1 : 0, dst);
    return check_launch("vis_shrink_half", err);
}

}  // namespace soccdpt
