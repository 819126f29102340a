// The targets of a training / evaluation batch from its uint8 frames (include/soccdpt_data.h):
//   rgb_seg_to_bool    SOccDPT/datasets/bengaluru_driving_dataset.py:67-76   colour-coded labels -> one 0 / 1 plane per class
//   rgb_seg_to_class   SOccDPT/datasets/bdd_helper.py:10-25                  colour-coded labels -> class ids (compares the channel-flipped pixel)
//   torch.tensor(disparity_frame)                                            u8 / u16 / f32 disparity -> f32
//   cv2.resize of a one-channel u8 image                                     the integer bilinear of visualise.hip, one channel
// One streaming pass: 3 bytes of labels (+ 1, 2 or 4 of disparity) read per pixel, 4 * (C + 2) written.  A lane owns 4 consecutive pixels of a frame:
// three 4-byte loads of the labels and one 16-byte store per output plane when the addresses allow it, guarded element accesses otherwise (a frame
// whose pixel count is no multiple of 4, a frame stride or a base pointer that is not aligned).  Nothing on the data path goes through LDS or an atomic;
// the counters of `unmatched` take one integer add per workgroup that saw an unmatched pixel (four words of LDS to get there), and the grid is capped
// so that a batch issues about two thousand of them: every add of a frame lands on one address, and 8,100 per frame (one per wave of an uncapped
// grid at 1080p, B = 8) made the launch take 785 us against 57 us without the counters (profiles/batch_targets_cost.json, `unmatched_first_form`).
//
// Nothing here multiplies and adds floats (the conversions are exact, the resize is integer arithmetic); the pragma keeps it that way whatever
// -ffp-contract the file is compiled with.
#pragma clang fp contract(off)
#include "batch_targets.h"

#include "../../include/soccdpt_data.h"
#include "kernels.h"
#include "launch.h"

namespace soccdpt {

namespace {

typedef __attribute__((ext_vector_type(4))) float v4f;
typedef __attribute__((ext_vector_type(4))) uint32_t v4u;
typedef __attribute__((ext_vector_type(2))) uint32_t v2u;

constexpr int kPx = 4;             // pixels per lane
constexpr unsigned kMaxBlocks = 2048;   // per launch, shared among the frames; the rest of a frame is walked with a grid stride

// the n <= 4 pixels at p as 24-bit keys (stored channel k in bits 8k .. 8k+7); pixels past n read as 0
__device__ __forceinline__ void load_keys(const uint8_t* __restrict__ p, int n, uint32_t (&key)[kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        const uint32_t w0 = __builtin_nontemporal_load(q), w1 = __builtin_nontemporal_load(q + 1), w2 = __builtin_nontemporal_load(q + 2);
        key[0] = w0 & 0xffffffu;
        key[1] = (w0 >> 24) | ((w1 & 0xffffu) << 8);
        key[2] = (w1 >> 16) | ((w2 & 0xffu) << 16);
        key[3] = w2 >> 8;
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            key[j] = j < n ? ((uint32_t)p[3 * j] | ((uint32_t)p[3 * j + 1] << 8) | ((uint32_t)p[3 * j + 2] << 16)) : 0u;
    }
}

// 4 words to p (n of them valid): one 16-byte store when whole and aligned
__device__ __forceinline__ void store_w4(uint32_t* __restrict__ p, int n, const uint32_t (&w)[kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        __builtin_nontemporal_store(v4u{w[0], w[1], w[2], w[3]}, reinterpret_cast<v4u*>(p));   // written once, read by a later launch
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (j < n) p[j] = w[j];
    }
}

__device__ __forceinline__ uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }

// the n <= 4 disparity values at element index i of `disp` as f32 bit patterns: u8 / u16 widened exactly, f32 copied bit for bit
template <int kDtype>
__device__ __forceinline__ void load_disp(const void* __restrict__ disp, size_t i, int n, uint32_t (&w)[kPx]) {
    if (kDtype == SOCCDPT_DATA_U8) {
        const uint8_t* p = static_cast<const uint8_t*>(disp) + i;
        if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            const uint32_t u = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
#pragma unroll
            for (int j = 0; j < kPx; ++j) w[j] = f32_bits((float)((u >> (8 * j)) & 255u));
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j) w[j] = j < n ? f32_bits((float)p[j]) : 0u;
        }
    } else if (kDtype == SOCCDPT_DATA_U16) {
        const uint16_t* p = static_cast<const uint16_t*>(disp) + i;
        if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
            const v2u u = __builtin_nontemporal_load(reinterpret_cast<const v2u*>(p));
            w[0] = f32_bits((float)(u.x & 0xffffu)); w[1] = f32_bits((float)(u.x >> 16));
            w[2] = f32_bits((float)(u.y & 0xffffu)); w[3] = f32_bits((float)(u.y >> 16));
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j) w[j] = j < n ? f32_bits((float)p[j]) : 0u;
        }
    } else {
        const uint32_t* p = static_cast<const uint32_t*>(disp) + i;   // moved as words: no float instruction touches a NaN's payload
        if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const v4u u = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
            w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j) w[j] = j < n ? p[j] : 0u;
        }
    }
}

// kDtype: SOCCDPT_DATA_* of disp, -1 when there is no disparity to convert.  Every array below is indexed by unrolled constants only (registers, no
// private-segment scratch); the class loop reads colors[c] with wave-uniform addresses.
template <int kDtype>
__global__ __launch_bounds__(256) void data_targets_kernel(const uint8_t* __restrict__ seg, const uint8_t* __restrict__ colors, int C,
                                                            const void* __restrict__ disp, size_t npix, int flip, float* __restrict__ onehot,
                                                            int32_t* __restrict__ class_map, float* __restrict__ y_disp,
                                                            unsigned long long* __restrict__ unmatched) {
    const size_t b = blockIdx.y;
    const size_t ngroups = (npix + kPx - 1) / kPx;
    uint32_t miss = 0;   // pixels of this lane that equal no colour
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t p0 = g * kPx;
        const int n = npix - p0 < (size_t)kPx ? (int)(npix - p0) : kPx;
        uint32_t key[kPx], cmp[kPx], cls[kPx], hit[kPx];
        load_keys(seg + 3 * (b * npix + p0), n, key);
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
            cmp[j] = flip ? (((key[j] & 0xffu) << 16) | (key[j] & 0xff00u) | (key[j] >> 16)) : key[j];   // what the class map compares
            cls[j] = 0;
            hit[j] = 0;
        }
        for (int c = 0; c < C; ++c) {
            const uint32_t ck = (uint32_t)colors[3 * c] | ((uint32_t)colors[3 * c + 1] << 8) | ((uint32_t)colors[3 * c + 2] << 16);
            uint32_t one[kPx];
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                const bool m = key[j] == ck;
                one[j] = m ? 0x3f800000u : 0u;   // 1.0f / 0.0f
                hit[j] |= m ? 1u : 0u;
                if (cmp[j] == ck) cls[j] = (uint32_t)c;
            }
            if (onehot) store_w4(reinterpret_cast<uint32_t*>(onehot) + (b * (size_t)C + (size_t)c) * npix + p0, n, one);
        }
        if (class_map) store_w4(reinterpret_cast<uint32_t*>(class_map) + b * npix + p0, n, cls);
        if (kDtype >= 0 && y_disp) {
            uint32_t w[kPx];
            load_disp<(kDtype < 0 ? 0 : kDtype)>(disp, b * npix + p0, n, w);
            store_w4(reinterpret_cast<uint32_t*>(y_disp) + b * npix + p0, n, w);
        }
#pragma unroll
        for (int j = 0; j < kPx; ++j) miss += (j < n && !hit[j]) ? 1u : 0u;
    }
    if (unmatched) {   // uniform over the workgroup: every lane is here
        __shared__ uint32_t wave_miss[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) miss += __shfl_xor(miss, o);
        if ((threadIdx.x & 63) == 0) wave_miss[threadIdx.x >> 6] = miss;
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = wave_miss[0] + wave_miss[1] + wave_miss[2] + wave_miss[3];
            if (total) atomicAdd(unmatched + b, (unsigned long long)total);
        }
    }
}

// taps [len][3] = {i0, i1, w1}; the indices are clamped here as well, so a bad table cannot make the kernel read outside the source
__device__ __forceinline__ void read_taps(const int32_t* __restrict__ taps, int i, int src_len, int& i0, int& i1, uint32_t& w0, uint32_t& w1) {
    const int a = taps[3 * i], c = taps[3 * i + 1], w = taps[3 * i + 2];
    i0 = a < 0 ? 0 : (a > src_len - 1 ? src_len - 1 : a);
    i1 = c < 0 ? 0 : (c > src_len - 1 ? src_len - 1 : c);
    w1 = (uint32_t)(w < 0 ? 0 : (w > 2048 ? 2048 : w));
    w0 = 2048u - w1;
}

__device__ __forceinline__ void store_b4(uint8_t* __restrict__ p, int n, const uint8_t (&c)[kPx]) {
    if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < kPx; ++j)
            if (j < n) p[j] = c[j];
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

__global__ __launch_bounds__(256) void data_copy_u8c1_kernel(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst) {
    int y, x0, n;
    if (!lane_pixels(H, W, y, x0, n)) return;
    const size_t at = ((size_t)blockIdx.y * H + y) * W + x0;
    uint8_t c[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) c[j] = j < n ? src[at + j] : (uint8_t)0;
    store_b4(dst + at, n, c);
}

// out = (sum over the four taps of p * wx * wy + 2^21) >> 22, wx + wx' = wy + wy' = 2048: at most 255 * 2^22 + 2^21 < 2^31 (visualise.hip, one channel)
__global__ __launch_bounds__(256) void data_resize_u8c1_kernel(const uint8_t* __restrict__ src, int Hs, int Ws, const int32_t* __restrict__ ytaps,
                                                                const int32_t* __restrict__ xtaps, int Hd, int Wd, uint8_t* __restrict__ dst) {
    int y, x0, n;
    if (!lane_pixels(Hd, Wd, y, x0, n)) return;
    const size_t b = blockIdx.y;
    int ya, yb;
    uint32_t wy0, wy1;
    read_taps(ytaps, y, Hs, ya, yb, wy0, wy1);
    const uint8_t* ra = src + (b * Hs + ya) * (size_t)Ws;
    const uint8_t* rb = src + (b * Hs + yb) * (size_t)Ws;
    uint8_t c[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        int xa = 0, xb = 0;
        uint32_t wx0 = 2048u, wx1 = 0u;
        if (j < n) read_taps(xtaps, x0 + j, Ws, xa, xb, wx0, wx1);
        const uint32_t s = (uint32_t)ra[xa] * wx0 * wy0 + (uint32_t)ra[xb] * wx1 * wy0 + (uint32_t)rb[xa] * wx0 * wy1 + (uint32_t)rb[xb] * wx1 * wy1;
        c[j] = (uint8_t)((s + (1u << 21)) >> 22);
    }
    store_b4(dst + (b * Hd + y) * (size_t)Wd + x0, n, c);
}

bool image_ok(int B, int H, int W, const char* what, std::string& err) {
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24) || (size_t)H * (size_t)W > ((size_t)1 << 32)) {
        err = std::string(what) + ": need 1 <= B <= 65535, 1 <= H, W <= 2^24 and H * W <= 2^32";
        return false;
    }
    return true;
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int launch_data_targets(const uint8_t* seg, const uint8_t* colors, int C, const void* disp, int disp_dtype, int B, int H, int W, int flip, float* onehot,
                        int32_t* class_map, float* y_disp, unsigned long long* unmatched, hipStream_t st, std::string& err) {
    if (C < 1 || C > SOCCDPT_DATA_MAX_CLASSES) { err = "data_targets: need 1 <= C <= 8 classes"; return 1; }
    if (!seg || !colors) { err = "data_targets: null seg or colors"; return 1; }
    if (!image_ok(B, H, W, "data_targets", err)) return 1;
    if (y_disp && !disp) { err = "data_targets: y_disp requested without disp"; return 1; }
    if (disp && disp_dtype != SOCCDPT_DATA_U8 && disp_dtype != SOCCDPT_DATA_U16 && disp_dtype != SOCCDPT_DATA_F32) {
        err = "data_targets: unknown disp_dtype (SOCCDPT_DATA_U8, _U16 or _F32)";
        return 1;
    }
    const size_t disp_elem = disp_dtype == SOCCDPT_DATA_U8 ? 1 : (disp_dtype == SOCCDPT_DATA_U16 ? 2 : 4);
    if (!aligned(onehot, 4) || !aligned(class_map, 4) || !aligned(y_disp, 4) || !aligned(unmatched, 8) || (disp && !aligned(disp, disp_elem))) {
        err = "data_targets: a pointer is not aligned to its element type";
        return 1;
    }
    const size_t npix = (size_t)H * (size_t)W;
    if (unmatched && hipMemsetAsync(unmatched, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess) {
        (void)hipGetLastError();
        err = "data_targets: clearing the unmatched counters failed";
        return 1;
    }
    const size_t blocks = ((npix + kPx - 1) / kPx + 255) / 256;
    const size_t cap = kMaxBlocks / (unsigned)B > 0 ? kMaxBlocks / (unsigned)B : 1;   // per frame
    const dim3 grid((unsigned)(blocks > cap ? cap : blocks), (unsigned)B);
    const int dt = (disp && y_disp) ? disp_dtype : -1;
#define SOCCDPT_DATA_TARGETS(DT) \
    SOCCDPT_LAUNCH(data_targets_kernel<DT>, grid, dim3(256), 0, st, seg, colors, C, disp, npix, flip ? 1 : 0, onehot, class_map, y_disp, unmatched)
    switch (dt) {
        case SOCCDPT_DATA_U8: SOCCDPT_DATA_TARGETS(SOCCDPT_DATA_U8); break;
        case SOCCDPT_DATA_U16: SOCCDPT_DATA_TARGETS(SOCCDPT_DATA_U16); break;
        case SOCCDPT_DATA_F32: SOCCDPT_DATA_TARGETS(SOCCDPT_DATA_F32); break;
        default: SOCCDPT_DATA_TARGETS(-1); break;
    }
#undef SOCCDPT_DATA_TARGETS
    return check_launch("data_targets", err);
}

int launch_data_resize_u8c1(const uint8_t* src, int B, int Hs, int Ws, const int32_t* ytaps, const int32_t* xtaps, int Hd, int Wd, uint8_t* dst,
                            hipStream_t st, std::string& err) {
    if (!src || !dst) { err = "data_resize_u8c1: null argument"; return 1; }
    if (!image_ok(B, Hs, Ws, "data_resize_u8c1", err) || !image_ok(B, Hd, Wd, "data_resize_u8c1", err)) return 1;
    const size_t lanes = (size_t)Hd * (((size_t)Wd + kPx - 1) / kPx);
    const dim3 grid((unsigned)((lanes + 255) / 256), (unsigned)B);
    if (Hs == Hd && Ws == Wd) {   // every tap has weight 2048 on the pixel itself
        SOCCDPT_LAUNCH(data_copy_u8c1_kernel, grid, dim3(256), 0, st, src, Hd, Wd, dst);
        return check_launch("data_resize_u8c1", err);
    }
    if (!ytaps || !xtaps) { err = "data_resize_u8c1: the row and column tap tables are needed when the sizes differ"; return 1; }
    SOCCDPT_LAUNCH(data_resize_u8c1_kernel, grid, dim3(256), 0, st, src, Hs, Ws, ytaps, xtaps, Hd, Wd, dst);
    return check_launch("data_resize_u8c1", err);
}

}  // namespace soccdpt
