// The targets of a batch from PALETTE-INDEXED label frames (include/soccdpt_pack.h; the file format is soccdpt_amd/datasets/frame_pack.py, DESIGN.md
// section 12.4).  A stored label frame holds a handful of colours, so a frame pack keeps k = 1, 2, 4 or 8 bits per pixel and the palette u8 [P][3];
// soccdpt_pack_targets writes what soccdpt_data_targets (batch_targets.hip) writes for the frames the indices stand for, bit for bit, reading
// k / 8 bytes of labels per pixel instead of 3.
//
// What a palette entry means for the outputs does not depend on the pixel, so it is worked out once per workgroup: the first P lanes compare their
// entry with the C class colours and leave {plane mask, class id, hit} as one word in LDS (at most 256 words).  The pixel loop is then a shift, a
// mask, a clamp and one LDS read per pixel.  Everything after that is batch_targets.hip's: a lane owns 4 consecutive pixels (4 * k bits, which never
// straddle a word because the group starts at a multiple of 4 pixels), one 16-byte non-temporal store per output plane when the address allows it and
// guarded element stores otherwise, a grid capped at 2048 workgroups walked with a grid stride, one integer add per workgroup for `unmatched`.
// The store / disparity helpers are restated here rather than shared through a header: batch_targets.hip keeps them in its unnamed namespace, and a
// new header in this directory would rebuild every object of the library (the Makefile's header wildcard).
//
// No float arithmetic anywhere (conversions are exact); the pragma keeps it that way whatever -ffp-contract the file is compiled with.
#pragma clang fp contract(off)
#include "../../include/soccdpt_pack.h"

#include "../../include/soccdpt_data.h"
#include "kernels.h"
#include "launch.h"

namespace soccdpt {

void set_last_error(const std::string& msg);   // what soccdpt_last_error(NULL) returns (capi.cpp)

namespace {

typedef __attribute__((ext_vector_type(4))) uint32_t v4u;
typedef __attribute__((ext_vector_type(2))) uint32_t v2u;

constexpr int kPx = 4;                  // pixels per lane
constexpr unsigned kMaxBlocks = 2048;   // per launch, shared among the frames; the rest of a frame is walked with a grid stride
constexpr int kMaxPalette = 256;

// a palette entry resolved against the class colours
constexpr uint32_t kHitBit = 1u << 16;   // bits 0 .. 7: plane c is set; bits 8 .. 15: class id; bit 16: equals some colour

__device__ __forceinline__ uint32_t key24(const uint8_t* __restrict__ p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

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

// The (clamped) palette indices of the 4 pixels that start at pixel p0 of a record, p0 a multiple of 4: the 4 * kBits bits at bit p0 * kBits, all in
// one word.  Pixels past the frame's end read the record's zero padding or its last real word; the caller ignores them.
template <int kBits>
__device__ __forceinline__ void load_indices(const uint32_t* __restrict__ rec, size_t p0, uint32_t last, uint32_t (&v)[kPx]) {
    const size_t bit = p0 * kBits;
    const uint32_t word = rec[bit >> 5] >> (uint32_t)(bit & 31);   // neighbouring lanes share the word (k < 8): left to the cache
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        const uint32_t x = (word >> (kBits * j)) & ((1u << kBits) - 1u);
        v[j] = x < last ? x : last;
    }
}

// kDtype: SOCCDPT_DATA_* of disp, -1 when there is no disparity to convert.  Every array below is indexed by unrolled constants only (registers, no
// private-segment scratch).
template <int kBits, int kDtype>
__global__ __launch_bounds__(256) void pack_targets_kernel(const uint32_t* __restrict__ idx, size_t words_per_frame, const uint8_t* __restrict__ palette,
                                                            int P, const uint8_t* __restrict__ colors, int C, const void* __restrict__ disp, size_t npix,
                                                            int flip, float* __restrict__ onehot, int32_t* __restrict__ class_map,
                                                            float* __restrict__ y_disp, unsigned long long* __restrict__ unmatched) {
    __shared__ uint32_t entry[kMaxPalette];
    __shared__ uint32_t wave_miss[4];
    if ((int)threadIdx.x < P) {   // P <= 256 = the workgroup's size (checked by the launcher)
        const uint32_t key = key24(palette + 3 * threadIdx.x);
        const uint32_t cmp = flip ? (((key & 0xffu) << 16) | (key & 0xff00u) | (key >> 16)) : key;   // what the class map compares
        uint32_t planes = 0, cls = 0;
        for (int c = 0; c < C; ++c) {
            const uint32_t ck = key24(colors + 3 * c);
            if (key == ck) planes |= 1u << c;
            if (cmp == ck) cls = (uint32_t)c;   // the last match wins
        }
        entry[threadIdx.x] = planes | (cls << 8) | (planes ? kHitBit : 0u);
    }
    __syncthreads();
    const size_t b = blockIdx.y;
    const uint32_t* rec = idx + b * words_per_frame;
    const uint32_t last = (uint32_t)P - 1u;
    const size_t ngroups = (npix + kPx - 1) / kPx;
    uint32_t miss = 0;   // pixels of this lane that equal no colour
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t p0 = g * kPx;
        const int n = npix - p0 < (size_t)kPx ? (int)(npix - p0) : kPx;
        uint32_t v[kPx], e[kPx];
        load_indices<kBits>(rec, p0, last, v);
#pragma unroll
        for (int j = 0; j < kPx; ++j) e[j] = entry[v[j]];
        if (onehot) {
            for (int c = 0; c < C; ++c) {
                uint32_t one[kPx];
#pragma unroll
                for (int j = 0; j < kPx; ++j) one[j] = ((e[j] >> c) & 1u) ? 0x3f800000u : 0u;   // 1.0f / 0.0f
                store_w4(reinterpret_cast<uint32_t*>(onehot) + (b * (size_t)C + (size_t)c) * npix + p0, n, one);
            }
        }
        if (class_map) {
            uint32_t cls[kPx];
#pragma unroll
            for (int j = 0; j < kPx; ++j) cls[j] = (e[j] >> 8) & 0xffu;
            store_w4(reinterpret_cast<uint32_t*>(class_map) + b * npix + p0, n, cls);
        }
        if (kDtype >= 0 && y_disp) {
            uint32_t w[kPx];
            load_disp<(kDtype < 0 ? 0 : kDtype)>(disp, b * npix + p0, n, w);
            store_w4(reinterpret_cast<uint32_t*>(y_disp) + b * npix + p0, n, w);
        }
#pragma unroll
        for (int j = 0; j < kPx; ++j) miss += (j < n && !(e[j] & kHitBit)) ? 1u : 0u;
    }
    if (unmatched) {   // uniform over the workgroup: every lane is here
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

// dst u8 [B][npix][3] = palette[min(idx, P - 1)]: a lane writes its 4 pixels as three words when whole and aligned, as bytes otherwise
template <int kBits>
__global__ __launch_bounds__(256) void pack_expand_kernel(const uint32_t* __restrict__ idx, size_t words_per_frame, const uint8_t* __restrict__ palette,
                                                           int P, size_t npix, uint8_t* __restrict__ dst) {
    __shared__ uint32_t color[kMaxPalette];
    if ((int)threadIdx.x < P) color[threadIdx.x] = key24(palette + 3 * threadIdx.x);
    __syncthreads();
    const size_t b = blockIdx.y;
    const uint32_t* rec = idx + b * words_per_frame;
    const uint32_t last = (uint32_t)P - 1u;
    const size_t ngroups = (npix + kPx - 1) / kPx;
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t p0 = g * kPx;
        const int n = npix - p0 < (size_t)kPx ? (int)(npix - p0) : kPx;
        uint32_t v[kPx], key[kPx];
        load_indices<kBits>(rec, p0, last, v);
#pragma unroll
        for (int j = 0; j < kPx; ++j) key[j] = color[v[j]];
        uint8_t* p = dst + 3 * (b * npix + p0);
        if (n >= kPx && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
            uint32_t* q = reinterpret_cast<uint32_t*>(p);
            __builtin_nontemporal_store(key[0] | (key[1] << 24), q);
            __builtin_nontemporal_store((key[1] >> 8) | (key[2] << 16), q + 1);
            __builtin_nontemporal_store((key[2] >> 16) | (key[3] << 8), q + 2);
        } else {
#pragma unroll
            for (int j = 0; j < kPx; ++j)
                if (j < n) {
                    p[3 * j] = (uint8_t)key[j];
                    p[3 * j + 1] = (uint8_t)(key[j] >> 8);
                    p[3 * j + 2] = (uint8_t)(key[j] >> 16);
                }
        }
    }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the checks the two entry points share; false with err set
bool packed_ok(const char* what, const uint32_t* idx, int k, size_t words_per_frame, const uint8_t* palette, int P, int B, int H, int W, std::string& err) {
    const std::string w(what);
    if (k != 1 && k != 2 && k != 4 && k != 8) { err = w + ": k (bits per index) must be 1, 2, 4 or 8"; return false; }
    if (P < 1 || P > (1 << k)) { err = w + ": need 1 <= P <= 2^k palette entries"; return false; }
    if (!idx || !palette) { err = w + ": null idx or palette"; return false; }
    if (!aligned(idx, 4)) { err = w + ": idx is not aligned to 4 bytes"; return false; }
    if (B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > (1 << 24) || W > (1 << 24) || (size_t)H * (size_t)W > ((size_t)1 << 32)) {
        err = w + ": need 1 <= B <= 65535, 1 <= H, W <= 2^24 and H * W <= 2^32";
        return false;
    }
    const size_t need = ((size_t)H * (size_t)W * (size_t)k + 31) / 32;
    if (words_per_frame < need) { err = w + ": words_per_frame is smaller than ceil(H * W * k / 32)"; return false; }
    return true;
}

dim3 capped_grid(size_t npix, int B) {
    const size_t blocks = ((npix + kPx - 1) / kPx + 255) / 256;
    const size_t cap = kMaxBlocks / (unsigned)B > 0 ? kMaxBlocks / (unsigned)B : 1;   // per frame
    return dim3((unsigned)(blocks > cap ? cap : blocks), (unsigned)B);
}

int launch_pack_targets(const uint32_t* idx, int k, size_t words_per_frame, const uint8_t* palette, int P, const uint8_t* colors, int C, const void* disp,
                        int disp_dtype, int B, int H, int W, int flip, float* onehot, int32_t* class_map, float* y_disp, unsigned long long* unmatched,
                        hipStream_t st, std::string& err) {
    if (C < 1 || C > SOCCDPT_DATA_MAX_CLASSES) { err = "pack_targets: need 1 <= C <= 8 classes"; return 1; }
    if (!colors) { err = "pack_targets: null colors"; return 1; }
    if (!packed_ok("pack_targets", idx, k, words_per_frame, palette, P, B, H, W, err)) return 1;
    if (y_disp && !disp) { err = "pack_targets: y_disp requested without disp"; return 1; }
    if (disp && disp_dtype != SOCCDPT_DATA_U8 && disp_dtype != SOCCDPT_DATA_U16 && disp_dtype != SOCCDPT_DATA_F32) {
        err = "pack_targets: unknown disp_dtype (SOCCDPT_DATA_U8, _U16 or _F32)";
        return 1;
    }
    const size_t disp_elem = disp_dtype == SOCCDPT_DATA_U8 ? 1 : (disp_dtype == SOCCDPT_DATA_U16 ? 2 : 4);
    if (!aligned(onehot, 4) || !aligned(class_map, 4) || !aligned(y_disp, 4) || !aligned(unmatched, 8) || (disp && !aligned(disp, disp_elem))) {
        err = "pack_targets: a pointer is not aligned to its element type";
        return 1;
    }
    const size_t npix = (size_t)H * (size_t)W;
    if (unmatched && hipMemsetAsync(unmatched, 0, (size_t)B * sizeof(unsigned long long), st) != hipSuccess) {
        (void)hipGetLastError();
        err = "pack_targets: clearing the unmatched counters failed";
        return 1;
    }
    const dim3 grid = capped_grid(npix, B);
    const int dt = (disp && y_disp) ? disp_dtype : -1;
#define SOCCDPT_PACK_TARGETS(K, DT)                                                                                                                 \
    SOCCDPT_LAUNCH((pack_targets_kernel<K, DT>), grid, dim3(256), 0, st, idx, words_per_frame, palette, P, colors, C, disp, npix, flip ? 1 : 0, onehot, \
                   class_map, y_disp, unmatched)
#define SOCCDPT_PACK_TARGETS_K(K)                                                        \
    switch (dt) {                                                                        \
        case SOCCDPT_DATA_U8: SOCCDPT_PACK_TARGETS(K, SOCCDPT_DATA_U8); break;           \
        case SOCCDPT_DATA_U16: SOCCDPT_PACK_TARGETS(K, SOCCDPT_DATA_U16); break;         \
        case SOCCDPT_DATA_F32: SOCCDPT_PACK_TARGETS(K, SOCCDPT_DATA_F32); break;         \
        default: SOCCDPT_PACK_TARGETS(K, -1); break;                                     \
    }
    switch (k) {
        case 1: SOCCDPT_PACK_TARGETS_K(1); break;
        case 2: SOCCDPT_PACK_TARGETS_K(2); break;
        case 4: SOCCDPT_PACK_TARGETS_K(4); break;
        default: SOCCDPT_PACK_TARGETS_K(8); break;
    }
#undef SOCCDPT_PACK_TARGETS_K
#undef SOCCDPT_PACK_TARGETS
    return check_launch("pack_targets", err);
}

int launch_pack_expand(const uint32_t* idx, int k, size_t words_per_frame, const uint8_t* palette, int P, int B, int H, int W, uint8_t* dst, hipStream_t st,
                       std::string& err) {
    if (!packed_ok("pack_expand", idx, k, words_per_frame, palette, P, B, H, W, err)) return 1;
    if (!dst) { err = "pack_expand: null dst"; return 1; }
    const size_t npix = (size_t)H * (size_t)W;
    const dim3 grid = capped_grid(npix, B);
#define SOCCDPT_PACK_EXPAND(K) SOCCDPT_LAUNCH((pack_expand_kernel<K>), grid, dim3(256), 0, st, idx, words_per_frame, palette, P, npix, dst)
    switch (k) {
        case 1: SOCCDPT_PACK_EXPAND(1); break;
        case 2: SOCCDPT_PACK_EXPAND(2); break;
        case 4: SOCCDPT_PACK_EXPAND(4); break;
        default: SOCCDPT_PACK_EXPAND(8); break;
    }
#undef SOCCDPT_PACK_EXPAND
    return check_launch("pack_expand", err);
}

int failed(const std::string& err) {
    set_last_error("soccdpt_" + err);
    return 1;
}

}  // namespace

}  // namespace soccdpt

extern "C" {

int soccdpt_pack_targets(const uint32_t* dev_idx, int k, size_t words_per_frame, const uint8_t* dev_palette, int P, const uint8_t* dev_colors, int C,
                         const void* dev_disp, int disp_dtype, int B, int H, int W, int flip, float* dev_onehot, int32_t* dev_class_map,
                         float* dev_y_disp, uint64_t* dev_unmatched, void* stream) {
    std::string err;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the unmatched counters are 64-bit");
    if (soccdpt::launch_pack_targets(dev_idx, k, words_per_frame, dev_palette, P, dev_colors, C, dev_disp, disp_dtype, B, H, W, flip, dev_onehot,
                                     dev_class_map, dev_y_disp, reinterpret_cast<unsigned long long*>(dev_unmatched), (hipStream_t)stream, err))
        return soccdpt::failed(err);
    return 0;
}

int soccdpt_pack_expand(const uint32_t* dev_idx, int k, size_t words_per_frame, const uint8_t* dev_palette, int P, int B, int H, int W, uint8_t* dev_dst,
                        void* stream) {
    std::string err;
    if (soccdpt::launch_pack_expand(dev_idx, k, words_per_frame, dev_palette, P, B, H, W, dev_dst, (hipStream_t)stream, err)) return soccdpt::failed(err);
    return 0;
}

}  // extern "C"
