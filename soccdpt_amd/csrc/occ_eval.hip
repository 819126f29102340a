// Consumers of the semantic occupancy grid (include/soccdpt_hip.h, "occupancy evaluation"):
//   occupancy_grid_to_points   SOccDPT/utils/__init__.py:532-568     dense grid -> [N,4] (x, y, z, class_id), class-major
//   occupancy_points of the GT SOccDPT/datasets/bdd_helper.py:339-355 the same list from the counting grid (counts >= threshold)
//   iou_3D                     SOccDPT/utils/__init__.py:392,504      "# TODO: Implement" there; a popcount here
// Bit layout (projection.hip occ_expand_kernel): cell n = row-major index of [g0][g1][g2][C], class n % C, bit n & 31 of word n >> 5; bits at or
// beyond ncell in a row's last word are written as 0 by the packer and masked off by the readers.
//
// The coordinates carry a bit-exact contract with numpy: x = f32((double)i / g0 * (double)shape_f32[0]) widened to f64.  a / b * c has no
// contractable add, and this pragma keeps it that way whatever -ffp-contract the file is compiled with.
#pragma clang fp contract(off)
#include "occ_eval.h"

#include "../../include/soccdpt_hip.h"
#include "kernels.h"
#include "launch.h"

namespace soccdpt {

namespace {

constexpr int kWordsPerLane = 4;                       // one 16-byte load
constexpr int kWordsPerBlock = 256 * kWordsPerLane;    // 1024 words = 32,768 cells per workgroup

typedef __attribute__((ext_vector_type(4))) float v4f;
typedef __attribute__((ext_vector_type(4))) uint32_t v4u;

__device__ __forceinline__ bool occ_pred(float v, float thr, int strict) { return strict ? (v > thr) : (v >= thr); }   // NaN: false either way

template <typename T>
struct PackTraits;
template <>
struct PackTraits<float> {
    static constexpr int V = 4;
    static __device__ __forceinline__ uint32_t vec(const float* p, float thr, int strict) {
        const v4f v = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
        return (occ_pred(v.x, thr, strict) ? 1u : 0u) | (occ_pred(v.y, thr, strict) ? 2u : 0u) | (occ_pred(v.z, thr, strict) ? 4u : 0u) |
               (occ_pred(v.w, thr, strict) ? 8u : 0u);
    }
};
template <>
struct PackTraits<int32_t> {
    static constexpr int V = 4;
    static __device__ __forceinline__ uint32_t vec(const int32_t* p, float thr, int strict) {
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
        return (occ_pred((float)(int32_t)v.x, thr, strict) ? 1u : 0u) | (occ_pred((float)(int32_t)v.y, thr, strict) ? 2u : 0u) |
               (occ_pred((float)(int32_t)v.z, thr, strict) ? 4u : 0u) | (occ_pred((float)(int32_t)v.w, thr, strict) ? 8u : 0u);
    }
};
template <>
struct PackTraits<uint8_t> {
    static constexpr int V = 16;
    static __device__ __forceinline__ uint32_t vec(const uint8_t* p, float thr, int strict) {
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(p));
        const uint32_t q[4] = {v.x, v.y, v.z, v.w};
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) m |= (occ_pred((float)((q[i] >> (8 * j)) & 255u), thr, strict) ? 1u : 0u) << (4 * i + j);
        return m;
    }
};

// dense [rows][ncell] -> bits [rows][nwords].  A lane takes V consecutive cells with one 16-byte load, the 32 / V lanes of a word OR their pieces
// together, the first of them stores the word.  Rows whose start is not 16-byte aligned (ncell not a multiple of V) and the last, partial group of
// a row go through guarded element loads.
template <typename T>
__global__ __launch_bounds__(256) void occ_pack_kernel(const T* __restrict__ dense, uint32_t* __restrict__ bits, size_t ncell, size_t nwords, float thr,
                                                        int strict) {
    constexpr int V = PackTraits<T>::V;
    constexpr int LPW = 32 / V;
    const T* row = dense + (size_t)blockIdx.y * ncell;
    uint32_t* out = bits + (size_t)blockIdx.y * nwords;
    const size_t ngroups = nwords * LPW;   // whole words only: the LPW lanes of one word are all inside or all outside the loop
    for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (size_t)gridDim.x * 256) {
        const size_t cell0 = g * V;
        const T* p = row + cell0;
        uint32_t piece = 0;
        if (cell0 + V <= ncell && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            piece = PackTraits<T>::vec(p, thr, strict);
        } else {
            for (int e = 0; e < V; ++e)
                if (cell0 + e < ncell) piece |= (occ_pred((float)p[e], thr, strict) ? 1u : 0u) << e;
        }
        const int sub = (int)(threadIdx.x & (LPW - 1));
        uint32_t word = piece << (sub * V);
#pragma unroll
        for (int o = 1; o < LPW; o <<= 1) word |= __shfl_xor(word, o);
        if (sub == 0) out[g / LPW] = word;
    }
}

// the four words of one lane: words [wi0, wi0 + 4) of a row, zero beyond the row, padding bits of the last word cleared
__device__ __forceinline__ void load_words(const uint32_t* __restrict__ row, size_t nwords, size_t ncell, size_t wi0, uint32_t (&w)[kWordsPerLane]) {
    const uint32_t* p = row + wi0;
    if (wi0 + kWordsPerLane <= nwords && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const v4u v = *reinterpret_cast<const v4u*>(p);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < kWordsPerLane; ++k) w[k] = (wi0 + k < nwords) ? p[k] : 0u;
    }
    const uint32_t tail = (uint32_t)(ncell & 31);
    if (tail) {
        const uint32_t keep = (1u << tail) - 1u;
#pragma unroll
        for (int k = 0; k < kWordsPerLane; ++k)
            if (wi0 + k == nwords - 1) w[k] &= keep;
    }
}

// bits of word `wi` that belong to class c: positions b with (32 wi + b) % C == c.  The pattern of class 0 in a word that starts a period is
// P = {0, C, 2C, ...}; every other (word, class) is P shifted left by first = (c - 32 wi) mod C < C (no wanted bit is shifted out: first + jC < 32
// implies jC < 32).
template <int C>
__device__ __forceinline__ uint32_t class_mask(uint32_t phase, int c) {
    uint32_t P = 0;
#pragma unroll
    for (int b = 0; b < 32; b += C) P |= 1u << b;
    const uint32_t first = ((uint32_t)c + (uint32_t)C - phase) % (uint32_t)C;
    return P << first;
}

template <int C>
__device__ __forceinline__ void class_counts(const uint32_t (&w)[kWordsPerLane], size_t wi0, uint32_t (&cnt)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) cnt[c] = 0;
#pragma unroll
    for (int k = 0; k < kWordsPerLane; ++k) {
        const uint32_t phase = (uint32_t)(((wi0 + k) * 32) % C);
#pragma unroll
        for (int c = 0; c < C; ++c) cnt[c] += __popc(w[k] & class_mask<C>(phase, c));
    }
}

// step 1 of the point list: blk_counts[(r * C + c) * nblk + blk] = set bits of class c in the block's 1024 words of row r
template <int C>
__global__ __launch_bounds__(256) void occ_points_count_kernel(const uint32_t* __restrict__ bits, size_t ncell, size_t nwords, size_t nblk,
                                                                uint32_t* __restrict__ blk_counts) {
    __shared__ uint32_t sh[4][C];
    const size_t r = blockIdx.y, blk = blockIdx.x;
    const size_t wi0 = (blk * 256 + threadIdx.x) * kWordsPerLane;
    uint32_t w[kWordsPerLane], cnt[C];
    load_words(bits + r * nwords, nwords, ncell, wi0, w);
    class_counts<C>(w, wi0, cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        uint32_t v = cnt[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) sh[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < C) blk_counts[(r * C + threadIdx.x) * nblk + blk] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

// step 2: exclusive scan of the n = rows * C * nblk block counts in (row, class, block) order -> offsets[0..n] (offsets[n] = N), the per-row
// per-class counts and N.  One workgroup: n is a few thousand.
__global__ __launch_bounds__(256) void occ_points_scan_kernel(const uint32_t* __restrict__ blk_counts, unsigned long long* offsets, size_t n, int rows_c,
                                                               size_t nblk, long long* __restrict__ counts, long long* __restrict__ total) {
    __shared__ unsigned long long sh[256];
    const size_t per = (n + 255) / 256;
    const size_t lo = threadIdx.x * per < n ? threadIdx.x * per : n;
    const size_t hi = lo + per < n ? lo + per : n;
    unsigned long long s = 0;
    for (size_t i = lo; i < hi; ++i) s += blk_counts[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long run = 0;
        for (int i = 0; i < 256; ++i) {
            const unsigned long long v = sh[i];
            sh[i] = run;
            run += v;
        }
        offsets[n] = run;
        if (total) *total = (long long)run;
    }
    __syncthreads();
    unsigned long long run = sh[threadIdx.x];
    for (size_t i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += blk_counts[i];
    }
    __syncthreads();   // offsets[] written by this workgroup are visible to it from here on
    if (counts)
        for (int rc = threadIdx.x; rc < rows_c; rc += 256) counts[rc] = (long long)(offsets[(size_t)(rc + 1) * nblk] - offsets[(size_t)rc * nblk]);
}

// step 3: every set bit writes its row at offsets[row, class, block] + (set bits of its class in earlier waves, lanes, words and bits of the block).
// All of these are counts of cells with a smaller index, so the list comes out class-major and ascending in the cell index inside a class, the order
// of np.argwhere followed by the per-class filter, without atomics.
template <int C>
__global__ __launch_bounds__(256) void occ_points_write_kernel(const uint32_t* __restrict__ bits, const unsigned long long* __restrict__ offsets, size_t ncell,
                                                                size_t nwords, size_t nblk, uint32_t g1, uint32_t g2, double d0, double d1, double d2,
                                                                double s0, double s1, double s2, unsigned long long capacity, double* __restrict__ points,
                                                                const uint8_t* __restrict__ class_colors, uint8_t* __restrict__ colors) {
    __shared__ uint32_t sh[4][C];
    const size_t r = blockIdx.y, blk = blockIdx.x;
    const size_t wi0 = (blk * 256 + threadIdx.x) * kWordsPerLane;
    uint32_t w[kWordsPerLane], cnt[C];
    load_words(bits + r * nwords, nwords, ncell, wi0, w);
    class_counts<C>(w, wi0, cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t excl[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        uint32_t inc = cnt[c];
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        excl[c] = inc - cnt[c];
        if (lane == 63) sh[wave][c] = inc;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (cnt[c] == 0) continue;
        unsigned long long pos = offsets[(r * C + c) * nblk + blk] + excl[c];
        for (int v = 0; v < wave; ++v) pos += sh[v][c];
#pragma unroll
        for (int k = 0; k < kWordsPerLane; ++k) {
            const size_t wi = wi0 + k;
            uint32_t m = w[k] & class_mask<C>((uint32_t)((wi * 32) % C), c);
            while (m) {
                const uint32_t b = (uint32_t)__builtin_ctz(m);
                m &= m - 1;
                if (pos < capacity) {
                    const uint32_t cell = (uint32_t)((wi * 32 + b) / C);
                    const uint32_t kz = cell % g2, ij = cell / g2;
                    const uint32_t jy = ij % g1, ix = ij / g1;
                    // (indices / grid_size * occupancy_shape).astype(np.float32): int64 / int -> f64, times the f32 shape widened -> f64, rounded once
                    const double x = (double)(float)((double)ix / d0 * s0);
                    const double y = (double)(float)((double)jy / d1 * s1);
                    const double z = (double)(float)((double)kz / d2 * s2);
                    double2* dst = reinterpret_cast<double2*>(points + pos * 4);
                    dst[0] = make_double2(x, y);
                    dst[1] = make_double2(z, (double)c);
                    if (colors) {
                        colors[pos * 3 + 0] = class_colors[c * 3 + 0];
                        colors[pos * 3 + 1] = class_colors[c * 3 + 1];
                        colors[pos * 3 + 2] = class_colors[c * 3 + 2];
                    }
                }
                ++pos;
            }
        }
    }
}

// counts[r][c][4] += {|p & g|, |p | g|, |p|, |g|} over the block's 1024 words; pred_stride 0 broadcasts one predicted grid over the rows
template <int C>
__global__ __launch_bounds__(256) void occ_iou_counts_kernel(const uint32_t* __restrict__ pred, size_t pred_stride, const uint32_t* __restrict__ gt,
                                                              size_t ncell, size_t nwords, unsigned long long* __restrict__ counts) {
    __shared__ uint32_t sh[4][C * 4];
    const size_t r = blockIdx.y;
    const size_t wi0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * kWordsPerLane;
    uint32_t p[kWordsPerLane], g[kWordsPerLane], a[kWordsPerLane], o[kWordsPerLane];
    load_words(pred + r * pred_stride, nwords, ncell, wi0, p);
    load_words(gt + r * nwords, nwords, ncell, wi0, g);
#pragma unroll
    for (int k = 0; k < kWordsPerLane; ++k) {
        a[k] = p[k] & g[k];
        o[k] = p[k] | g[k];
    }
    uint32_t ca[C], co[C], cp[C], cg[C];
    class_counts<C>(a, wi0, ca);
    class_counts<C>(o, wi0, co);
    class_counts<C>(p, wi0, cp);
    class_counts<C>(g, wi0, cg);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        uint32_t v0 = ca[c], v1 = co[c], v2 = cp[c], v3 = cg[c];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            v0 += __shfl_xor(v0, s);
            v1 += __shfl_xor(v1, s);
            v2 += __shfl_xor(v2, s);
            v3 += __shfl_xor(v3, s);
        }
        if (lane == 0) {
            sh[wave][c * 4 + 0] = v0;
            sh[wave][c * 4 + 1] = v1;
            sh[wave][c * 4 + 2] = v2;
            sh[wave][c * 4 + 3] = v3;
        }
    }
    __syncthreads();
    if (threadIdx.x < C * 4) {
        const uint32_t v = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
        if (v) atomicAdd(&counts[r * (C * 4) + threadIdx.x], (unsigned long long)v);   // integer sums: the order does not matter
    }
}

struct Geometry {
    size_t nwords, nblk, n;   // words per row, workgroups per row, scan length
};

bool geometry(int rows, size_t ncell, int C, Geometry& g, const char* what, std::string& err) {
    if (rows <= 0 || rows > 65535 || ncell == 0 || ncell > ((size_t)1 << 32) || C < 1 || C > 8 || ncell % (size_t)C != 0) {
        err = std::string(what) + ": need 1 <= rows <= 65535, 1 <= C <= 8 and ncell a multiple of C, at most 2^32";
        return false;
    }
    g.nwords = (ncell + 31) / 32;
    g.nblk = (g.nwords + kWordsPerBlock - 1) / kWordsPerBlock;
    g.n = (size_t)rows * C * g.nblk;
    return true;
}

size_t offsets_bytes(const Geometry& g) { return (g.n + 1) * sizeof(unsigned long long); }

}  // namespace

#define OCC_DISPATCH_C(C, ...)                   \
    switch (C) {                                 \
        case 1: { constexpr int kC = 1; __VA_ARGS__; } break; \
        case 2: { constexpr int kC = 2; __VA_ARGS__; } break; \
        case 3: { constexpr int kC = 3; __VA_ARGS__; } break; \
        case 4: { constexpr int kC = 4; __VA_ARGS__; } break; \
        case 5: { constexpr int kC = 5; __VA_ARGS__; } break; \
        case 6: { constexpr int kC = 6; __VA_ARGS__; } break; \
        case 7: { constexpr int kC = 7; __VA_ARGS__; } break; \
        default: { constexpr int kC = 8; __VA_ARGS__; } break; \
    }

int launch_occ_pack(const void* dense, int dtype, int rows, size_t ncell, float threshold, int strict, uint32_t* bits, hipStream_t st, std::string& err) {
    if (!dense || !bits || rows <= 0 || rows > 65535 || ncell == 0) { err = "occ_pack: bad argument"; return 1; }
    const size_t nwords = (ncell + 31) / 32;
    const int lanes_per_word = dtype == SOCCDPT_OCC_U8 ? 2 : 8;
    size_t blocks = (nwords * lanes_per_word + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    const dim3 grid((unsigned)blocks, (unsigned)rows);
    switch (dtype) {
        case SOCCDPT_OCC_F32:
            SOCCDPT_LAUNCH(occ_pack_kernel<float>, grid, dim3(256), 0, st, static_cast<const float*>(dense), bits, ncell, nwords, threshold, strict);
            break;
        case SOCCDPT_OCC_U8:
            SOCCDPT_LAUNCH(occ_pack_kernel<uint8_t>, grid, dim3(256), 0, st, static_cast<const uint8_t*>(dense), bits, ncell, nwords, threshold, strict);
            break;
        case SOCCDPT_OCC_I32:
            SOCCDPT_LAUNCH(occ_pack_kernel<int32_t>, grid, dim3(256), 0, st, static_cast<const int32_t*>(dense), bits, ncell, nwords, threshold, strict);
            break;
        default:
            err = "occ_pack: dtype must be SOCCDPT_OCC_F32, SOCCDPT_OCC_U8 or SOCCDPT_OCC_I32";
            return 1;
    }
    return check_launch("occ_pack", err);
}

size_t occ_points_scratch_bytes(int rows, size_t ncell, int C) {
    Geometry g;
    std::string err;
    if (!geometry(rows, ncell, C, g, "occ_points", err)) return 0;
    return offsets_bytes(g) + g.n * sizeof(uint32_t);
}

int launch_occ_points_count(const uint32_t* bits, int rows, size_t ncell, int C, void* scratch, size_t scratch_bytes, int64_t* counts, int64_t* total,
                            hipStream_t st, std::string& err) {
    Geometry g;
    if (!geometry(rows, ncell, C, g, "occ_points_count", err)) return 1;
    if (!bits || !scratch || scratch_bytes < offsets_bytes(g) + g.n * sizeof(uint32_t)) { err = "occ_points_count: null argument or scratch too small"; return 1; }
    unsigned long long* offsets = static_cast<unsigned long long*>(scratch);
    uint32_t* blk_counts = reinterpret_cast<uint32_t*>(static_cast<char*>(scratch) + offsets_bytes(g));
    const dim3 grid((unsigned)g.nblk, (unsigned)rows);
    OCC_DISPATCH_C(C, SOCCDPT_LAUNCH(occ_points_count_kernel<kC>, grid, dim3(256), 0, st, bits, ncell, g.nwords, g.nblk, blk_counts));
    SOCCDPT_LAUNCH(occ_points_scan_kernel, dim3(1), dim3(256), 0, st, blk_counts, offsets, g.n, rows * C, g.nblk, reinterpret_cast<long long*>(counts),
                   reinterpret_cast<long long*>(total));
    return check_launch("occ_points_count", err);
}

int launch_occ_points_write(const uint32_t* bits, int rows, const int* grid3, int C, const float* occ_shape, const void* scratch, size_t scratch_bytes,
                            size_t capacity, double* points, const uint8_t* class_colors, uint8_t* colors, hipStream_t st, std::string& err) {
    if (!grid3 || !occ_shape || grid3[0] <= 0 || grid3[1] <= 0 || grid3[2] <= 0) { err = "occ_points_write: bad grid"; return 1; }
    const size_t ncell = (size_t)grid3[0] * grid3[1] * grid3[2] * (size_t)(C > 0 ? C : 1);
    Geometry g;
    if (!geometry(rows, ncell, C, g, "occ_points_write", err)) return 1;
    if (!bits || !scratch || scratch_bytes < offsets_bytes(g) + g.n * sizeof(uint32_t)) { err = "occ_points_write: null argument or scratch too small"; return 1; }
    if ((colors != nullptr) != (class_colors != nullptr)) { err = "occ_points_write: colours need both the [C][3] table and the output"; return 1; }
    if (capacity == 0) return 0;
    if (!points) { err = "occ_points_write: null output"; return 1; }
    const unsigned long long* offsets = static_cast<const unsigned long long*>(scratch);
    const dim3 grid((unsigned)g.nblk, (unsigned)rows);
    OCC_DISPATCH_C(C, SOCCDPT_LAUNCH(occ_points_write_kernel<kC>, grid, dim3(256), 0, st, bits, offsets, ncell, g.nwords, g.nblk, (uint32_t)grid3[1],
                                     (uint32_t)grid3[2], (double)grid3[0], (double)grid3[1], (double)grid3[2], (double)occ_shape[0], (double)occ_shape[1],
                                     (double)occ_shape[2], (unsigned long long)capacity, points, class_colors, colors));
    return check_launch("occ_points_write", err);
}

int launch_occ_iou_counts(const uint32_t* pred_bits, int pred_rows, const uint32_t* gt_bits, int rows, size_t ncell, int C, uint64_t* counts,
                          hipStream_t st, std::string& err) {
    Geometry g;
    if (!geometry(rows, ncell, C, g, "occ_iou_counts", err)) return 1;
    if (!pred_bits || !gt_bits || !counts || (pred_rows != 1 && pred_rows != rows)) { err = "occ_iou_counts: null argument, or pred_rows is neither 1 nor rows"; return 1; }
    if (hipMemsetAsync(counts, 0, (size_t)rows * C * 4 * sizeof(uint64_t), st) != hipSuccess) { err = "occ_iou_counts: memset failed"; return 1; }
    const dim3 grid((unsigned)g.nblk, (unsigned)rows);
    const size_t pred_stride = pred_rows == 1 ? 0 : g.nwords;
    OCC_DISPATCH_C(C, SOCCDPT_LAUNCH(occ_iou_counts_kernel<kC>, grid, dim3(256), 0, st, pred_bits, pred_stride, gt_bits, ncell, g.nwords,
                                     reinterpret_cast<unsigned long long*>(counts)));
    return check_launch("occ_iou_counts", err);
}

}  // namespace soccdpt
