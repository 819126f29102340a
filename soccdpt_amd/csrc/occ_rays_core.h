// One ray of soccdpt_occ_rays_observed (include/soccdpt_occ_rays.h), for the host and the device: occ_rays.hip runs it one lane per cast pixel,
// tests/occ_rays_main.cpp runs the same text on the CPU under the sanitizers.  Nothing here touches memory: every voxel entered goes to
// `sink(m)` with m = (i0 g1 + i1) g2 + i2, already checked against the grid.
//
// The contract is bit-exact in float64: every product, sum and quotient below is rounded on its own, in the order the header writes them.  The
// pragma turns contraction off for whatever includes this file, whichever -ffp-contract it is compiled with.
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCC_RAYS_HD __host__ __device__ __forceinline__
#else
#define OCC_RAYS_HD inline
#endif

namespace soccdpt {

struct OccRayCam {
    double N[12], fx, fy, cx, cy, z_near, max_depth;   // camera metres -> continuous voxel coordinates; intrinsics; max_depth <= 0: none
    int g[3];                                            // g0 g1 g2 < 2^31
};

// number of cast pixels along an axis of `len` pixels: those a >= 0 with step / 2 + a * step < len
OCC_RAYS_HD int occ_rays_cast_count(int len, int step) {
    const int first = step / 2;
    return len > first ? (len - first + step - 1) / step : 0;
}

// floor(x) as an index of 0 .. n - 1; anything below (NaN included) gives 0, anything above n - 1
OCC_RAYS_HD int occ_rays_clamp_floor(double x, int n) {
    const double f = floor(x);
    if (!(f >= 0.0)) return 0;
    if (f > (double)(n - 1)) return n - 1;
    return (int)f;
}

// The ray of pixel (u, v) with the measured depth `depth`.  Returns the number of voxels handed to the sink.
template <class Sink>
OCC_RAYS_HD int occ_ray_walk(const OccRayCam& cam, int u, int v, float depth, Sink&& sink) {
    double Z = (double)depth;
    if (!(Z - Z == 0.0) || !(Z > cam.z_near)) return 0;   // Z - Z is NaN for NaN and +-inf
    if (cam.max_depth > 0.0 && Z > cam.max_depth) Z = cam.max_depth;
    const double dx = ((double)u - cam.cx) / cam.fx;
    const double dy = ((double)v - cam.cy) / cam.fy;
    const double A0 = dx * cam.z_near, A1 = dy * cam.z_near, A2 = cam.z_near;
    const double B0 = dx * Z, B1 = dy * Z, B2 = Z;
    double S[3], D[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double* n = cam.N + 4 * a;
        S[a] = ((n[0] * A0 + n[1] * A1) + n[2] * A2) + n[3];
        const double E = ((n[0] * B0 + n[1] * B1) + n[2] * B2) + n[3];
        D[a] = E - S[a];
        if (!(S[a] - S[a] == 0.0) || !(D[a] - D[a] == 0.0)) return 0;
    }
    double t0 = 0.0, t1 = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double ga = (double)cam.g[a];
        if (D[a] == 0.0) {
            if (!(S[a] >= 0.0 && S[a] < ga)) return 0;
        } else {
            const double p = (0.0 - S[a]) / D[a], q = (ga - S[a]) / D[a];
            const double lo = p < q ? p : q, hi = p < q ? q : p;
            if (lo > t0) t0 = lo;
            if (hi < t1) t1 = hi;
        }
        if (!(t0 <= t1)) return 0;
    }
    int i[3], e[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        i[a] = occ_rays_clamp_floor(S[a] + t0 * D[a], cam.g[a]);
        e[a] = occ_rays_clamp_floor(S[a] + t1 * D[a], cam.g[a]);
    }
    const int trips = cam.g[0] + cam.g[1] + cam.g[2] + 3;
    int marked = 0;
    for (int trip = 0; trip < trips; ++trip) {
        if (i[0] < 0 || i[0] >= cam.g[0] || i[1] < 0 || i[1] >= cam.g[1] || i[2] < 0 || i[2] >= cam.g[2]) break;
        sink((uint32_t)(((int64_t)i[0] * cam.g[1] + i[1]) * cam.g[2] + i[2]));
        ++marked;
        if (i[0] == e[0] && i[1] == e[1] && i[2] == e[2]) break;
        int k = -1;
        double ck = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (D[a] == 0.0) continue;
            const double b = D[a] > 0.0 ? (double)(i[a] + 1) : (double)i[a];
            const double c = (b - S[a]) / D[a];
            if (k < 0 || c < ck) { k = a; ck = c; }
        }
        if (k < 0 || !(ck <= t1)) break;
#pragma unroll
        for (int a = 0; a < 3; ++a)   // (no indexing by k: the three indices stay in registers)
            if (a == k) i[a] += D[a] > 0.0 ? 1 : -1;
    }
    return marked;
}

}  // namespace soccdpt
