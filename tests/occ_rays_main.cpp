// The per-ray traversal of soccdpt_occ_rays_observed (soccdpt_amd/csrc/occ_rays_core.h) on the CPU: the text the kernel of csrc/occ_rays.hip runs
// one lane per ray, here one ray after the other, built by tests/test_occ_rays_cpu.py with -ffp-contract=off under the address and
// undefined-behaviour sanitizers and run as a child process.
//
//   occ_rays_main <case file> <result file>
// case file:   int32 g0 g1 g2 H W rows step has_init | float64 N[12] fx fy cx cy z_near max_depth | float32 depth[rows][H][W] | uint32 init[rows][nvw]
// result file: uint32 mask[rows][nvw] (init, or zeros, with every voxel a ray entered OR-ed in)
// The mask lives in a vector of exactly rows * nvw words, so a write past a row's end that stays inside the vector would show in the comparison
// with the restatement and one past the vector is an AddressSanitizer report.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../soccdpt_amd/csrc/occ_rays_core.h"

template <class T>
static bool read_n(FILE* f, T* p, size_t n) { return fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: occ_rays_main <case file> <result file>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t h[8];
    double d[18];
    if (!read_n(f, h, 8) || !read_n(f, d, 18)) { fprintf(stderr, "short header\n"); return 2; }
    soccdpt::OccRayCam cam;
    for (int i = 0; i < 12; ++i) cam.N[i] = d[i];
    cam.fx = d[12]; cam.fy = d[13]; cam.cx = d[14]; cam.cy = d[15]; cam.z_near = d[16]; cam.max_depth = d[17];
    cam.g[0] = h[0]; cam.g[1] = h[1]; cam.g[2] = h[2];
    const int H = h[3], W = h[4], rows = h[5], step = h[6];
    const size_t nvox = (size_t)h[0] * h[1] * h[2], nvw = (nvox + 31) / 32;
    std::vector<float> depth((size_t)rows * H * W);
    std::vector<uint32_t> mask((size_t)rows * nvw, 0u);
    if (!read_n(f, depth.data(), depth.size()) || (h[7] && !read_n(f, mask.data(), mask.size()))) { fprintf(stderr, "short body\n"); return 2; }
    fclose(f);
    const int nu = soccdpt::occ_rays_cast_count(W, step), nv = soccdpt::occ_rays_cast_count(H, step);
    long long marked = 0;
    for (int r = 0; r < rows; ++r) {
        uint32_t* row = mask.data() + (size_t)r * nvw;
        for (int b = 0; b < nv; ++b)
            for (int a = 0; a < nu; ++a) {
                const int u = step / 2 + a * step, v = step / 2 + b * step;
                marked += soccdpt::occ_ray_walk(cam, u, v, depth[((size_t)r * H + v) * W + u], [&](uint32_t m) { row[m >> 5] |= 1u << (m & 31); });
            }
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(mask.data(), sizeof(uint32_t), mask.size(), o) != mask.size() || fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    printf("%lld\n", marked);
    return 0;
}
