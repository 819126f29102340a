/* Observed space of one camera frame in the occupancy grid, and the 3-D IoU over it: the seventh public header of libsoccdpt_hip.so, beside
 * soccdpt_hip.h (whose ABI version these entry points leave alone: nothing declared there changed).  Kernels: soccdpt_amd/csrc/occ_rays.hip; the
 * per-ray traversal: soccdpt_amd/csrc/occ_rays_core.h (host and device).  Python: soccdpt_amd/utils/occupancy_rays.py.
 *
 * No handle and no scratch: stateless, like soccdpt_occ_* and soccdpt_occ_view_*; both entry points take the HIP stream as their last argument.
 * Return 0 on success; otherwise soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure, naming the entry point.  Bad arguments are
 * refused before any launch: NULL pointers, rows / H / W / step <= 0, rows > 65535, a grid size <= 0 or g0 g1 g2 >= 2^31, C outside 1 .. 8,
 * mask_rows / pred_rows neither 1 nor rows, a non-finite entry of host_camera_to_voxel, of host_intrinsics, of z_near or of max_depth, z_near < 0,
 * fx == 0 or fy == 0.
 *
 * The voxel mask [rows][nvw] of uint32: voxel m = (i0 g1 + i1) g2 + i2 is bit m & 31 of word m >> 5, nvw = ceil(g0 g1 g2 / 32).  One bit per
 * VOXEL: this is not the [g0][g1][g2][C] cell layout of the packed grids (soccdpt_occ_pack), which has C bits per voxel.  With g2 = 32 one word
 * is one (i0, i1) column.  `host_grid` is int32[3] in host memory.
 *
 * soccdpt_occ_rays_observed: depth [rows][H][W] f32 in camera metres -> the voxels the camera saw.  With clear != 0 the rows' nvw words are set to
 *   zero first; otherwise the result is OR-ed onto what is there (like clear_bits of soccdpt_voxelise_frames).  The caster never sets a bit at or
 *   beyond g0 g1 g2.  The result is a set: it does not depend on the order of execution.
 *     host_camera_to_voxel N: 3 x 4 row-major float64, camera metres -> continuous voxel coordinates in which voxel i covers [i, i + 1) on every
 *       axis: the inverse of the affine map that a voxel_to_camera matrix of soccdpt_occ_view.h describes (that one takes i + 0.5).  The caller
 *       inverts; the library inverts nothing.
 *     host_intrinsics: fx, fy, cx, cy.   z_near >= 0.   max_depth <= 0: no limit.   step >= 1.
 *   Pixels cast: u = step / 2 + a step (column), v = step / 2 + b step (row) with C integer division, for every a, b >= 0 with u < W and v < H.
 *   One ray per cast pixel of every row r, in float64, every operation rounded on its own (no contraction) in this order:
 *     Z = (double)depth[r][v][u];  the ray is skipped unless Z is finite and Z > z_near  (NaN, +-inf, 0 and negatives cast nothing)
 *     if max_depth > 0 and Z > max_depth: Z = max_depth
 *     dx = (u - cx) / fx;  dy = (v - cy) / fy
 *     A = (dx z_near, dy z_near, z_near);  B = (dx Z, dy Z, Z)                          the camera segment
 *     S_a = ((N[4a] A0 + N[4a+1] A1) + N[4a+2] A2) + N[4a+3];  E_a likewise from B;  D_a = E_a - S_a        for a = 0, 1, 2
 *     the ray is skipped unless all of S and D are finite
 *   Clipping to the box [0, g_a] (slab method), t0 = 0, t1 = 1, for a = 0, 1, 2 in turn:
 *     D_a == 0: the ray is skipped unless 0 <= S_a < g_a
 *     else p = (0 - S_a) / D_a, q = (g_a - S_a) / D_a;  t0 = max(t0, min(p, q));  t1 = min(t1, max(p, q))
 *     the ray is skipped unless t0 <= t1
 *   Entry and end voxel: i_a = clamp(floor(S_a + t0 D_a), 0, g_a - 1);  e_a = clamp(floor(S_a + t1 D_a), 0, g_a - 1).
 *   Traversal (Amanatides-Woo), at most g0 + g1 + g2 + 3 rounds:
 *     mark voxel (i0, i1, i2);  stop if i == e
 *     for every axis with D_a != 0: c_a = (b_a - S_a) / D_a with the integer boundary b_a = i_a + 1 if D_a > 0, i_a if D_a < 0 -- computed afresh
 *       from the boundary every round, never accumulated, so its error stays a few ulps whatever the length of the ray
 *     k = the axis with the smallest c_a, the lowest index among equal ones (so at a crossing of two boundaries at once the lower axis steps
 *       first and the voxel in between is marked too: a superset, never a gap);  stop unless c_k <= t1
 *     i_k += 1 if D_k > 0, -= 1 otherwise;  stop if i_k left 0 .. g_k - 1
 *   Every index is checked against the grid before its word is touched; no input, NaN included, can make the loop write outside [rows][nvw].
 *
 * soccdpt_occ_iou_counts_masked: counts [rows][C][4] uint64 = (intersection, union, pred, gt) per class, the contract of soccdpt_occ_iou_counts
 *   (soccdpt_hip.h) over only those cells n of [g0][g1][g2][C] whose voxel n / C is in the row's effective mask
 *     mask[r, or 0 with mask_rows == 1] | (include_gt ? the voxels of gt[r] with any class bit set : nothing).
 *   pred [pred_rows][nwords] and gt [rows][nwords] are packed cell grids, nwords = ceil(nvox C / 32); mask [mask_rows][nvw] is a voxel mask as above;
 *   nvox = g0 g1 g2 < 2^31.  An all-zero mask with include_gt != 0 scores over any-class(gt) alone.  dev_observed, optional (may be NULL): [rows]
 *   uint64, the number of voxels in the effective mask.  Integer sums only.  Bits at or beyond nvox in a mask's last word, and at or beyond nvox C in a
 *   grid's, are ignored. */
#ifndef SOCCDPT_OCC_RAYS_H
#define SOCCDPT_OCC_RAYS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int soccdpt_occ_rays_observed(const float* dev_depth, int rows, int H, int W, const int32_t* host_grid, const double* host_camera_to_voxel,
                              const double* host_intrinsics, double z_near, double max_depth, int step, int clear, uint32_t* dev_mask, void* stream);
int soccdpt_occ_iou_counts_masked(const uint32_t* dev_pred_bits, int pred_rows, const uint32_t* dev_gt_bits, int rows, size_t nvox, int C,
                                  const uint32_t* dev_mask, int mask_rows, int include_gt, uint64_t* dev_counts, uint64_t* dev_observed,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_OCC_RAYS_H */
