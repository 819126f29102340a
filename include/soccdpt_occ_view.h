/* Pictures of the packed semantic occupancy grid on the GPU: the sixth public header of libsoccdpt_hip.so, beside soccdpt_hip.h (whose ABI version
 * these entry points leave alone: nothing declared there changed).  Kernels: soccdpt_amd/csrc/occ_view.hip.  Python: soccdpt_amd/utils/occupancy_views.py.
 *
 * No handle and no scratch: stateless, like soccdpt_occ_* and soccdpt_vis_*; every entry point takes the HIP stream as its last argument.  Return 0 on
 * success; otherwise soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure, naming the entry point.  Bad arguments are refused before any launch.
 *
 * Input: the packed grid [rows][nwords] of uint32 in the layout of soccdpt_occ_pack / soccdpt_forward: cell n is the row-major index of
 * [g0][g1][g2][C], its class is n % C, it is bit n & 31 of word n >> 5, nwords = ceil(g0 g1 g2 C / 32).  1 <= rows <= 65535, 1 <= C <= 8, any grid
 * with g0 g1 g2 C < 2^32.  Bits at or beyond g0 g1 g2 C in the last word are ignored.  `host_grid` is int32[3] in host memory.
 *
 * Pictures are u8, 3 interleaved channels, rows top to bottom, written into a destination rectangle exactly as soccdpt_vis_* do (soccdpt_vis.h): pixel
 * (b, y, x) goes to pixel index b * dst_frame_px + dst_offset_px + y * dst_pitch_px + x of a buffer of dst_total_px pixels; the library checks that
 * the rectangle fits, bytes outside it are not touched.  Colours are written in the channel order of the tables handed in.
 *
 * soccdpt_occ_view_columns: reduce the grid along `axis` (0, 1 or 2).  A column is the g[axis] voxels along it; a voxel is occupied when any of its
 *   C class bits is set.  Outputs are [rows][A][B], A and B the sizes of the two remaining axes in ascending order; any of them may be NULL:
 *     first   int32  index along `axis` of the first occupied voxel, scanning from 0 upwards (from_high == 0) or from g[axis] - 1 downwards; -1: empty
 *     top     uint8  the highest class id set at that voxel (the "last matching class wins" rule of soccdpt_vis_color_masks); 255: empty
 *     count   int32  occupied voxels of the column
 *     classes uint8  OR over the column of the voxels' class masks, bit c standing for class c
 * soccdpt_occ_view_paint: top / first [rows][A][B] -> a picture in which one column is a zoom x zoom block: [A zoom][B zoom], or [B zoom][A zoom] with
 *   transpose != 0; flip_a / flip_b reverse that axis of the map first.  Integer arithmetic only:
 *     rank = from_high ? depth_len - 1 - first : first                     (clamped to 0 .. depth_len - 1)
 *     w    = 256 - (shade * rank) / max(depth_len - 1, 1)                  (C integer division; 0 <= shade <= 192)
 *     out  = (class_colors[top][ch] * w + 128) >> 8
 *   An empty column (first < 0, or top >= C) gets host_background[3].  class_colors [C][3] u8 in device memory.  depth_len = g[axis] of the reduction.
 * soccdpt_occ_view_iou2d: two `classes` maps, pred [pred_rows][ncol] (pred_rows 1 or rows) and gt [rows][ncol] -> counts [rows][C][4] uint64 =
 *   (intersection, union, pred, gt) per class: the contract of soccdpt_occ_iou_counts over columns instead of cells.
 * soccdpt_occ_view_splat: the camera view's z-buffer.  zbuf [rows][H][W] uint64 is set to all ones, then for every set bit n of voxel (i0, i1, i2),
 *   in float64, every operation rounded on its own in this order (host_voxel_to_camera M: 3 x 4 row-major, voxel-centre index -> camera metres;
 *   host_intrinsics: fx, fy, cx, cy):
 *     a = i0 + 0.5; b = i1 + 0.5; c = i2 + 0.5
 *     X = ((M[0] a + M[1] b) + M[2] c) + M[3]        Y from M[4..7], Z from M[8..11]
 *     skipped unless Z > z_near
 *     u = floor(((X / Z) fx + cx) + 0.5);  v = floor(((Y / Z) fy + cy) + 0.5)
 *     r = min(max_radius_px, (int)floor((half_extent_m / Z) fx))           (skipped when that floor is negative or NaN; 0 <= max_radius_px <= 256)
 *   every pixel of [u - r, u + r] x [v - r, v + r] inside the frame takes the minimum of its value and ((uint64)bits_of((float)Z) << 32) | n: the nearer
 *   surface wins, at equal f32 depth the lower cell index; the result does not depend on the order of execution.
 * soccdpt_occ_view_resolve: zbuf + frames [frame_rows][H][W][3] u8 (frame_rows 1 or rows; NULL: black) -> the frame pixel where zbuf is all ones,
 *   elsewhere (frame * (256 - alpha) + class_colors[c] * alpha + 128) >> 8 with c = (low 32 bits of the key) % C and 0 <= alpha <= 256. */
#ifndef SOCCDPT_OCC_VIEW_H
#define SOCCDPT_OCC_VIEW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int soccdpt_occ_view_columns(const uint32_t* dev_bits, int rows, const int32_t* host_grid, int C, int axis, int from_high, uint8_t* dev_top,
                             int32_t* dev_first, int32_t* dev_count, uint8_t* dev_classes, void* stream);
int soccdpt_occ_view_paint(const uint8_t* dev_top, const int32_t* dev_first, int rows, int A, int B, int depth_len, int from_high,
                           const uint8_t* dev_class_colors, int C, const uint8_t* host_background, int shade, int zoom, int flip_a, int flip_b,
                           int transpose, uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px,
                           void* stream);
int soccdpt_occ_view_iou2d(const uint8_t* dev_pred_classes, int pred_rows, const uint8_t* dev_gt_classes, int rows, size_t ncol, int C,
                           uint64_t* dev_counts, void* stream);
int soccdpt_occ_view_splat(const uint32_t* dev_bits, int rows, const int32_t* host_grid, int C, const double* host_voxel_to_camera,
                           const double* host_intrinsics, double half_extent_m, int max_radius_px, double z_near, int H, int W, uint64_t* dev_zbuf,
                           void* stream);
int soccdpt_occ_view_resolve(const uint64_t* dev_zbuf, const uint8_t* dev_frames, int frame_rows, int rows, int H, int W, int C,
                             const uint8_t* dev_class_colors, int alpha, uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px,
                             size_t dst_frame_px, size_t dst_total_px, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_OCC_VIEW_H */
