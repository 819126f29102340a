// Launchers of occ_view.hip: pictures of the packed semantic occupancy grid (include/soccdpt_occ_view.h) -- column reduction along one grid axis,
// painting of a column map, 2-D IoU of two column maps, and the camera view (z-buffer splat + resolve).  Stateless: no handle, no scratch, explicit stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "visualise.h"

namespace soccdpt {

constexpr int kOccViewMaxRadiusPx = 256;   // upper bound of max_radius_px: a lane visits (2 r + 1)^2 pixels per set bit

int launch_occ_view_columns(const uint32_t* bits, int rows, const int* grid3, int C, int axis, int from_high, uint8_t* top, int32_t* first, int32_t* count,
                            uint8_t* classes, hipStream_t st, std::string& err);
int launch_occ_view_paint(const uint8_t* top, const int32_t* first, int rows, int A, int B, int depth_len, int from_high, const uint8_t* class_colors, int C,
                          const uint8_t* background, int shade, int zoom, int flip_a, int flip_b, int transpose, uint8_t* dst, const VisDst& d,
                          hipStream_t st, std::string& err);
int launch_occ_view_iou2d(const uint8_t* pred_classes, int pred_rows, const uint8_t* gt_classes, int rows, size_t ncol, int C, uint64_t* counts,
                          hipStream_t st, std::string& err);
int launch_occ_view_splat(const uint32_t* bits, int rows, const int* grid3, int C, const double* voxel_to_camera, const double* intrinsics,
                          double half_extent_m, int max_radius_px, double z_near, int H, int W, uint64_t* zbuf, hipStream_t st, std::string& err);
int launch_occ_view_resolve(const uint64_t* zbuf, const uint8_t* frames, int frame_rows, int rows, int H, int W, int C, const uint8_t* class_colors,
                            int alpha, uint8_t* dst, const VisDst& d, hipStream_t st, std::string& err);

}  // namespace soccdpt
