// Launchers of occ_rays.hip: the observed-space voxel mask of a depth map by ray casting, and the 3-D IoU counts over a voxel mask
// (include/soccdpt_occ_rays.h).  Stateless: no handle, no scratch, explicit stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace soccdpt {

int launch_occ_rays_observed(const float* depth, int rows, int H, int W, const int* grid3, const double* camera_to_voxel, const double* intrinsics,
                             double z_near, double max_depth, int step, int clear, uint32_t* mask, hipStream_t st, std::string& err);
int launch_occ_iou_counts_masked(const uint32_t* pred_bits, int pred_rows, const uint32_t* gt_bits, int rows, size_t nvox, int C, const uint32_t* mask,
                                 int mask_rows, int include_gt, uint64_t* counts, uint64_t* observed, hipStream_t st, std::string& err);

}  // namespace soccdpt
