// Launchers of occ_eval.hip: consumers of the semantic occupancy grid (pack a dense grid to bits, packed bits -> the reference's ordered
// point list, per-class intersection / union counts of two packed grids).  Stateless: no handle, explicit scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace soccdpt {

// dtype of the dense grid handed to launch_occ_pack (SOCCDPT_OCC_F32 / _U8 / _I32 of include/soccdpt_hip.h)
int launch_occ_pack(const void* dense, int dtype, int rows, size_t ncell, float threshold, int strict, uint32_t* bits, hipStream_t st, std::string& err);

size_t occ_points_scratch_bytes(int rows, size_t ncell, int C);
int launch_occ_points_count(const uint32_t* bits, int rows, size_t ncell, int C, void* scratch, size_t scratch_bytes, int64_t* counts, int64_t* total,
                            hipStream_t st, std::string& err);
int launch_occ_points_write(const uint32_t* bits, int rows, const int* grid, int C, const float* occ_shape, const void* scratch, size_t scratch_bytes,
                            size_t capacity, double* points, const uint8_t* class_colors, uint8_t* colors, hipStream_t st, std::string& err);

int launch_occ_iou_counts(const uint32_t* pred_bits, int pred_rows, const uint32_t* gt_bits, int rows, size_t ncell, int C, uint64_t* counts,
                          hipStream_t st, std::string& err);

}  // namespace soccdpt
