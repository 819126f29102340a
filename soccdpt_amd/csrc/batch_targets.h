// Launchers of batch_targets.hip: the training / evaluation targets of a batch from its uint8 label and disparity frames, and the one-channel form of
// the integer bilinear resize (include/soccdpt_data.h).  Stateless: no handle, no scratch, explicit stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace soccdpt {

int launch_data_targets(const uint8_t* seg, const uint8_t* colors, int C, const void* disp, int disp_dtype, int B, int H, int W, int flip, float* onehot,
                        int32_t* class_map, float* y_disp, unsigned long long* unmatched, hipStream_t st, std::string& err);
int launch_data_resize_u8c1(const uint8_t* src, int B, int Hs, int Ws, const int32_t* ytaps, const int32_t* xtaps, int Hd, int Wd, uint8_t* dst,
                            hipStream_t st, std::string& err);

}  // namespace soccdpt
