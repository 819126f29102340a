// The operand format of the training step's gradient GEMMs.  Host-only (no HIP header): train.h and train_plan.h share it.
#pragma once
#include <cstddef>

namespace soccdpt {

// Format of a gradient GEMM's staged operands.  The values are soccdpt_train_set_amp's codes: Handle::train_amp converts with a cast.
enum class OpFmt : int { F32 = 0, BF16 = 1, F16 = 2, X3 = 3 };   // exact f32, bf16, IEEE fp16, x3 split-fp16 pairs (half16.h: 4 bytes per element)
constexpr bool op_is16(OpFmt f) { return f == OpFmt::BF16 || f == OpFmt::F16; }
constexpr size_t op_size(OpFmt f) { return op_is16(f) ? 2 : 4; }                                      // bytes per element

}  // namespace soccdpt
