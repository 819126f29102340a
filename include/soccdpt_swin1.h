/* Kernel-level entries of the Swin-V1 block (dpt_swin_large_384, SOCCDPT_BACKBONE_SWINL12_384): the fifth public header of libsoccdpt_hip.so, beside
 * soccdpt_hip.h (whose ABI version and prototypes these entry points leave alone), soccdpt_vis.h, soccdpt_data.h and soccdpt_pack.h.  Kernels:
 * soccdpt_amd/csrc/swin1.hip.  For tests: the forward of the model launches the same kernels itself.
 *
 * No handle, no allocation, no synchronisation; every entry point takes the HIP stream as its last argument.  Return 0 on success; otherwise
 * soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure, and on such a refusal nothing was launched or written.  Every device pointer is
 * 16-byte aligned.  Formats are the SOCCDPT_PREC_* of soccdpt_hip.h: _BF16 and _F16 = 2 bytes per element, _F32 = 4, _F16X3 = the x3 pair layout (4).
 *
 * soccdpt_swin1_window_attention: timm WindowAttention.forward of Swin-V1 with roll / partition / mask / reverse folded in.
 *   qkv [B*res*res][3*heads*32] -> out [B*res*res][heads*32]; per (window, head) softmax(q k^T 32^-0.5 + table[index(q, k)] + mask) v, where
 *   dev_table is relative_position_bias_table [(2 ws - 1)^2][heads] f32, index(q, k) = (rq - rk + ws - 1) (2 ws - 1) + (cq - ck + ws - 1), and mask is
 *   -100 between the regions of the last window row / column when shift != 0.  dev_bias_scratch: heads * 5 * 5 * 1024 floats (the table in accumulator
 *   order).  precision = element type of qkv and out: _BF16 / _F16 (16-bit kernels), _F32, _F16X3 (f32 qkv in, x3 operand out).  out_x3 != 0
 *   (precision == _F16 only): fp16 qkv in, x3 operand out.  Refused: a null pointer, B / res / heads <= 0, ws != 12, res % ws != 0, shift other than
 *   0 or ws / 2.
 * soccdpt_swin1_ln_rows: out[row] = LayerNorm(xf[row]) * g + beta over C in out_format; xf [rows][C] f32 is read and not written.
 *   C = 192, 384, 768 or 1536; rows > 0; eps > 0; out must not be xf.
 * soccdpt_swin1_merge_ln: PatchMerging up to its reduction.  xf [B][R][R][C] f32 -> out [B*(R/2)^2][4C] in out_format: row (b, y, x) is
 *   LayerNorm over 4C of cat(xf[b][2y][2x], xf[b][2y+1][2x], xf[b][2y][2x+1], xf[b][2y+1][2x+1]) * g + beta (g, beta [4C]).  R even; C = 192, 384 or 768. */
#ifndef SOCCDPT_SWIN1_H
#define SOCCDPT_SWIN1_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int soccdpt_swin1_window_attention(const void* dev_qkv, const float* dev_table, void* dev_out, float* dev_bias_scratch, int B, int res, int ws, int shift,
                                   int heads, int precision, int out_x3, void* stream);
int soccdpt_swin1_ln_rows(const float* dev_xf, const float* dev_g, const float* dev_beta, void* dev_out, int out_format, int rows, int C, float eps,
                          void* stream);
int soccdpt_swin1_merge_ln(const float* dev_xf, const float* dev_g, const float* dev_beta, void* dev_out, int out_format, int B, int R, int C, float eps,
                           void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_SWIN1_H */
