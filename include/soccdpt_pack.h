/* Targets of a batch from palette-indexed label frames: the fourth public header of libsoccdpt_hip.so, beside soccdpt_hip.h (whose ABI version these
 * entry points leave alone: nothing declared there changed), soccdpt_vis.h and soccdpt_data.h.  Kernels: soccdpt_amd/csrc/frame_pack.hip.  Python:
 * soccdpt_amd/datasets/frame_pack.py (the file format).
 *
 * No handle: stateless, like soccdpt_data_*; every entry point takes the HIP stream as its last argument.  Return 0 on success; otherwise
 * soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure; on an argument error nothing was launched or written.
 *
 * Packed labels: a frame of H * W pixels is a record of words_per_frame >= ceil(H * W * k / 32) little-endian 32-bit words, k in {1, 2, 4, 8}.
 *   Pixel p (row-major) occupies bits [(p * k) mod 32, + k) of word floor(p * k / 32); its value is an index into palette u8 [P][3], 1 <= P <= 2^k,
 *   whose rows are label colours with the channels as soccdpt_data_targets reads them in seg.  dev_idx holds B consecutive records and is 4-byte
 *   aligned.  An index >= P is read as P - 1: nothing outside the palette is ever read.
 *
 * soccdpt_pack_targets: what soccdpt_data_targets writes for the label frames seg[b][p] = palette[min(idx[b][p], P - 1)], bit for bit, without those
 *   frames ever existing: the same colors, disp / disp_dtype, flip and the same four nullable outputs with the same layouts and rules (onehot planes
 *   independent, class_map last match wins and alone follows flip, y_disp exact with NaN payloads kept, unmatched zeroed on the stream and exact).
 *   Errors: k not 1, 2, 4 or 8; P < 1 or P > 2^k; words_per_frame < ceil(H * W * k / 32); NULL or misaligned dev_idx; NULL palette; and everything
 *   soccdpt_data_targets refuses (C, colors, disp_dtype, y_disp without disp, B / H / W out of range, a pointer not aligned to its element).
 *
 * soccdpt_pack_expand: the label frames themselves, dst u8 [B][H][W][3] = palette[min(idx, P - 1)], any byte alignment: for label frames stored at
 *   another size than the one the targets are wanted at (expand -> soccdpt_vis_resize -> soccdpt_data_targets). */
#ifndef SOCCDPT_PACK_H
#define SOCCDPT_PACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int soccdpt_pack_targets(const uint32_t* dev_idx, int k, size_t words_per_frame, const uint8_t* dev_palette, int P, const uint8_t* dev_colors, int C,
                         const void* dev_disp, int disp_dtype, int B, int H, int W, int flip, float* dev_onehot, int32_t* dev_class_map,
                         float* dev_y_disp, uint64_t* dev_unmatched, void* stream);
int soccdpt_pack_expand(const uint32_t* dev_idx, int k, size_t words_per_frame, const uint8_t* dev_palette, int P, int B, int H, int W,
                        uint8_t* dev_dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_PACK_H */
