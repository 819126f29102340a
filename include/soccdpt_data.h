/* Training and evaluation targets of a batch on the GPU: the third public header of libsoccdpt_hip.so, beside soccdpt_hip.h (whose ABI version
 * these entry points leave alone: nothing declared there changed) and soccdpt_vis.h.  Kernels: soccdpt_amd/csrc/batch_targets.hip.  Python:
 * soccdpt_amd/datasets/.
 *
 * No handle: stateless, like soccdpt_vis_*; every entry point takes the HIP stream as its last argument.  Return 0 on success; otherwise
 * soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure; on an argument error nothing was launched or written.
 *
 * soccdpt_data_targets: the colour-coded label frames (and the disparity frames) of a batch -> every target the criterion and the occupancy
 *   evaluation read.
 *     seg      u8 [B][H][W][3], channels as stored; any byte alignment.
 *     colors   u8 [C][3] in device memory, 1 <= C <= 8: colors[c] is the colour of class c.
 *     disp     [B][H][W] of u8 / u16 / f32 (disp_dtype = SOCCDPT_DATA_U8 / _U16 / _F32), aligned to its element; may be NULL.
 *   Outputs, each may be NULL (not wanted); each aligned to its element:
 *     onehot    f32 [B][C][H][W]: plane c is 1.0f where all three stored channels equal colors[c], else 0.0f.  The classes are independent: a colour
 *               listed twice sets both planes (rgb_seg_to_bool, SOccDPT/datasets/bengaluru_driving_dataset.py:67-76).
 *     class_map i32 [B][H][W]: 0, then for c = 0 .. C-1 in order c where the pixel equals colors[c] (the last match wins).  flip != 0 compares
 *               the pixel with channels 0 and 2 exchanged (rgb_seg_to_class, SOccDPT/datasets/bdd_helper.py:10-25, which flips before it compares).
 *               flip affects class_map only.
 *     y_disp    f32 [B][H][W]: the exact conversion of disp (every u8 / u16 value is an f32; f32 is copied bit for bit, NaN payloads included).
 *               Asking for y_disp without disp is an error.
 *     unmatched u64 [B]: the number of pixels of frame b whose stored channels equal no colour of the table (the pixels that are 0 in every
 *               onehot plane).  The entry point zeroes the counters itself on the stream and the kernel adds integers, so the value is exact and the
 *               same on every run.
 *   Errors: C < 1, C > 8, NULL seg or colors, an unknown disp_dtype with disp given, y_disp without disp, B / H / W out of range
 *   (1 <= B <= 65535, H * W <= 2^32), a pointer not aligned to its element.
 *
 * soccdpt_data_resize_u8c1: soccdpt_vis_resize for one-channel u8 images: src [B][Hs][Ws], ytaps [Hd][3] and xtaps [Wd][3] int32 in device
 *   memory (soccdpt_vis_resize_taps) -> dst [B][Hd][Wd] contiguous, integer arithmetic only:
 *   out = (sum over the four taps of p * wx * wy + 2^21) >> 22.  Hs == Hd and Ws == Wd is a copy (the tables may then be NULL).  Tap indices are
 *   clamped to the source and weights to [0, 2048] by the kernel. */
#ifndef SOCCDPT_DATA_H
#define SOCCDPT_DATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOCCDPT_DATA_U8 0
#define SOCCDPT_DATA_U16 1
#define SOCCDPT_DATA_F32 2
#define SOCCDPT_DATA_MAX_CLASSES 8

int soccdpt_data_targets(const uint8_t* dev_seg, const uint8_t* dev_colors, int C, const void* dev_disp, int disp_dtype, int B, int H, int W, int flip,
                         float* dev_onehot, int32_t* dev_class_map, float* dev_y_disp, uint64_t* dev_unmatched, void* stream);
int soccdpt_data_resize_u8c1(const uint8_t* dev_src, int B, int Hs, int Ws, const int32_t* dev_ytaps, const int32_t* dev_xtaps, int Hd, int Wd,
                             uint8_t* dev_dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_DATA_H */
