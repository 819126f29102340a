/* Evaluation pictures on the GPU: the second public header of libsoccdpt_hip.so, beside soccdpt_hip.h (whose ABI version these entry points
 * leave alone: nothing declared there changed).  Kernels: soccdpt_amd/csrc/visualise.hip.  Python: soccdpt_amd/utils/visualise.py.
 *
 * No handle: stateless, like soccdpt_occ_* and soccdpt_metrics_*; scratch (soccdpt_vis_minmax only) is the caller's; every launching entry point
 * takes the HIP stream as its last argument.  Return 0 on success; otherwise soccdpt_last_error(NULL) of soccdpt_hip.h describes the failure.
 *
 * Images are u8, 3 interleaved channels, rows top to bottom.  The kernels do not interpret the channel order: the colour map is written in
 * the order of the table handed in (B, G, R in the Python layer, as cv2.applyColorMap returns it), class colours as they are given.
 *
 * Destination rectangle.  soccdpt_vis_colorize, _color_masks and _resize write a [B][H][W][3] result into a larger buffer of dst_total_px pixels:
 * pixel (b, y, x) goes to pixel index  b * dst_frame_px + dst_offset_px + y * dst_pitch_px + x.  A plain contiguous destination is
 * (pitch, offset, frame, total) = (W, 0, H * W, B * H * W); a tile of a panel of width PW whose top-left corner is (py, px) is
 * (PW, py * PW + px, ., PH * PW).  The library checks that the rectangle fits the buffer; bytes outside it are not touched.
 *
 * soccdpt_vis_minmax: x [B][npix] f32 -> minmax [B][2] f32 = {min, max} over the FINITE values of each row ({+inf, -inf} when a row has none;
 *   -0 is reported as +0).  `scratch` = soccdpt_vis_minmax_scratch_bytes(B, npix) bytes of device memory (0: bad arguments), free again when the
 *   call's work on the stream is done.
 * soccdpt_vis_colorize: x [B][H][W] f32, minmax [B][2], lut [256][3] u8 -> lut[idx] per pixel, idx = (uint8)(v * 255.0f) truncated with
 *   v = (x - min_b) / (max_b - min_b) in f32 (one subtract, one IEEE divide, one multiply: numpy's ((d - min) / (max - min) * 255).astype(np.uint8),
 *   SOccDPT/utils/__init__.py:649-655).  idx = 0 where that expression is undefined: a non-finite pixel, or max_b <= min_b.
 * soccdpt_vis_color_masks: seg [B][C][H][W] f32 (channels_last == 0) or [B][H][W][C] (channels_last != 0), class_colors [C][3] u8, any C >= 1 ->
 *   zeros, then for c = 0 .. C-1 class_colors[c] where seg > 0.5 (the last matching class wins; 0.5 itself and NaN do not match):
 *   color_segmentation of SOccDPT/utils/__init__.py:35-43.
 * soccdpt_vis_resize_taps (host only, no GPU work): the tap table of one axis of the bilinear resize, taps [dst][3] int32 = {i0, i1, w1}:
 *   f = (i + 0.5) * src / dst - 0.5 in double precision, i0 = floor(f), w1 = round-half-even((f - i0) * 2048); i0 < 0 -> (0, w1 = 0),
 *   i0 >= src - 1 -> (src - 1, w1 = 0); i1 = min(i0 + 1, src - 1).  w0 = 2048 - w1.
 * soccdpt_vis_resize: src [B][Hs][Ws][3] u8, ytaps [Hd][3] and xtaps [Wd][3] int32 in device memory -> [B][Hd][Wd][3], integer arithmetic only:
 *   out = (sum over the four taps of p * wx * wy + 2^21) >> 22.  Hs == Hd and Ws == Wd is a copy (the tables may then be NULL).  Tap indices
 *   are clamped to the source and weights to [0, 2048] by the kernel.
 * soccdpt_vis_half_size: the size soccdpt_vis_shrink_half writes: round-half-even(H / 2), round-half-even(W / 2).
 * soccdpt_vis_shrink_half: src [B][H][W][3] u8 -> dst [B][Hd][Wd][3] (both contiguous), out = (a + b + c + d + 2) >> 2 over source rows 2y, 2y+1 and
 *   columns 2x, 2x+1, each clamped to the last row / column; swap_rb != 0 also exchanges channels 0 and 2 (BGR -> RGB).  H, W >= 2. */
#ifndef SOCCDPT_VIS_H
#define SOCCDPT_VIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t soccdpt_vis_minmax_scratch_bytes(int B, size_t npix);
int soccdpt_vis_minmax(const float* dev_x, int B, size_t npix, float* dev_minmax, void* dev_scratch, size_t scratch_bytes, void* stream);
int soccdpt_vis_colorize(const float* dev_x, const float* dev_minmax, const uint8_t* dev_lut, int B, int H, int W, uint8_t* dev_dst,
                         size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream);
int soccdpt_vis_color_masks(const float* dev_seg, int B, int C, int H, int W, int channels_last, const uint8_t* dev_class_colors, uint8_t* dev_dst,
                            size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream);
int soccdpt_vis_resize_taps(int src, int dst, int32_t* host_taps);
int soccdpt_vis_resize(const uint8_t* dev_src, int B, int Hs, int Ws, const int32_t* dev_ytaps, const int32_t* dev_xtaps, int Hd, int Wd,
                       uint8_t* dev_dst, size_t dst_pitch_px, size_t dst_offset_px, size_t dst_frame_px, size_t dst_total_px, void* stream);
int soccdpt_vis_half_size(int H, int W, int32_t* Hd, int32_t* Wd);
int soccdpt_vis_shrink_half(const uint8_t* dev_src, int B, int H, int W, int swap_rb, uint8_t* dev_dst, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SOCCDPT_VIS_H */
