// Launchers of visualise.hip: the evaluation pictures (include/soccdpt_vis.h) -- per-frame min / max, inverse depth -> colour map, class maps ->
// class colours, integer bilinear resize and the half-size shrink of u8 x 3 images.  Stateless: no handle, explicit scratch (min / max only), explicit stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace soccdpt {

// Where a kernel writes its [B][H][W][3] u8 result inside a larger image buffer: pixel (b, y, x) goes to pixel index
// b * frame_px + offset_px + y * pitch_px + x of a buffer of total_px pixels.  A plain [B][H][W][3] destination is {W, 0, H * W, B * H * W}.
struct VisDst {
    size_t pitch_px, offset_px, frame_px, total_px;
};

// the two argument checks every picture launcher makes (also occ_view.hip's): the image sizes, and that the destination rectangle fits its buffer
bool vis_image_ok(int B, int H, int W, const char* what, std::string& err);
bool vis_dst_ok(int B, int H, int W, const VisDst& d, const char* what, std::string& err);

size_t vis_minmax_scratch_bytes(int B, size_t npix);
int launch_vis_minmax(const float* x, int B, size_t npix, float* minmax, void* scratch, size_t scratch_bytes, hipStream_t st, std::string& err);
int launch_vis_colorize(const float* x, const float* minmax, const uint8_t* lut, int B, int H, int W, uint8_t* dst, const VisDst& d, hipStream_t st,
                        std::string& err);
int launch_vis_color_masks(const float* seg, int B, int C, int H, int W, int channels_last, const uint8_t* class_colors, uint8_t* dst, const VisDst& d,
                           hipStream_t st, std::string& err);
// host: taps[dst][3] = {i0, i1, w1} of one axis of the resize (w0 = 2048 - w1)
int vis_resize_taps(int src, int dst, int32_t* taps, std::string& err);
int launch_vis_resize(const uint8_t* src, int B, int Hs, int Ws, const int32_t* ytaps, const int32_t* xtaps, int Hd, int Wd, uint8_t* dst, const VisDst& d,
                      hipStream_t st, std::string& err);
void vis_half_size(int H, int W, int* Hd, int* Wd);
int launch_vis_shrink_half(const uint8_t* src, int B, int H, int W, int swap_rb, uint8_t* dst, hipStream_t st, std::string& err);

}  // namespace soccdpt
