"""The reference's evaluation pictures on the GPU (csrc/visualise.hip, include/soccdpt_vis.h):

  colorize_disparity   ((d - min) / (max - min) * 255).astype(np.uint8) -> cv2.applyColorMap(.., COLORMAP_PLASMA)   SOccDPT/utils/__init__.py:649-655
  color_segmentation   SOccDPT/utils/__init__.py:35-43 (same name and arguments); color_masks is its batched [B,C,H,W] form
  resize_bgr           cv2.resize(img, (W, H)), bilinear
  shrink_half          cv2.resize(img, (0, 0), fx=0.5, fy=0.5), with cv2.cvtColor(img, cv2.COLOR_BGR2RGB) folded in
  evaluation_panel     the `plot` image of evaluate (utils/__init__.py:627-708) and evaluate_occupancy (:410-460)
  write_png            cv2.imwrite(path.png, img) with the standard library only

Every picture is a u8 [..,H,W,3] cuda tensor.  Inverse depth, class maps and ground truth are already device tensors at camera resolution; the
reference pulls each to the host, normalises with numpy, colours with cv2 and concatenates.  Here the tiles are coloured straight into the panel
buffer and that buffer is read once by the shrink.  There is no CPU fallback: a CPU tensor raises RuntimeError like the rest of the product path.

The colour table is matplotlib's plasma (plasma_lut.py, written by tools/make_plasma_lut.py), which OpenCV documents COLORMAP_PLASMA to be; cv2 is
not a dependency, so byte parity with cv2.applyColorMap itself is not pinned."""
from __future__ import annotations

import ctypes
import struct
import zlib
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..lib import _call, _ptr, load_library
from .occupancy import class_color_table
from .plasma_lut import PLASMA_BGR_HEX

PLASMA_BGR = np.frombuffer(bytes.fromhex(PLASMA_BGR_HEX), dtype=np.uint8).reshape(256, 3)      # LUT[i] = (B, G, R)

_lut_on = {}


def _need_cuda(t, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what}: the visualisation kernels run on the GPU only; pass a cuda tensor (there is no CPU fallback)")


def _lut(device: torch.device) -> torch.Tensor:
    key = (device.type, device.index)
    if key not in _lut_on:
        _lut_on[key] = torch.from_numpy(PLASMA_BGR.copy()).to(device)
    return _lut_on[key]


class _Rect:
    """Where a [B,H,W,3] result goes inside a destination buffer (include/soccdpt_vis.h, destination rectangle)."""

    def __init__(self, buf: torch.Tensor, pitch: int, offset: int, frame: int):
        assert buf.dtype == torch.uint8 and buf.is_contiguous() and buf.numel() % 3 == 0
        self.buf, self.args = buf, (int(pitch), int(offset), int(frame), buf.numel() // 3)

    @staticmethod
    def whole(B: int, H: int, W: int, device) -> "_Rect":
        return _Rect(torch.empty((B, H, W, 3), dtype=torch.uint8, device=device), W, 0, H * W)

    @staticmethod
    def tile(panel: torch.Tensor, row: int, col: int) -> "_Rect":
        """The rectangle of a [PH,PW,3] panel whose top-left pixel is (row, col)."""
        return _Rect(panel, panel.shape[1], row * panel.shape[1] + col, panel.shape[0] * panel.shape[1])


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def disparity_minmax(disp: torch.Tensor) -> torch.Tensor:
    """[B,H,W] (cuda) -> [B,2] f32: min and max over the finite values of each frame."""
    _need_cuda(disp, "disparity_minmax")
    d = _f32(disp)
    B = d.shape[0]
    npix = d.numel() // B
    out = torch.empty((B, 2), dtype=torch.float32, device=d.device)
    nscratch = load_library().soccdpt_vis_minmax_scratch_bytes(B, npix)
    if nscratch == 0:
        raise ValueError("disparity_minmax: need 1 <= B <= 65535 non-empty frames")
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=d.device)
    _call("soccdpt_vis_minmax", _ptr(d), B, npix, _ptr(out), _ptr(scratch), nscratch, device=d.device)
    return out


def _colorize_into(disp: torch.Tensor, rect: _Rect) -> None:
    d = _f32(disp)
    B, H, W = d.shape
    mm = disparity_minmax(d)
    _call("soccdpt_vis_colorize", _ptr(d), _ptr(mm), _ptr(_lut(d.device)), B, H, W, _ptr(rect.buf), *rect.args, device=d.device)


def colorize_disparity(disp: torch.Tensor) -> torch.Tensor:
    """[H,W] or [B,H,W] (cuda) -> u8 [..,H,W,3] BGR: every frame normalised by its own min and max, index (uint8)(v * 255) truncated into the plasma
    table.  Index 0 where the reference's expression is undefined: a non-finite pixel (which takes no part in the min / max either), or max == min."""
    _need_cuda(disp, "colorize_disparity")
    if disp.dim() not in (2, 3):
        raise ValueError("colorize_disparity: expected [H,W] or [B,H,W]")
    d = disp if disp.dim() == 3 else disp.unsqueeze(0)
    rect = _Rect.whole(d.shape[0], d.shape[1], d.shape[2], d.device)
    _colorize_into(d, rect)
    return rect.buf if disp.dim() == 3 else rect.buf[0]


def _masks_into(seg: torch.Tensor, channels_last: bool, class_2_color, rect: _Rect) -> None:
    s = _f32(seg)
    if channels_last:
        B, H, W, C = s.shape
    else:
        B, C, H, W = s.shape
    table = torch.from_numpy(class_color_table(class_2_color, C)).to(s.device)
    _call("soccdpt_vis_color_masks", _ptr(s), B, C, H, W, 1 if channels_last else 0, _ptr(table), _ptr(rect.buf), *rect.args, device=s.device)


def color_masks(seg: torch.Tensor, class_2_color) -> torch.Tensor:
    """seg [B,C,H,W] (cuda), class_2_color {class: colour} or a sequence -> u8 [B,H,W,3]: zeros, then class_2_color[c] where seg[:, c] > 0.5 for
    c = 0 .. C-1 (the last matching class wins; 0.5 itself and NaN do not match).  Colours are written as given."""
    _need_cuda(seg, "color_masks")
    if seg.dim() != 4:
        raise ValueError("color_masks: expected [B,C,H,W]")
    rect = _Rect.whole(seg.shape[0], seg.shape[2], seg.shape[3], seg.device)
    _masks_into(seg, False, class_2_color, rect)
    return rect.buf


def color_segmentation(disp_img_masks: torch.Tensor, frame, class_2_color) -> torch.Tensor:
    """The reference's color_segmentation: disp_img_masks [H,W,C] (cuda); `frame` only gives the shape, as np.zeros_like(frame) does there."""
    _need_cuda(disp_img_masks, "color_segmentation")
    if disp_img_masks.dim() != 3:
        raise ValueError("color_segmentation: expected [H,W,C] masks")
    H, W, _ = disp_img_masks.shape
    if frame is not None and tuple(frame.shape[:2]) != (H, W):
        raise ValueError(f"color_segmentation: masks are {H} x {W}, the frame is {tuple(frame.shape[:2])}")
    rect = _Rect.whole(1, H, W, disp_img_masks.device)
    _masks_into(disp_img_masks.unsqueeze(0), True, class_2_color, rect)
    return rect.buf[0]


def resize_taps(src: int, dst: int) -> np.ndarray:
    """[dst,3] int32 {i0, i1, w1} of one axis (soccdpt_vis_resize_taps: built on the host in double precision)."""
    taps = np.empty((int(dst), 3), dtype=np.int32)
    L = load_library()
    if L.soccdpt_vis_resize_taps(int(src), int(dst), taps.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) != 0:
        raise RuntimeError("soccdpt_vis_resize_taps failed: " + L.soccdpt_last_error(None).decode())
    return taps


def _u8_image(img: torch.Tensor, what: str) -> Tuple[torch.Tensor, bool]:
    _need_cuda(img, what)
    if img.dtype != torch.uint8 or img.dim() not in (3, 4) or img.shape[-1] != 3:
        raise ValueError(f"{what}: expected a uint8 image [H,W,3] or [B,H,W,3], got {tuple(img.shape)} {img.dtype}")
    return (img if img.dim() == 4 else img.unsqueeze(0)).detach().contiguous(), img.dim() == 4


def _resize_into(img4: torch.Tensor, Hd: int, Wd: int, rect: _Rect) -> None:
    B, Hs, Ws, _ = img4.shape
    yt = xt = None
    if (Hs, Ws) != (Hd, Wd):
        yt = torch.from_numpy(resize_taps(Hs, Hd)).to(img4.device)
        xt = torch.from_numpy(resize_taps(Ws, Wd)).to(img4.device)
    _call("soccdpt_vis_resize", _ptr(img4), B, Hs, Ws, _ptr(yt), _ptr(xt), Hd, Wd, _ptr(rect.buf), *rect.args, device=img4.device)


def resize_bgr(img: torch.Tensor, dsize: Sequence[int]) -> torch.Tensor:
    """cv2.resize(img, dsize) with dsize = (width, height): bilinear, half-pixel centres, clamped borders, 11-bit integer weights and integer
    arithmetic (exactly reproducible in numpy).  img u8 [H,W,3] or [B,H,W,3] (cuda).  An equal size is a copy."""
    img4, batched = _u8_image(img, "resize_bgr")
    Wd, Hd = int(dsize[0]), int(dsize[1])
    rect = _Rect.whole(img4.shape[0], Hd, Wd, img4.device)
    _resize_into(img4, Hd, Wd, rect)
    return rect.buf if batched else rect.buf[0]


def half_size(H: int, W: int) -> Tuple[int, int]:
    """(round-half-even(H / 2), round-half-even(W / 2)): Python's round()."""
    return int(round(H / 2)), int(round(W / 2))


def shrink_half(img: torch.Tensor, swap_rb: bool = False) -> torch.Tensor:
    """cv2.resize(img, (0, 0), fx=0.5, fy=0.5): u8 [H,W,3] or [B,H,W,3] -> [.., round(H/2), round(W/2), 3], (a + b + c + d + 2) >> 2 over rows 2y, 2y+1
    and columns 2x, 2x+1, clamped to the last.  swap_rb also exchanges channels 0 and 2 (cv2.cvtColor(img, cv2.COLOR_BGR2RGB))."""
    img4, batched = _u8_image(img, "shrink_half")
    B, H, W, _ = img4.shape
    if H < 2 or W < 2:
        raise ValueError("shrink_half: the image must be at least 2 x 2")
    Hd, Wd = half_size(H, W)
    out = torch.empty((B, Hd, Wd, 3), dtype=torch.uint8, device=img4.device)
    _call("soccdpt_vis_shrink_half", _ptr(img4), B, H, W, 1 if swap_rb else 0, _ptr(out), device=img4.device)
    return out if batched else out[0]


def evaluation_panel(frame_bgr: torch.Tensor, disp_pred: torch.Tensor, seg_pred: torch.Tensor, class_2_color, disp_gt: Optional[torch.Tensor] = None,
                     seg_gt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The reference's `plot` picture: u8 RGB [H, round(k W / 2), 3] (cuda) from

        [frame | depth pred | depth gt]
        [frame | seg pred   | seg gt  ]      k = 3 with ground truth (evaluate), k = 2 without (evaluate_occupancy)

    frame_bgr u8 [H,W,3]; disp_* [h,w] inverse depth; seg_* [C,h,w] class maps; all cuda.  Depth and class pictures of another size than the frame's
    are coloured at their own size and resized (bilinear) into their tile.  Every tile is written straight into the [2H, kW, 3] BGR panel, which the
    half-size shrink reads once, swapping B and R on the way (the reference's cvtColor + resize)."""
    frame, _ = _u8_image(frame_bgr, "evaluation_panel(frame_bgr)")
    if frame.shape[0] != 1:
        raise ValueError("evaluation_panel: one frame [H,W,3]")
    if (disp_gt is None) != (seg_gt is None):
        raise ValueError("evaluation_panel: give both ground-truth pictures or neither")
    dev = frame.device
    _, H, W, _ = frame.shape
    k = 3 if disp_gt is not None else 2
    panel = torch.empty((2 * H, k * W, 3), dtype=torch.uint8, device=dev)

    def depth(t, col):
        _need_cuda(t, "evaluation_panel(disp)")
        t = t.detach().squeeze()
        if t.dim() != 2:
            raise ValueError("evaluation_panel: inverse depth is [h,w]")
        if tuple(t.shape) == (H, W):
            _colorize_into(t.unsqueeze(0), _Rect.tile(panel, 0, col))
        else:
            _resize_into(colorize_disparity(t.unsqueeze(0)), H, W, _Rect.tile(panel, 0, col))

    def classes(t, col):
        _need_cuda(t, "evaluation_panel(seg)")
        t = t.detach()
        t = t[0] if t.dim() == 4 else t
        if t.dim() != 3:
            raise ValueError("evaluation_panel: class maps are [C,h,w]")
        if tuple(t.shape[1:]) == (H, W):
            _masks_into(t.unsqueeze(0), False, class_2_color, _Rect.tile(panel, H, col))
        else:
            _resize_into(color_masks(t.unsqueeze(0), class_2_color), H, W, _Rect.tile(panel, H, col))

    _resize_into(frame, H, W, _Rect.tile(panel, 0, 0))
    _resize_into(frame, H, W, _Rect.tile(panel, H, 0))
    depth(disp_pred, W)
    classes(seg_pred, W)
    if k == 3:
        depth(disp_gt, 2 * W)
        classes(seg_gt, 2 * W)
    return shrink_half(panel, swap_rb=True)


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(img, bgr: bool = False) -> bytes:
    """u8 [H,W,3] (torch tensor on any device, or numpy) -> the bytes of an 8-bit RGB PNG: filter-0 rows, one zlib stream, standard library only."""
    a = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"write_png: expected a uint8 image [H,W,3], got {a.shape} {a.dtype}")
    if bgr:
        a = a[:, :, ::-1]
    H, W, _ = a.shape
    rows = np.zeros((H, 1 + 3 * W), dtype=np.uint8)      # byte 0 of every row: filter type 0 (none)
    rows[:, 1:] = a.reshape(H, 3 * W)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)   # 8 bits, colour type 2 (RGB), deflate, adaptive filtering, no interlace
    return b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", ihdr) + _png_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _png_chunk(b"IEND", b"")


def write_png(path: str, img, bgr: bool = False) -> None:
    """Write u8 [H,W,3] as an 8-bit RGB PNG; bgr=True: the image is B, G, R (what cv2.imwrite expects) and is swapped on the way out."""
    data = png_bytes(img, bgr=bgr)
    with open(path, "wb") as f:
        f.write(data)
