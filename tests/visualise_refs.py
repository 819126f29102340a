"""numpy specification of the evaluation pictures (soccdpt_amd/utils/visualise.py, csrc/visualise.hip): what the reference does with numpy and cv2
(SOccDPT/utils/__init__.py:35-43, 627-708), restated with the arithmetic spelled out so that every result is exact:

  colorize      f32 subtract, f32 divide, f32 multiply by 255, truncation to u8, table look-up; per-frame min / max over the finite values
  color_masks   zeros, then class_2_color[c] where seg[c] > 0.5 for c = 0 .. C-1
  resize        cv2.resize's bilinear geometry with 11-bit integer weights and a 22-bit integer accumulation
  shrink_half   2 x 2 box mean (a + b + c + d + 2) >> 2 with clamped taps, optional B <-> R swap
  panel         np.concatenate of the tiles, then shrink_half with the swap"""
import numpy as np

from soccdpt_amd.utils.plasma_lut import PLASMA_BGR_HEX

LUT_BGR = np.frombuffer(bytes.fromhex(PLASMA_BGR_HEX), dtype=np.uint8).reshape(256, 3)


def minmax(frame):
    """-> (min, max) as f32 over the finite values; (+inf, -inf) when there is none."""
    d = np.asarray(frame, dtype=np.float32)
    fin = d[np.isfinite(d)]
    if fin.size == 0:
        return np.float32(np.inf), np.float32(-np.inf)
    return fin.min(), fin.max()


def colorize_index(frame):
    """[H,W] f32 -> [H,W] u8 index: ((d - min) / (max - min) * 255).astype(np.uint8) in f32; 0 where that is undefined."""
    d = np.asarray(frame, dtype=np.float32)
    mn, mx = minmax(d)
    idx = np.zeros(d.shape, dtype=np.uint8)
    if not mx > mn:
        return idx
    with np.errstate(all="ignore"):
        v = (d - mn) / np.float32(mx - mn)
        assert v.dtype == np.float32
        ok = np.isfinite(d) & (v >= 0) & (v <= 1)
        idx[ok] = (v[ok] * np.float32(255.0)).astype(np.uint8)
    return idx


def colorize(disp):
    """[H,W] or [B,H,W] -> u8 [..,H,W,3] BGR."""
    d = np.asarray(disp, dtype=np.float32)
    if d.ndim == 2:
        return LUT_BGR[colorize_index(d)]
    return np.stack([LUT_BGR[colorize_index(f)] for f in d])


def color_table(class_2_color, C):
    return np.array([class_2_color[c] for c in range(C)], dtype=np.uint8).reshape(C, 3)


def color_masks_hwc(masks, class_2_color):
    """[H,W,C] -> u8 [H,W,3]: the reference's color_segmentation."""
    m = np.asarray(masks) > 0.5
    out = np.zeros(m.shape[:2] + (3,), dtype=np.uint8)
    table = color_table(class_2_color, m.shape[2])
    for c in range(m.shape[2]):
        out[m[:, :, c]] = table[c]
    return out


def color_masks(seg, class_2_color):
    """[B,C,H,W] -> u8 [B,H,W,3]."""
    return np.stack([color_masks_hwc(np.moveaxis(s, 0, 2), class_2_color) for s in np.asarray(seg)])


def resize_taps(src, dst):
    """[dst,3] int32 {i0, i1, w1}, computed in double precision."""
    i = np.arange(dst, dtype=np.float64)
    f = (i + 0.5) * (float(src) / float(dst)) - 0.5
    i0 = np.floor(f).astype(np.int64)
    f = f - i0
    lo, hi = i0 < 0, i0 >= src - 1
    f[lo | hi] = 0.0
    i0[lo] = 0
    i0[hi] = src - 1
    return np.stack([i0, np.minimum(i0 + 1, src - 1), np.rint(f * 2048.0).astype(np.int64)], axis=1).astype(np.int32)


def resize(img, dsize):
    """u8 [H,W,3], dsize = (width, height) -> u8 [height,width,3]."""
    a = np.asarray(img).astype(np.int64)
    Wd, Hd = int(dsize[0]), int(dsize[1])
    yt, xt = resize_taps(a.shape[0], Hd).astype(np.int64), resize_taps(a.shape[1], Wd).astype(np.int64)
    wy1, wx1 = yt[:, 2][:, None, None], xt[:, 2][None, :, None]
    wy0, wx0 = 2048 - wy1, 2048 - wx1
    ya, yb, xa, xb = yt[:, 0], yt[:, 1], xt[:, 0], xt[:, 1]
    s = a[ya][:, xa] * wx0 * wy0 + a[ya][:, xb] * wx1 * wy0 + a[yb][:, xa] * wx0 * wy1 + a[yb][:, xb] * wx1 * wy1
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


def half_size(H, W):
    return int(np.rint(H / 2)), int(np.rint(W / 2))      # np.rint rounds half to even


def shrink_half(img, swap_rb=False):
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape[:2]
    Hd, Wd = half_size(H, W)
    ya, yb = np.minimum(2 * np.arange(Hd), H - 1), np.minimum(2 * np.arange(Hd) + 1, H - 1)
    xa, xb = np.minimum(2 * np.arange(Wd), W - 1), np.minimum(2 * np.arange(Wd) + 1, W - 1)
    out = ((a[ya][:, xa] + a[ya][:, xb] + a[yb][:, xa] + a[yb][:, xb] + 2) >> 2).astype(np.uint8)
    return np.ascontiguousarray(out[:, :, ::-1]) if swap_rb else out


def panel(frame_bgr, disp_pred, seg_pred, class_2_color, disp_gt=None, seg_gt=None):
    """The reference's concatenate-then-shrink (utils/__init__.py:666-708): frame u8 [H,W,3], disp [h,w], seg [C,h,w] -> u8 RGB [H, round(kW/2), 3]."""
    frame = np.asarray(frame_bgr)
    H, W = frame.shape[:2]

    def fit(img):
        return img if img.shape[:2] == (H, W) else resize(img, (W, H))
    top = [frame, fit(colorize(disp_pred))]
    bottom = [frame, fit(color_masks_hwc(np.moveaxis(np.asarray(seg_pred), 0, 2), class_2_color))]
    if disp_gt is not None:
        top.append(fit(colorize(disp_gt)))
        bottom.append(fit(color_masks_hwc(np.moveaxis(np.asarray(seg_gt), 0, 2), class_2_color)))
    vis = np.concatenate([np.concatenate(top, 1), np.concatenate(bottom, 1)], 0)
    return shrink_half(vis, swap_rb=True)


def plot_points(points0, gt_color_img):
    """utils/__init__.py:718-732: every tenth point beside every tenth pixel colour, rows whose first colour channel is 0 dropped -> [N,6]."""
    p = np.asarray(points0).reshape(-1, 3)[::10]
    c = np.asarray(gt_color_img).reshape(-1, 3)[::10]
    keep = c[:, 0] > 0
    return np.hstack([p[keep], c[keep]])


def png_decode(data):
    """A minimal reader for what write_png writes: 8-bit RGB, no interlace, filter-0 rows -> u8 [H,W,3]."""
    import struct
    import zlib
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, size = 8, b"", None
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == (zlib.crc32(tag + body) & 0xFFFFFFFF), tag
        if tag == b"IHDR":
            W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            assert (depth, ctype, comp, filt, lace) == (8, 2, 0, 0, 0)
            size = (H, W)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    assert tag == b"IEND" and size is not None
    H, W = size
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(H, 1 + 3 * W)
    assert not rows[:, 0].any(), "filter type 0 on every row"
    return rows[:, 1:].reshape(H, W, 3).copy()
