"""numpy restatements of include/soccdpt_occ_view.h (TEST INFRASTRUCTURE ONLY): what csrc/occ_view.hip must return, bit for bit.  The reference
project has no picture of the occupancy grid, so these follow the header's definitions, not reference code.  tests/test_occ_view_cpu.py holds them
against hand-written cases; tests/test_occ_view_gpu.py holds the kernels against them."""
import math

import numpy as np

EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pack(dense: np.ndarray, tail_garbage: bool = False) -> np.ndarray:
    """bool [rows,g0,g1,g2,C] -> uint32 [rows,nwords], bit n & 31 of word n >> 5 for row-major cell n; tail_garbage sets the bits past the last cell."""
    rows = dense.shape[0]
    flat = dense.reshape(rows, -1).astype(bool)
    pad = (-flat.shape[1]) % 32
    flat = np.concatenate([flat, np.full((rows, pad), tail_garbage, dtype=bool)], axis=1)
    return np.ascontiguousarray(np.packbits(flat, axis=1, bitorder="little")).view(np.uint32).reshape(rows, -1)


def columns(dense: np.ndarray, axis: int, from_high: bool):
    """bool [rows,g0,g1,g2,C] -> (top u8, first i32, count i32, classes u8), each [rows,A,B]."""
    rows, C = dense.shape[0], dense.shape[-1]
    d = np.moveaxis(dense.astype(bool), 1 + axis, 3)             # [rows, A, B, len, C]
    L = d.shape[3]
    if from_high:
        d = d[:, :, :, ::-1]
    occ = d.any(axis=-1)                                          # [rows, A, B, len]
    count = occ.sum(axis=-1).astype(np.int32)
    empty = count == 0
    k = occ.argmax(axis=-1)                                       # first True along the scan
    first = np.where(empty, -1, (L - 1 - k) if from_high else k).astype(np.int32)
    at_first = np.take_along_axis(d, k[..., None, None], axis=3)[:, :, :, 0]     # [rows, A, B, C]
    top = np.where(empty, 255, (C - 1 - at_first[..., ::-1].argmax(axis=-1))).astype(np.uint8)
    weights = (1 << np.arange(C)).astype(np.int64)
    classes = (d.any(axis=3) * weights).sum(axis=-1).astype(np.uint8)
    return top, first, count, classes


def paint(top, first, depth_len: int, from_high: bool, colors, background, shade: int, zoom: int, flip_a: bool, flip_b: bool, transpose: bool) -> np.ndarray:
    """top / first [rows,A,B] -> u8 [rows,h,w,3]; integer arithmetic as in the header (Python's // on non-negative operands is C's division)."""
    colors = np.asarray(colors, dtype=np.int64)
    C = colors.shape[0]
    f = first.astype(np.int64)
    rank = np.clip((depth_len - 1 - f) if from_high else f, 0, depth_len - 1)
    w = 256 - (shade * rank) // max(depth_len - 1, 1)
    empty = (f < 0) | (top >= C)
    col = colors[np.where(empty, 0, top)]                                    # [rows,A,B,3]
    img = ((col * w[..., None] + 128) >> 8).astype(np.uint8)
    img[empty] = np.asarray(background, dtype=np.uint8)
    if flip_a:
        img = img[:, ::-1]
    if flip_b:
        img = img[:, :, ::-1]
    if transpose:
        img = img.transpose(0, 2, 1, 3)
    return np.ascontiguousarray(img.repeat(zoom, axis=1).repeat(zoom, axis=2))


def iou2d(pred_classes, gt_classes, C: int) -> np.ndarray:
    """[pred_rows,..] and [rows,..] u8 maps -> counts [rows,C,4] uint64 (intersection, union, pred, gt)."""
    rows = gt_classes.shape[0]
    p = np.broadcast_to(pred_classes.reshape(pred_classes.shape[0], -1), (rows, gt_classes[0].size))
    g = gt_classes.reshape(rows, -1)
    out = np.zeros((rows, C, 4), dtype=np.uint64)
    for c in range(C):
        pb, gb = (p >> c) & 1, (g >> c) & 1
        out[:, c] = np.stack([(pb & gb).sum(1), (pb | gb).sum(1), pb.sum(1), gb.sum(1)], axis=1)
    return out


def splat(dense: np.ndarray, M, K, half_extent_m: float, max_radius_px: int, z_near: float, H: int, W: int) -> np.ndarray:
    """bool [rows,g0,g1,g2,C] -> zbuf uint64 [rows,H,W].  Python floats are IEEE float64 and every operation below is rounded on its own, in the
    header's order."""
    M = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(12)]
    fx, fy, cx, cy = [float(v) for v in K]
    rows, g0, g1, g2, C = dense.shape
    z = np.full((rows, H, W), EMPTY_KEY, dtype=np.uint64)
    for r, i0, i1, i2, cls in np.argwhere(dense):
        n = ((int(i0) * g1 + int(i1)) * g2 + int(i2)) * C + int(cls)
        a, b, c = i0 + 0.5, i1 + 0.5, i2 + 0.5
        X = ((M[0] * a + M[1] * b) + M[2] * c) + M[3]
        Y = ((M[4] * a + M[5] * b) + M[6] * c) + M[7]
        Z = ((M[8] * a + M[9] * b) + M[10] * c) + M[11]
        if not Z > z_near:
            continue
        try:
            u = math.floor(((X / Z) * fx + cx) + 0.5)
            v = math.floor(((Y / Z) * fy + cy) + 0.5)
            rd = math.floor((half_extent_m / Z) * fx)
        except (OverflowError, ValueError):      # inf / NaN: the kernel drops what cannot reach the frame
            continue
        if rd < 0 or abs(u) > 1 << 30 or abs(v) > 1 << 30:
            continue
        rad = min(max_radius_px, rd)
        key = np.uint64((int(np.float32(Z).view(np.uint32)) << 32) | n)
        x0, x1, y0, y1 = max(u - rad, 0), min(u + rad, W - 1), max(v - rad, 0), min(v + rad, H - 1)
        if x0 <= x1 and y0 <= y1:
            z[r, y0:y1 + 1, x0:x1 + 1] = np.minimum(z[r, y0:y1 + 1, x0:x1 + 1], key)
    return z


def resolve(zbuf: np.ndarray, frames, colors, C: int, alpha: int) -> np.ndarray:
    """zbuf uint64 [rows,H,W], frames u8 [1 or rows,H,W,3] or None -> u8 [rows,H,W,3]."""
    rows, H, W = zbuf.shape
    f = np.zeros((rows, H, W, 3), dtype=np.int64) if frames is None else np.broadcast_to(frames.astype(np.int64), (rows, H, W, 3))
    hit = zbuf != EMPTY_KEY
    cls = ((zbuf & np.uint64(0xFFFFFFFF)) % np.uint64(C)).astype(np.int64)
    col = np.asarray(colors, dtype=np.int64)[np.where(hit, cls, 0)]
    blend = (f * (256 - alpha) + col * alpha + 128) >> 8
    return np.where(hit[..., None], blend, f).astype(np.uint8)
