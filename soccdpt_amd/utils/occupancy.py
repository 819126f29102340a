"""Consumers of the semantic occupancy grid on the GPU: dense grid <-> packed bits, the reference's ordered point list and a 3-D IoU.

  occupancy_grid_to_points      SOccDPT/utils/__init__.py:532-568 (same name, arguments, assert, order and f64 [N,4] result)
  semantic_pc_to_colors_and_pc  SOccDPT/utils/__init__.py:571-595
  occupancy_iou                 the `iou_3D` that utils/__init__.py:392,504 leaves as "# TODO: Implement"

The reference pulls the dense grid to the host and runs np.argwhere over its 6.3 M cells per frame.  Here the grid stays in HBM as packed bits
(`net.last_occ_bits`: 786,432 bytes for the default geometry, layout of csrc/projection.hip) and the kernels of csrc/occ_eval.hip read those.
There is no CPU fallback: a CPU tensor raises RuntimeError like the rest of the product path."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from ..lib import _call, _ptr, load_library

OCC_F32, OCC_U8, OCC_I32 = 0, 1, 2          # SOCCDPT_OCC_* of include/soccdpt_hip.h
_DTYPES = {torch.float32: OCC_F32, torch.uint8: OCC_U8, torch.bool: OCC_U8, torch.int32: OCC_I32}


class OccupancyPoints(NamedTuple):
    points: torch.Tensor                 # [N,4] f64 (x, y, z, class_id); [max_points,4] in the no-sync form (rows past N are zero)
    colors: Optional[torch.Tensor]       # [N,3] u8 when a class_2_color table was given
    counts: torch.Tensor                 # [rows,C] int64: list rows per grid row and class (the list is row-major, class-major in these)
    total: torch.Tensor                  # 0-dim int64 device tensor: the true N


def _need_cuda(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"{what}: the occupancy kernels run on the GPU only; pass a cuda tensor (there is no CPU fallback)")


def occupancy_shape_f32(grid_size: Sequence[int], scale: Sequence[float]) -> np.ndarray:
    """Grid extent in metres as the reference computes it: float(grid_size[i] / scale[i]) rounded to f32 (utils/__init__.py:541-547)."""
    return np.array([float(grid_size[i] / scale[i]) for i in range(3)], dtype=np.float32)


def class_color_table(class_2_color, num_classes: int) -> np.ndarray:
    """{class_id: (r, g, b)} or a sequence of colours -> [C,3] u8."""
    return np.array([class_2_color[c] for c in range(num_classes)], dtype=np.uint8).reshape(num_classes, 3)


def pack_occupancy(grid: torch.Tensor, threshold: float = 0.5, strict: bool = False) -> torch.Tensor:
    """Dense [g0,g1,g2,C] or [rows,g0,g1,g2,C] (f32, bool, u8, or int32 point counts; cuda) -> packed [rows, nwords] int32, the dtype and bit
    layout of `net.last_occ_bits`.  A bit is set where v >= threshold, or v > threshold with strict=True; the comparison is done in f32."""
    _need_cuda(grid, "pack_occupancy")
    if grid.dim() not in (4, 5):
        raise ValueError("pack_occupancy: expected a dense grid [g0,g1,g2,C] or [rows,g0,g1,g2,C]")
    if grid.dtype not in _DTYPES:
        raise TypeError(f"pack_occupancy: dtype {grid.dtype} is not one of float32, bool, uint8, int32")
    rows = 1 if grid.dim() == 4 else grid.shape[0]
    g = grid.detach().contiguous()
    ncell = g.numel() // rows
    bits = torch.empty((rows, (ncell + 31) // 32), dtype=torch.int32, device=g.device)
    _call("soccdpt_occ_pack", _ptr(g), _DTYPES[grid.dtype], rows, ncell, float(threshold), 1 if strict else 0, _ptr(bits), device=g.device)
    return bits


def occupancy_bits_to_points(bits: torch.Tensor, grid_size: Sequence[int] = (256, 256, 32), scale: Sequence[float] = (2.0, 2.0, 0.666),
                             num_classes: int = 3, rows: int = 1, class_2_color=None, max_points: Optional[int] = None) -> OccupancyPoints:
    """Packed bits [rows * nwords] int32 (cuda) -> OccupancyPoints.  The list holds the `rows` grids one after the other, each class-major with the
    cell index ascending inside a class: for rows == 1 exactly what the reference's occupancy_grid_to_points returns for the dense grid.
    max_points=None reads N back once (one 8-byte device-to-host copy) and allocates exactly; max_points=K never synchronises: the result has K rows, the
    first min(N, K) of them the head of the full list, and `total` holds N on the device."""
    _need_cuda(bits, "occupancy_bits_to_points")
    g = [int(v) for v in grid_size[:3]]
    C, rows = int(num_classes), int(rows)
    ncell = g[0] * g[1] * g[2] * C
    nwords = (ncell + 31) // 32
    if bits.dtype != torch.int32 or bits.numel() != rows * nwords:
        raise ValueError(f"occupancy_bits_to_points: expected {rows} x {nwords} int32 words for grid {tuple(g)} x {C} classes, got {tuple(bits.shape)} {bits.dtype}")
    b = bits.detach().contiguous()
    dev = b.device
    nscratch = load_library().soccdpt_occ_points_scratch_bytes(rows, ncell, C)
    if nscratch == 0:
        raise ValueError("occupancy_bits_to_points: need 1 <= num_classes <= 8 and 1 <= rows <= 65535")
    scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
    counts = torch.empty((rows, C), dtype=torch.int64, device=dev)
    total = torch.empty((), dtype=torch.int64, device=dev)
    shape = occupancy_shape_f32(g, scale)
    table = colors = None
    _call("soccdpt_occ_points_count", _ptr(b), rows, ncell, C, _ptr(scratch), nscratch, _ptr(counts), _ptr(total), device=dev)
    if max_points is None:
        n = int(total.item())
        points = torch.empty((n, 4), dtype=torch.float64, device=dev)
    else:
        n = int(max_points)
        points = torch.zeros((n, 4), dtype=torch.float64, device=dev)
    if class_2_color is not None:
        table = torch.from_numpy(class_color_table(class_2_color, C)).to(dev)
        colors = torch.empty((n, 3), dtype=torch.uint8, device=dev) if max_points is None else torch.zeros((n, 3), dtype=torch.uint8, device=dev)
    _call("soccdpt_occ_points_write", _ptr(b), rows, (ctypes.c_int32 * 3)(*g), C, (ctypes.c_float * 3)(*[float(v) for v in shape]), _ptr(scratch), nscratch,
          n, _ptr(points), _ptr(table), _ptr(colors), device=dev)
    return OccupancyPoints(points, colors, counts, total)


def occupancy_grid_to_points(occupancy_grid: torch.Tensor, grid_size=(256, 256, 32), scale=(2.0, 2.0, 0.666), shift=(0.0, 0.0, 0.0)) -> torch.Tensor:
    """The reference's occupancy_grid_to_points on the GPU: dense [g0,g1,g2,C] (f32, bool or u8; cuda) -> float64 [N,4] rows
    (x, y, z, class_id) in metres for every cell >= 0.5, class-major, bit-equal to the numpy original.  `shift` is accepted and unused, as there."""
    _need_cuda(occupancy_grid, "occupancy_grid_to_points")
    assert len(occupancy_grid.shape) == 4, "occupancy_grid must be 3D with one channel per class"
    if tuple(occupancy_grid.shape[:3]) != tuple(int(v) for v in grid_size[:3]):
        raise ValueError(f"occupancy_grid_to_points: grid of shape {tuple(occupancy_grid.shape)} does not match grid_size {tuple(grid_size)}")
    bits = pack_occupancy(occupancy_grid, 0.5, strict=False)
    return occupancy_bits_to_points(bits, grid_size, scale, num_classes=occupancy_grid.shape[3]).points


def semantic_pc_to_colors_and_pc(semantic_pc: torch.Tensor, class_2_color):
    """[N,4] (x, y, z, class_id) -> (points [N,3], colors [N,3] u8), a gather on the list's device."""
    _need_cuda(semantic_pc, "semantic_pc_to_colors_and_pc")
    cls = semantic_pc[:, 3].long()
    n = (max(class_2_color) + 1) if isinstance(class_2_color, dict) else len(class_2_color)
    table = np.zeros((n, 3), dtype=np.uint8)
    for c in (class_2_color if isinstance(class_2_color, dict) else range(len(class_2_color))):
        table[c] = class_2_color[c]
    return semantic_pc[:, :3], torch.from_numpy(table).to(semantic_pc.device)[cls]


def _as_bits(t: torch.Tensor, num_classes: int, what: str):
    """-> ([rows, nwords] int32, ncell or None when only the word count is known)."""
    _need_cuda(t, what)
    if t.dim() >= 4:
        if t.shape[-1] != num_classes:
            raise ValueError(f"{what}: dense grids are [.., g0, g1, g2, {num_classes}], got {tuple(t.shape)}")
        ncell = int(np.prod(t.shape[-4:]))
        return pack_occupancy(t if t.dim() <= 5 else t.reshape((-1,) + tuple(t.shape[-4:])), 0.5, strict=False), ncell
    if t.dtype != torch.int32 or t.dim() > 2:
        raise ValueError(f"{what}: expected packed int32 words [nwords] / [rows, nwords] or a dense grid, got {tuple(t.shape)} {t.dtype}")
    return t.detach().reshape(1 if t.dim() == 1 else t.shape[0], -1).contiguous(), None


def occupancy_iou(pred: torch.Tensor, gt: torch.Tensor, num_classes: int = 3, grid_size: Optional[Sequence[int]] = None) -> dict:
    """3-D IoU of two semantic occupancy grids on the GPU.  pred / gt: packed int32 words ([nwords] or [rows, nwords]) or dense grids
    ([g0,g1,g2,C] / [rows,g0,g1,g2,C], occupied where >= 0.5).  pred may have one row against several gt rows (the model's grid is the union over
    the batch).  grid_size is only needed when both are packed and g0 * g1 * g2 * C is not a multiple of 32.  Returns device tensors:
    counts [rows,C,4] int64 (intersection, union, pred, gt), iou_per_class [rows,C] = inter / (union + 1e-7) in f64, iou_3D [rows] = its mean over
    the classes (the convention of the 2-D iou_metric), precision, recall [rows,C]; an empty union gives 0, never NaN."""
    C = int(num_classes)
    pb, pn = _as_bits(pred, C, "occupancy_iou(pred)")
    gb, gn = _as_bits(gt, C, "occupancy_iou(gt)")
    if pb.shape[1] != gb.shape[1] or (pn is not None and gn is not None and pn != gn):
        raise ValueError("occupancy_iou: pred and gt describe grids of different sizes")
    if pb.shape[0] not in (1, gb.shape[0]) or pb.device != gb.device:
        raise ValueError("occupancy_iou: pred must have one row or as many as gt, on the same device")
    ncell = pn or gn or (int(np.prod(grid_size[:3])) * C if grid_size is not None else gb.shape[1] * 32)
    if (ncell + 31) // 32 != gb.shape[1]:
        raise ValueError("occupancy_iou: grid_size does not match the number of packed words")
    rows = gb.shape[0]
    counts = torch.empty((rows, C, 4), dtype=torch.int64, device=gb.device)
    _call("soccdpt_occ_iou_counts", _ptr(pb), pb.shape[0], _ptr(gb), rows, ncell, C, _ptr(counts), device=gb.device)
    c = counts.double()
    inter, union, npred, ngt = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    iou = inter / (union + 1e-7)
    return dict(counts=counts, iou_per_class=iou, iou_3D=iou.sum(dim=1) / C, precision=inter / (npred + 1e-7), recall=inter / (ngt + 1e-7))
