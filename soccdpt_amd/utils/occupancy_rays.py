"""Observed space of a camera frame in the occupancy grid, and the 3-D IoU over it (csrc/occ_rays.hip, include/soccdpt_occ_rays.h).

The ground-truth grid knows only what one camera frame saw: voxels behind the first surface, outside the frustum or under the hidden half of the
depth map are unknown, not empty.  `occupancy_iou` counts them all the same.  Here one ray per pixel runs from the camera to the measured depth
and marks every voxel it enters -- free space and the surface voxel at its end --, and the IoU is counted over those voxels only.

  camera_to_voxel         the 3 x 4 matrix the caster takes, from a voxel_to_camera() matrix (float64 inverse, on the host)
  observed_voxels         depth [rows,H,W] -> voxel mask [rows, nvw] int32: voxel m = (i0 g1 + i1) g2 + i2 is bit m & 31 of word m >> 5 (one bit per
                          VOXEL, not the C bits per voxel of the packed grids)
  occupancy_iou_observed  occupancy_iou over the observed voxels, plus `observed_voxels` and `observed_fraction`
  apply_observed          a packed grid with its unobserved voxels cleared, for the pictures of utils/occupancy_views.py

The reference has no such mask (its iou_3D is a TODO), so the caster is held to a float64 restatement of its own contract
(tests/occ_rays_refs.py), bit for bit.  There is no CPU fallback: a CPU tensor raises RuntimeError like the rest of the product path."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from ..lib import _call, _ptr
from .occupancy import _as_bits, _need_cuda, pack_occupancy

DEFAULT_STEP = 1     # every pixel: DESIGN.md section 12.6 has the share of observed voxels that coarser steps lose, and what step 1 costs


def camera_to_voxel(voxel_to_camera) -> np.ndarray:
    """3 x 4 float64 N: camera metres -> continuous voxel coordinates in which voxel i covers [i, i + 1).  voxel_to_camera (SOccDPT.voxel_to_camera(),
    OccupancyProcessor.voxel_to_camera()) maps the voxel-centre index i + 0.5 to camera metres as p = L c + t, and c is that continuous coordinate at
    the centre, so N = [L^-1 | -L^-1 t].  The inverse is taken here, in float64; the library inverts nothing."""
    M = np.asarray(voxel_to_camera, dtype=np.float64)
    if M.shape != (3, 4):
        raise ValueError("voxel_to_camera is a 3 x 4 matrix (voxel-centre index -> camera metres)")
    Li = np.linalg.inv(M[:, :3])
    return np.ascontiguousarray(np.concatenate([Li, -(Li @ M[:, 3]).reshape(3, 1)], axis=1))


def _intrinsics(intrinsics) -> np.ndarray:
    K = np.asarray(intrinsics, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if K.shape != (4,):
        raise ValueError("intrinsics are (fx, fy, cx, cy) or the 3 x 3 camera matrix")
    return np.ascontiguousarray(K)


def mask_words(grid_size: Sequence[int]) -> int:
    """nvw: words of one row of a voxel mask."""
    g = [int(v) for v in grid_size[:3]]
    return (g[0] * g[1] * g[2] + 31) // 32


def observed_voxels_raw(depth: torch.Tensor, N: np.ndarray, K: np.ndarray, grid_size: Sequence[int], z_near: float, max_depth: Optional[float], step: int,
                        out: torch.Tensor, clear: bool) -> None:
    """soccdpt_occ_rays_observed with the camera -> voxel matrix N given as it is (no inverse taken)."""
    f64 = ctypes.POINTER(ctypes.c_double)
    N, K = np.ascontiguousarray(N, dtype=np.float64), np.ascontiguousarray(K, dtype=np.float64)
    rows, H, W = depth.shape
    _call("soccdpt_occ_rays_observed", _ptr(depth), rows, H, W, (ctypes.c_int32 * 3)(*[int(v) for v in grid_size[:3]]), N.ctypes.data_as(f64),
          K.ctypes.data_as(f64), float(z_near), 0.0 if max_depth is None else float(max_depth), int(step), 1 if clear else 0, _ptr(out), device=depth.device)


def observed_voxels(depth: torch.Tensor, voxel_to_camera, intrinsics, grid_size: Sequence[int], z_near: float = 0.0, max_depth: Optional[float] = None,
                    step: int = DEFAULT_STEP, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """depth [rows,H,W] or [H,W] f32 in camera metres (cuda; OccupancyProcessor.process's `depth`) -> voxel mask int32 [rows, nvw] of the voxels the
    camera saw: one ray per cast pixel (every step-th, starting at step // 2) from z_near along the pixel's direction to the measured depth (at most
    max_depth), every voxel entered is set, the one holding the end point included.  Pixels whose depth is NaN, +-inf, 0, negative or <= z_near --
    the hidden half of the generator's depth map among them -- cast nothing.  out: a mask to OR the result onto (row b onto row b); None: a new one."""
    _need_cuda(depth, "observed_voxels")
    d = depth.detach()
    if d.dim() == 2:
        d = d.unsqueeze(0)
    if d.dim() != 3:
        raise ValueError("observed_voxels: depth is [rows,H,W] or [H,W]")
    d = d.to(torch.float32).contiguous()
    nvw = mask_words(grid_size)
    clear = out is None
    if out is None:
        out = torch.empty((d.shape[0], nvw), dtype=torch.int32, device=d.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (d.shape[0], nvw) or out.device != d.device or not out.is_contiguous():
        raise ValueError(f"observed_voxels: out is a contiguous int32 [{d.shape[0]}, {nvw}] tensor on the depth's device")
    observed_voxels_raw(d, camera_to_voxel(voxel_to_camera), _intrinsics(intrinsics), grid_size, z_near, max_depth, step, out, clear)
    return out


def _mask(observed: torch.Tensor, nvox: int, rows: int, device, what: str) -> torch.Tensor:
    _need_cuda(observed, what)
    m = observed.detach()
    m = m.reshape(1, -1) if m.dim() == 1 else m
    if m.dtype != torch.int32 or m.dim() != 2 or m.shape[1] != (nvox + 31) // 32 or m.shape[0] not in (1, rows) or m.device != device:
        raise ValueError(f"{what}: observed is an int32 voxel mask [1 or {rows}, {(nvox + 31) // 32}] on the grid's device, got {tuple(observed.shape)} {observed.dtype}")
    return m.contiguous()


def _grids(pred, gt, num_classes: int, grid_size, what: str) -> Tuple[torch.Tensor, torch.Tensor, int]:
    C = int(num_classes)
    pb, pn = _as_bits(pred, C, f"{what}(pred)")
    gb, gn = _as_bits(gt, C, f"{what}(gt)")
    if pb.shape[1] != gb.shape[1] or (pn is not None and gn is not None and pn != gn):
        raise ValueError(f"{what}: pred and gt describe grids of different sizes")
    if pb.shape[0] not in (1, gb.shape[0]) or pb.device != gb.device:
        raise ValueError(f"{what}: pred must have one row or as many as gt, on the same device")
    ncell = pn or gn or (int(np.prod([int(v) for v in grid_size[:3]])) * C if grid_size is not None else gb.shape[1] * 32)
    if (ncell + 31) // 32 != gb.shape[1] or ncell % C:
        raise ValueError(f"{what}: grid_size does not match the number of packed words (give grid_size when g0 * g1 * g2 * C is no multiple of 32)")
    return pb, gb, ncell // C


def occupancy_iou_observed(pred: torch.Tensor, gt: torch.Tensor, observed: torch.Tensor, num_classes: int = 3, grid_size: Optional[Sequence[int]] = None,
                           include_gt: bool = True) -> dict:
    """occupancy_iou over observed space.  pred / gt as there (packed int32 words or dense grids, pred with one row or as many as gt); observed: a
    voxel mask of observed_voxels, [nvw] / [1, nvw] for every row or [rows, nvw].  Only cells whose voxel is in the row's effective mask are
    counted; include_gt (the default) puts the ground truth's own occupied voxels into it, so that a surface voxel is never lost to a rounding
    difference between the generator and the caster.  Returns the dict of occupancy_iou (counts, iou_per_class, iou_3D, precision, recall) plus
    observed_voxels [rows] int64, the size of the effective mask, and observed_fraction [rows] f64 = observed_voxels / (g0 g1 g2)."""
    C = int(num_classes)
    pb, gb, nvox = _grids(pred, gt, C, grid_size, "occupancy_iou_observed")
    rows = gb.shape[0]
    m = _mask(observed, nvox, rows, gb.device, "occupancy_iou_observed")
    counts = torch.empty((rows, C, 4), dtype=torch.int64, device=gb.device)
    nobs = torch.empty((rows,), dtype=torch.int64, device=gb.device)
    _call("soccdpt_occ_iou_counts_masked", _ptr(pb), pb.shape[0], _ptr(gb), rows, nvox, C, _ptr(m), m.shape[0], 1 if include_gt else 0, _ptr(counts), _ptr(nobs),
          device=gb.device)
    c = counts.double()
    inter, union, npred, ngt = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    iou = inter / (union + 1e-7)
    return dict(counts=counts, iou_per_class=iou, iou_3D=iou.sum(dim=1) / C, precision=inter / (npred + 1e-7), recall=inter / (ngt + 1e-7),
                observed_voxels=nobs, observed_fraction=nobs.double() / nvox)


def apply_observed(bits: torch.Tensor, observed: torch.Tensor, num_classes: int, grid_size: Sequence[int]) -> torch.Tensor:
    """A packed grid (or a dense one) with the class bits of every unobserved voxel cleared -> packed int32 [rows, nwords], for occupancy_view /
    occupancy_overlay / occupancy_panel to show observed space only.  The voxel mask is widened to C bits per voxel through soccdpt_occ_pack."""
    C = int(num_classes)
    g = tuple(int(v) for v in grid_size[:3])
    b, ncell = _as_bits(bits, C, "apply_observed")
    nvox = g[0] * g[1] * g[2]
    if (ncell is not None and ncell != nvox * C) or b.shape[1] != (nvox * C + 31) // 32:
        raise ValueError(f"apply_observed: the grid does not have {g} x {C} cells")
    m = _mask(observed, nvox, b.shape[0], b.device, "apply_observed")
    shifts = torch.arange(32, dtype=torch.int32, device=b.device)
    vox = ((m.unsqueeze(-1) >> shifts) & 1).reshape(m.shape[0], -1)[:, :nvox].to(torch.uint8)
    cells = pack_occupancy(vox.unsqueeze(-1).expand(-1, -1, C).reshape(m.shape[0], g[0], g[1], g[2], C).contiguous(), 0.5)
    return b & cells
