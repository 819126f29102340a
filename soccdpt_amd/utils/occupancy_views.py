"""Pictures of the semantic occupancy grid on the GPU (csrc/occ_view.hip, include/soccdpt_occ_view.h): the consumer utils/occupancy.py leaves out.

  occupancy_columns   the grid reduced along one axis: first occupied voxel, its class, occupied voxels and the classes seen, per column
  occupancy_view      that column map as a picture (class colour, darker with the depth of the first voxel); bird_eye_view: its top-down default
  bev_iou             per-class IoU of two grids' column maps (`iou_2D`), the 2-D companion of occupancy_iou
  occupancy_overlay   the grid drawn over the camera frame: every occupied voxel's centre goes through a 3 x 4 voxel -> camera matrix and the
                      intrinsics, nearest voxel wins per pixel (z-buffer), its class colour is blended over the frame
  occupancy_panel     overlay(pred) | overlay(gt) over view(pred) | view(gt), painted tile by tile into one buffer

The reference shows the grid only as wandb.Object3D point clouds (SOccDPT/utils/__init__.py:512-523, 754); there is no reference picture, so the
kernels are held to numpy restatements of their own definitions (tests/occ_view_refs.py), bit for bit.  Everything reads the packed bits
(`net.last_occ_bits`, layout of csrc/projection.hip); dense grids go through pack_occupancy first, as in occupancy_iou.  There is no CPU fallback:
a CPU tensor raises RuntimeError like the rest of the product path."""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ..lib import _call, _ptr
from .occupancy import _as_bits, class_color_table
from .visualise import _Rect, _need_cuda, _u8_image


class OccupancyColumns(NamedTuple):
    top: torch.Tensor        # [rows,A,B] u8: highest class id at the first occupied voxel; 255 for an empty column
    first: torch.Tensor      # [rows,A,B] int32: index along the axis of the first occupied voxel; -1 for an empty column
    count: torch.Tensor      # [rows,A,B] int32: occupied voxels of the column
    classes: torch.Tensor    # [rows,A,B] u8: bit c set when class c occurs in the column


def _grid_bits(t, grid_size: Sequence[int], num_classes: int, what: str) -> Tuple[torch.Tensor, Tuple[int, int, int]]:
    """packed [nwords] / [rows, nwords] int32 or a dense grid [.., g0, g1, g2, C] (cuda) -> ([rows, nwords] int32, (g0, g1, g2))."""
    _need_cuda(t, what)
    g = tuple(int(v) for v in grid_size[:3])
    C = int(num_classes)
    if t.dim() >= 4 and tuple(t.shape[-4:-1]) != g:
        raise ValueError(f"{what}: a dense grid of shape {tuple(t.shape)} does not match grid_size {g}")
    bits, _ = _as_bits(t, C, what)
    if min(g) < 1 or not 1 <= C <= 8 or g[0] * g[1] * g[2] * C >= 1 << 32 or bits.shape[1] != (g[0] * g[1] * g[2] * C + 31) // 32:
        raise ValueError(f"{what}: {bits.shape[1]} packed words do not describe a grid {g} x {C} classes (1 <= C <= 8, fewer than 2^32 cells)")
    return bits, g


def _plane(g: Tuple[int, int, int], axis: int) -> Tuple[int, int]:
    """The sizes (A, B) of the two axes that remain after reducing along `axis`, in ascending order."""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    rest = [g[i] for i in range(3) if i != axis]
    return rest[0], rest[1]


def _i32x3(g) -> ctypes.Array:
    return (ctypes.c_int32 * 3)(*g)


def _columns(bits: torch.Tensor, g, C: int, axis: int, from_high: bool, want=("top", "first", "count", "classes")) -> dict:
    rows, dev = bits.shape[0], bits.device
    A, B = _plane(g, axis)
    kinds = dict(top=torch.uint8, first=torch.int32, count=torch.int32, classes=torch.uint8)
    out = {k: (torch.empty((rows, A, B), dtype=dt, device=dev) if k in want else None) for k, dt in kinds.items()}
    _call("soccdpt_occ_view_columns", _ptr(bits), rows, _i32x3(g), C, int(axis), 1 if from_high else 0, _ptr(out["top"]), _ptr(out["first"]),
          _ptr(out["count"]), _ptr(out["classes"]), device=dev)
    return out


def occupancy_columns(bits_or_dense: torch.Tensor, grid_size: Sequence[int], num_classes: int = 3, axis: int = 1, from_high: bool = False) -> OccupancyColumns:
    """The grid reduced along `axis`: OccupancyColumns of [rows,A,B] tensors, A and B the two remaining axes in ascending order.  A voxel is occupied
    when any of its class bits is set; the scan for `first` goes from index 0 upwards, or from the far end downwards with from_high=True."""
    bits, g = _grid_bits(bits_or_dense, grid_size, num_classes, "occupancy_columns")
    return OccupancyColumns(**_columns(bits, g, int(num_classes), axis, from_high))


def view_size(grid_size: Sequence[int], axis: int = 1, zoom: int = 2, transpose: bool = False) -> Tuple[int, int]:
    """(height, width) of the picture occupancy_view paints."""
    A, B = _plane(tuple(int(v) for v in grid_size[:3]), axis)
    return (B * zoom, A * zoom) if transpose else (A * zoom, B * zoom)


def _view_into(bits: torch.Tensor, g, C: int, table: torch.Tensor, axis: int, from_high: bool, zoom: int, shade: int, background, flip, transpose: bool,
               rect: _Rect) -> None:
    cols = _columns(bits, g, C, axis, from_high, want=("top", "first"))
    A, B = _plane(g, axis)
    bg = (ctypes.c_uint8 * 3)(*[int(v) for v in background])
    _call("soccdpt_occ_view_paint", _ptr(cols["top"]), _ptr(cols["first"]), bits.shape[0], A, B, g[axis], 1 if from_high else 0, _ptr(table), C, bg, int(shade),
          int(zoom), 1 if flip[0] else 0, 1 if flip[1] else 0, 1 if transpose else 0, _ptr(rect.buf), *rect.args, device=bits.device)


def _table(class_2_color, C: int, device, reverse: bool = False) -> torch.Tensor:
    t = class_color_table(class_2_color, C)
    return torch.from_numpy(np.ascontiguousarray(t[:, ::-1] if reverse else t)).to(device)


def occupancy_view(bits_or_dense: torch.Tensor, grid_size: Sequence[int], class_2_color, num_classes: int = 3, axis: int = 1, from_high: bool = False,
                   zoom: int = 2, shade: int = 128, background=(32, 32, 32), flip=(False, False), transpose: bool = False) -> torch.Tensor:
    """The grid seen along `axis` -> u8 [rows, h, w, 3] (view_size): one column is a zoom x zoom block in the colour of the class on top of its first
    occupied voxel, scaled by (256 - shade * rank / (g[axis] - 1)) / 256 with rank the distance of that voxel from the side the scan started at
    (0 <= shade <= 192; 0: flat colours); empty columns get `background`.  flip = (A, B) reverses that axis of the [A,B] map, transpose puts B on
    the picture's rows.  Colours are written in the channel order of class_2_color."""
    bits, g = _grid_bits(bits_or_dense, grid_size, num_classes, "occupancy_view")
    h, w = view_size(g, axis, zoom, transpose)
    rect = _Rect.whole(bits.shape[0], h, w, bits.device)
    _view_into(bits, g, int(num_classes), _table(class_2_color, int(num_classes), bits.device), axis, from_high, zoom, shade, background, flip, transpose, rect)
    return rect.buf


# The model's grid is [camera X][camera Y, downwards][depth]: looking along axis 1 from its low end is looking down from above.  Depth on the
# picture's rows, reversed so that it grows upwards, X on its columns growing to the right.
BEV = dict(axis=1, from_high=False, flip=(False, True), transpose=True)


def bird_eye_view(bits_or_dense: torch.Tensor, grid_size: Sequence[int], class_2_color, num_classes: int = 3, zoom: int = 2, shade: int = 128,
                  background=(32, 32, 32)) -> torch.Tensor:
    """occupancy_view from above for the model's grid: u8 [rows, g2 * zoom, g0 * zoom, 3], camera X to the right, depth (axis 2) upwards."""
    return occupancy_view(bits_or_dense, grid_size, class_2_color, num_classes=num_classes, zoom=zoom, shade=shade, background=background, **BEV)


def bev_iou(pred: torch.Tensor, gt: torch.Tensor, grid_size: Sequence[int], num_classes: int = 3, axis: int = 1) -> dict:
    """2-D IoU of two grids seen along `axis`: class c occupies a column when any voxel of the column has it.  pred may have one row against several
    gt rows.  Returns the dict shape of occupancy_iou with `iou_2D` for `iou_3D`: counts [rows,C,4] int64 (intersection, union, pred, gt) over the
    columns, iou_per_class = inter / (union + 1e-7) in f64, iou_2D its mean over the classes, precision, recall; an empty union gives 0."""
    C = int(num_classes)
    pb, g = _grid_bits(pred, grid_size, C, "bev_iou(pred)")
    gb, _ = _grid_bits(gt, grid_size, C, "bev_iou(gt)")
    if pb.shape[0] not in (1, gb.shape[0]) or pb.device != gb.device:
        raise ValueError("bev_iou: pred must have one row or as many as gt, on the same device")
    pc = _columns(pb, g, C, axis, False, want=("classes",))["classes"]
    gc = _columns(gb, g, C, axis, False, want=("classes",))["classes"]
    rows = gb.shape[0]
    counts = torch.empty((rows, C, 4), dtype=torch.int64, device=gb.device)
    _call("soccdpt_occ_view_iou2d", _ptr(pc), pb.shape[0], _ptr(gc), rows, gc.shape[1] * gc.shape[2], C, _ptr(counts), device=gb.device)
    c = counts.double()
    inter, union, npred, ngt = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    iou = inter / (union + 1e-7)
    return dict(counts=counts, iou_per_class=iou, iou_2D=iou.sum(dim=1) / C, precision=inter / (npred + 1e-7), recall=inter / (ngt + 1e-7))


def _camera(voxel_to_camera, intrinsics) -> Tuple[np.ndarray, np.ndarray]:
    M = np.ascontiguousarray(np.asarray(voxel_to_camera, dtype=np.float64))
    if M.shape != (3, 4):
        raise ValueError("voxel_to_camera is a 3 x 4 matrix (voxel-centre index -> camera metres)")
    K = np.asarray(intrinsics, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    if K.shape != (4,):
        raise ValueError("intrinsics are (fx, fy, cx, cy) or the 3 x 3 camera matrix")
    return M, np.ascontiguousarray(K)


def default_half_extent(voxel_to_camera) -> float:
    """Half the largest cell edge in metres: the columns of the matrix's 3 x 3 part are the camera-space steps of one voxel along each grid axis."""
    return float(np.linalg.norm(np.asarray(voxel_to_camera, dtype=np.float64)[:, :3], axis=0).max() / 2.0)


def occupancy_zbuffer(bits: torch.Tensor, g, C: int, M: np.ndarray, K: np.ndarray, half_extent_m: float, max_radius_px: int, z_near: float, H: int,
                      W: int) -> torch.Tensor:
    """soccdpt_occ_view_splat: [rows,H,W] int64 keys (bits of the f32 depth << 32 | cell index; -1 where no voxel landed)."""
    zbuf = torch.empty((bits.shape[0], H, W), dtype=torch.int64, device=bits.device)
    f64 = ctypes.POINTER(ctypes.c_double)
    _call("soccdpt_occ_view_splat", _ptr(bits), bits.shape[0], _i32x3(g), C, M.ctypes.data_as(f64), K.ctypes.data_as(f64), float(half_extent_m),
          int(max_radius_px), float(z_near), H, W, _ptr(zbuf), device=bits.device)
    return zbuf


def _overlay_into(bits: torch.Tensor, g, C: int, frames: Optional[torch.Tensor], H: int, W: int, M: np.ndarray, K: np.ndarray, table: torch.Tensor, alpha: int,
                  half_extent_m: Optional[float], max_radius_px: int, z_near: float, rect: _Rect) -> None:
    rows = bits.shape[0]
    if frames is not None and (frames.shape[0] not in (1, rows) or tuple(frames.shape[1:3]) != (H, W) or frames.device != bits.device):
        raise ValueError(f"occupancy_overlay: frames are [1 or {rows}, {H}, {W}, 3] on the grid's device, got {tuple(frames.shape)}")
    half = default_half_extent(M) if half_extent_m is None else float(half_extent_m)
    zbuf = occupancy_zbuffer(bits, g, C, M, K, half, max_radius_px, z_near, H, W)
    _call("soccdpt_occ_view_resolve", _ptr(zbuf), _ptr(frames), 1 if frames is None else frames.shape[0], rows, H, W, C, _ptr(table), int(alpha), _ptr(rect.buf),
          *rect.args, device=bits.device)


def occupancy_overlay(bits_or_dense: torch.Tensor, frames_bgr: Optional[torch.Tensor], voxel_to_camera, intrinsics, grid_size: Sequence[int], class_2_color,
                      num_classes: int = 3, alpha: int = 160, half_extent_m: Optional[float] = None, max_radius_px: int = 12, z_near: float = 0.1,
                      size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The grid over the camera frame -> u8 [rows, H, W, 3].  frames_bgr u8 [H,W,3] or [1 or rows,H,W,3] (cuda), or None with size=(H, W) for a black
    background.  voxel_to_camera: 3 x 4 float64, voxel-centre index (i + 0.5) -> camera metres (SOccDPT.voxel_to_camera()); intrinsics (fx, fy, cx, cy)
    or the 3 x 3 matrix.  Every occupied (voxel, class) in front of z_near is drawn as a square of half-width min(max_radius_px, floor(half_extent_m / Z * fx))
    pixels around its projected centre; per pixel the nearest one wins (at equal f32 depth the lower cell index) and its class colour is blended
    over the frame with weight alpha / 256.  half_extent_m=None: half the largest cell edge.  Colours are written in the channel order given."""
    bits, g = _grid_bits(bits_or_dense, grid_size, num_classes, "occupancy_overlay")
    M, K = _camera(voxel_to_camera, intrinsics)
    frames = None
    if frames_bgr is not None:
        frames, _ = _u8_image(frames_bgr, "occupancy_overlay(frames_bgr)")
        H, W = int(frames.shape[1]), int(frames.shape[2])
    elif size is not None:
        H, W = int(size[0]), int(size[1])
    else:
        raise ValueError("occupancy_overlay: without frames give size=(H, W)")
    rect = _Rect.whole(bits.shape[0], H, W, bits.device)
    _overlay_into(bits, g, int(num_classes), frames, H, W, M, K, _table(class_2_color, int(num_classes), bits.device), alpha, half_extent_m, max_radius_px, z_near, rect)
    return rect.buf


def occupancy_panel(frame_bgr: torch.Tensor, pred_bits: torch.Tensor, gt_bits: Optional[torch.Tensor] = None, *, voxel_to_camera, intrinsics,
                    grid_size: Sequence[int], class_2_color, num_classes: int = 3, alpha: int = 160, half_extent_m: Optional[float] = None,
                    max_radius_px: int = 12, z_near: float = 0.1, zoom: Optional[int] = None, shade: int = 128, background=(32, 32, 32)) -> torch.Tensor:
    """One picture of one frame's grid, u8 RGB (cuda) like evaluation_panel:

        [overlay(pred) | overlay(gt)]
        [   bev(pred)  |   bev(gt)  ]      one column without gt_bits

    frame_bgr u8 [H,W,3]; pred_bits / gt_bits one grid each (packed or dense); class_2_color in the frame's channel order.  Every tile is W-wide or
    wider and is painted straight into the panel through its destination rectangle -- no concatenation pass; pixels no tile covers are black.
    zoom=None: the largest bird's-eye zoom that fits the frame's width."""
    frame, _ = _u8_image(frame_bgr, "occupancy_panel(frame_bgr)")
    if frame.shape[0] != 1:
        raise ValueError("occupancy_panel: one frame [H,W,3]")
    C = int(num_classes)
    grids = [_grid_bits(pred_bits, grid_size, C, "occupancy_panel(pred_bits)")]
    if gt_bits is not None:
        grids.append(_grid_bits(gt_bits, grid_size, C, "occupancy_panel(gt_bits)"))
    if any(b.shape[0] != 1 or b.device != frame.device for b, _ in grids):
        raise ValueError("occupancy_panel: one grid each for the prediction and the ground truth, on the frame's device")
    g = grids[0][1]
    M, K = _camera(voxel_to_camera, intrinsics)
    H, W = int(frame.shape[1]), int(frame.shape[2])
    zoom = max(1, W // g[0]) if zoom is None else int(zoom)
    bh, bw = view_size(g, zoom=zoom, axis=BEV["axis"], transpose=BEV["transpose"])
    tw = max(W, bw)
    panel = torch.zeros((H + bh, tw * len(grids), 3), dtype=torch.uint8, device=frame.device)
    rgb = frame.flip(-1).contiguous()                       # the one frame, R <-> B once: the tiles are then painted in RGB
    table = _table(class_2_color, C, frame.device, reverse=True)
    for k, (bits, _) in enumerate(grids):
        _overlay_into(bits, g, C, rgb, H, W, M, K, table, alpha, half_extent_m, max_radius_px, z_near, _Rect.tile(panel, 0, k * tw + (tw - W) // 2))
        _view_into(bits, g, C, table, BEV["axis"], BEV["from_high"], zoom, shade, tuple(background)[::-1], BEV["flip"], BEV["transpose"],
                   _Rect.tile(panel, H, k * tw + (tw - bw) // 2))
    return panel


def model_voxel_to_camera(grid_size: Sequence[int], occupancy_shape: Sequence[float], rot27: Sequence[float]) -> np.ndarray:
    """The 3 x 4 float64 matrix of SOccDPT.voxel_to_camera(): the model voxelises q = p . Ra . Rb . Rc (row vectors) as
    ijk = trunc(q / occupancy_shape * grid_size), so a voxel centre is q_c = (ijk + 0.5) * occupancy_shape / grid_size and p = q_c . (Ra Rb Rc)^-1."""
    r = np.asarray(rot27, dtype=np.float64).reshape(3, 3, 3)
    R = r[0] @ r[1] @ r[2]
    cell = np.asarray(occupancy_shape, dtype=np.float64)[:3] / np.asarray(grid_size, dtype=np.float64)[:3]
    return np.concatenate([np.linalg.inv(R).T @ np.diag(cell), np.zeros((3, 1))], axis=1)


def processor_voxel_to_camera(grid_size: Sequence[int], occupancy_shape: Sequence[float], pc_scale: Sequence[float], pc_shift: Sequence[float],
                              rot27_t: Sequence[float]) -> np.ndarray:
    """The 3 x 4 float64 matrix of OccupancyProcessor.voxel_to_camera(): the generator voxelises q = (p * pc_scale + pc_shift) . Ra^T . Rb^T . Rc^T
    (rot27_t holds the three transposes, as the processor keeps them); the inverse is un-rotate, un-shift, un-scale."""
    t = np.asarray(rot27_t, dtype=np.float64).reshape(3, 3, 3)
    T = t[0] @ t[1] @ t[2]
    cell = np.asarray(occupancy_shape, dtype=np.float64)[:3] / np.asarray(grid_size, dtype=np.float64)[:3]
    inv_scale = np.diag(1.0 / np.asarray(pc_scale, dtype=np.float64)[:3])
    lin = inv_scale @ np.linalg.inv(T).T @ np.diag(cell)
    return np.concatenate([lin, -(inv_scale @ np.asarray(pc_shift, dtype=np.float64)[:3]).reshape(3, 1)], axis=1)
