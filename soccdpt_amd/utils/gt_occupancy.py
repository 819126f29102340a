"""Ground-truth occupancy generator on the GPU with the constructor of the reference's
`OccupancyProcessor` (/root/reference/SOccDPT/datasets/bdd_helper.py:238-285).  The reference processes one frame at a time in
numpy on the host (2 M points, ~0.5 s per 1080p frame); here a batch of disparity frames and class maps that already sit in HBM
becomes depth, the rotated point cloud and the thresholded counting grid in two launches (csrc/gt_occ.hip).

What stays on the host, outside this boundary: decoding images (soccdpt_amd/datasets/bdd_helper.py) and the colourised point cloud used for
visualisation (:491-521).  `rgb_seg_to_class` (colour -> class id, :10-25) is a kernel too: the `class_map` output of soccdpt_data_targets
(csrc/batch_targets.hip, include/soccdpt_data.h) builds `seg_class` from the uint8 label frames of a batch, which is where `eval_SOccDPT --occupancy`
takes it from on real recordings.  The `occupancy_points` list of transform_points_to_occupancy_grid_vect (:339-355)
is available on request (`want_occupancy_points`, csrc/occ_eval.hip); the un-rotation / un-shift / un-scale that process_frame applies to it
afterwards for drawing (:500-528, numpy matmuls on the host) is `voxel_to_camera()`: one 3 x 4 matrix that utils/occupancy_views.py hands to the
overlay kernels, which draw the cells over the camera frame without a point list."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from ..lib import _call, _ptr


class OccupancyProcessor:
    def __init__(self, intrinsic_matrix, height: int, width: int, grid_size: Sequence[int], scale: Sequence[float], shift: Sequence[float],
                 pc_scale: Sequence[float], pc_shift: Sequence[float], point_count_threshold: float, class_2_color=None, color_2_class=None,
                 num_classes: int = 3, correction_angle: Sequence[float] = (7.0, 0.0, 0.0)) -> None:
        K = np.asarray(intrinsic_matrix, dtype=np.float64)
        self.height, self.width, self.num_classes = int(height), int(width), int(num_classes)
        self.class_2_color, self.color_2_class = class_2_color, color_2_class
        self.grid_size, self.scale, self.shift = tuple(int(g) for g in grid_size), tuple(scale), tuple(shift)
        self.pc_scale, self.pc_shift = tuple(float(v) for v in pc_scale), tuple(float(v) for v in pc_shift)
        self.point_count_threshold = float(point_count_threshold)
        self.occupancy_shape = np.array([float(self.grid_size[i] / self.scale[i]) for i in range(3)], dtype=np.float32)   # :264-270
        self.baseline = 1.0 * 10**-2                                                                                      # :274
        self.fx, self.fy, self.cx, self.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
        a, b, c = [math.radians(v) for v in correction_angle]                                                             # rotate_points, :604-652
        Ra = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
        Rb = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
        Rc = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
        self._rot = np.concatenate([Ra.T.reshape(-1), Rb.T.reshape(-1), Rc.T.reshape(-1)]).astype(np.float64)

    def voxel_to_camera(self) -> np.ndarray:
        """3 x 4 float64: voxel-centre index (i + 0.5 per axis) of this generator's grid -> camera coordinates in metres: the inverse of scale
        (pc_scale), shift (pc_shift), rotate and / occupancy_shape * grid_size -- what process_frame undoes for drawing (bdd_helper.py:500-524)."""
        from .occupancy_views import processor_voxel_to_camera
        return processor_voxel_to_camera(self.grid_size, self.occupancy_shape, self.pc_scale, self.pc_shift, self._rot)

    def observed_voxels(self, depth: torch.Tensor, **kw) -> torch.Tensor:
        """utils.occupancy_rays.observed_voxels of `depth` [B,H,W] (process's output of that name) with this generator's voxel_to_camera() and
        intrinsics: the voxel mask int32 [B, ceil(g0 g1 g2 / 32)] of the space the camera saw.  Keywords: z_near=, max_depth=, step=, out=."""
        from .occupancy_rays import observed_voxels
        return observed_voxels(depth, self.voxel_to_camera(), (self.fx, self.fy, self.cx, self.cy), self.grid_size, **kw)

    def process(self, disparity: torch.Tensor, seg_class: torch.Tensor, want_points: bool = True, want_depth: bool = True,
                want_occupancy_points: bool = False, want_observed: bool = False) -> Dict[str, Optional[torch.Tensor]]:
        """disparity [B,H,W] (or [H,W]) float, seg_class same shape integer class ids, both cuda ->
        depth [B,H,W] f32, points [B,H*W,3] f64, occupancy_grid [B,g0,g1,g2,C] bool, counts [B,g0,g1,g2,C] int32.
        want_occupancy_points adds `occupancy_points`: a list of B float64 [N_b,4] tensors (x, y, z, class_id), the value
        transform_points_to_occupancy_grid_vect returns under that key (cells with counts >= point_count_threshold, class-major; bdd_helper.py:339-355),
        built on the GPU from `counts`.  want_observed adds `observed`: observed_voxels(depth), the voxel mask [B, ceil(g0 g1 g2 / 32)] int32 of the
        space this frame's rays crossed (utils/occupancy_rays.py).  process_frame's later un-rotate / un-shift / un-scale of that list (:500-528, drawing only) is not applied to it: voxel_to_camera() is that mapping."""
        assert disparity.is_cuda, "the HIP path needs cuda tensors (no CPU fallback)"
        if disparity.dim() == 2:
            disparity, seg_class = disparity.unsqueeze(0), seg_class.unsqueeze(0)
        B, H, W = disparity.shape
        assert (H, W) == (self.height, self.width) and tuple(seg_class.shape) == (B, H, W)
        dev = disparity.device
        d = disparity.detach().to(torch.float32).contiguous()
        sc = seg_class.detach().to(torch.int32).contiguous()
        g = self.grid_size
        depth = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_depth or want_observed else None
        pts = torch.empty((B, H * W, 3), dtype=torch.float64, device=dev) if want_points else None
        counts = torch.empty((B, g[0], g[1], g[2], self.num_classes), dtype=torch.int32, device=dev)
        occ = torch.empty((B, g[0], g[1], g[2], self.num_classes), dtype=torch.uint8, device=dev)
        arr = lambda vals, t: (t * len(vals))(*vals)
        intr = arr([self.fx, self.fy, self.cx, self.cy, self.baseline], ctypes.c_double)
        _call("soccdpt_gt_occupancy", B, H, W, self.num_classes, intr, arr(self.pc_scale, ctypes.c_double), arr(self.pc_shift, ctypes.c_double),
              arr([float(v) for v in self._rot], ctypes.c_double), arr([float(v) for v in self.occupancy_shape], ctypes.c_float),
              arr(list(g), ctypes.c_int), self.point_count_threshold, _ptr(d), _ptr(sc), _ptr(depth), _ptr(pts),
              _ptr(counts), _ptr(occ), device=dev)
        out = dict(depth=depth if want_depth else None, points=pts, occupancy_grid=occ.bool(), counts=counts)
        if want_observed:
            out["observed"] = self.observed_voxels(depth)
        if want_occupancy_points:
            from .occupancy import occupancy_bits_to_points, pack_occupancy
            bits = pack_occupancy(counts, self.point_count_threshold, strict=False)           # the list uses >=, the grid above >
            res = occupancy_bits_to_points(bits, g, self.scale, num_classes=self.num_classes, rows=B)
            out["occupancy_points"] = list(torch.split(res.points, res.counts.sum(dim=1).tolist()))
        return out
