"""SOccDPT model API on MI355X: same classes, constructor arguments, forward signature and
return shapes as /root/reference/SOccDPT/model/SOccDPT.py, with the arithmetic in
libsoccdpt_hip.so (no CPU / eager-PyTorch fallback).

  SOccDPT              base: constants + calibration (:134-245), get_semantic_occupancy (:264-372)
  SOccDPT_V3           depth_net (DPTDepthModel) + seg_head + projection (:626-685)
  SOccDPT_versions     {3: SOccDPT_V3}; V1/V2 are out of scope of the hot path
  DepthNet / SegNet    output selectors (:697-724)
"""
from __future__ import annotations

import os
from typing import Optional, Type

import numpy as np
import torch
import torch.nn as nn
import yaml

from ..lib import PREC_BF16, PREC_MIXED, Engine, make_config
from .base_model import BaseModel
from .blocks import Interpolate
from .dpt import DPTDepthModel
from .scaled_tanh import ScaledTanh
from .spec import DEFAULT_DEPTH_WEIGHTS, HYBRID_ARCHS, MODEL_TYPE_TO_BACKBONE, SWIN1_ARCHS, SWIN_ARCHS, VIT_ARCHS, backbone_image_size, model_types  # noqa: F401

# /root/reference/SOccDPT/datasets/bdd_helper.py:53-56
DATASET_BASE = "~/Datasets/Depth_Dataset_Bengaluru"
DEFAULT_CALIB = os.path.join(DATASET_BASE, "calibration/pocoX3/calib.yaml")

cpu_device = torch.device("cpu")
default_depth_models = dict(DEFAULT_DEPTH_WEIGHTS)
default_seg_models = {k: None for k in default_depth_models}
DEPTH_l39icv3q = "checkpoints_pretrained/depth_dpt_hybrid/l39icv3q/checkpoint_epoch15.pth"  # noqa: E501


class SOccDPT(BaseModel):
    def __init__(self, model_type="dpt_swin2_tiny_256", backbone="swin2t16_256", path=None, num_classes: int = 3,
                 camera_intrinsics_yaml=DEFAULT_CALIB, point_compute_method="torch",
                 grid_size=(256, 256, 32), scale=(2.0, 2.0, 0.666), shift=(0.0, 0.0, 0.0),
                 pc_scale=(10000.0, 50000.0, 800.0), pc_shift=(55.0, -20.0, 15.0), correction_angle=(7.0, 0, 0),
                 compute_occ=False, precision: int = PREC_MIXED, streams: int = 1, graph: bool = False, share_occupancy_rows: bool = False,
                 occupancy_per_frame: bool = False, **kwargs):
        super().__init__()
        self.compute_occ = compute_occ
        self.share_occupancy_rows = bool(share_occupancy_rows)   # occupancy returned as a stride-0 expand of one row (read-only callers)
        # opt-in: row b of the occupancy output is the grid of frame b ALONE (what the reference computes for that frame as a batch of one) instead
        # of the union over the batch in every row; the packed rows are kept in last_occ_frame_bits, last_occ_bits stays the union
        self.occupancy_per_frame = bool(occupancy_per_frame)
        assert not (self.occupancy_per_frame and self.share_occupancy_rows), \
            "occupancy_per_frame gives every batch row its own grid; share_occupancy_rows returns one shared row: choose one"
        self.grid_size = grid_size
        self.scale = scale
        self.shift = shift
        self.pc_scale = pc_scale
        self.pc_shift = pc_shift
        self.correction_angle = correction_angle
        self.backbone = backbone
        self.model_type = model_type
        self.path = path
        self.num_classes = num_classes
        # arithmetic of the GEMMs / convolutions.  Default since round 4: PREC_MIXED (fp16 MFMA operands, x3 split where the shipped precision map
        # asks for it) -- the fastest mode that keeps depth, logits and features within half the north star's 1e-3 of the reference's fp32
        # forward (model/loader.py:126-139 computes in fp32 unless optimize=True); PREC_BF16 is the fast 3e-3 mode, PREC_F16 what optimize=True selects
        self.precision = precision
        self.streams = int(streams)  # sub-batches of one forward run concurrently on this many HIP streams
        self.graph = bool(graph)     # replay the network's launch sequence as a hipGraph when pointers repeat
        self.occupancy_shape = np.array([float(grid_size[i] / scale[i]) for i in range(len(grid_size))], dtype=np.float32)
        self.features = kwargs["features"] if "features" in kwargs else 256
        assert point_compute_method in ("torch", "numpy")
        assert point_compute_method == "torch", "the MI355X path fuses the 'torch' point computation"
        self.point_compute_method = point_compute_method
        # camera intrinsics (a missing file raises FileNotFoundError like the reference)
        self.camera_intrinsics_yaml = os.path.expanduser(camera_intrinsics_yaml)
        with open(self.camera_intrinsics_yaml, "r") as stream:
            try:
                self.cam_settings = yaml.load(stream, Loader=yaml.FullLoader)
            except yaml.YAMLError as exc:
                print(exc)
        cs = self.cam_settings
        k3 = cs["Camera.k3"] if "Camera.k3" in cs else 0
        self.DistCoef = np.array([cs["Camera.k1"], cs["Camera.k2"], cs["Camera.p1"], cs["Camera.p2"], k3])
        self.intrinsic_matrix = np.array([[cs["Camera.fx"], 0.0, cs["Camera.cx"]], [0.0, cs["Camera.fy"], cs["Camera.cy"]],
                                          [0.0, 0.0, 1.0]])
        self.fx = self.intrinsic_matrix[0, 0]
        self.fy = self.intrinsic_matrix[1, 1]
        self.cx = self.intrinsic_matrix[0, 2]
        self.cy = self.intrinsic_matrix[1, 2]
        self.width = cs["Camera.width"]
        self.height = cs["Camera.height"]
        self.occupancy_conv = nn.Identity()
        # ---- MI355X engine state (one handle per device, created lazily) ----
        self._engines = {}
        self._bound_versions = {}
        self._weight_refs = {}
        self.occ_exchange = None  # set by soccdpt_amd.dist for multi-GPU: callable(bits) -> union bits
        self.grad_exchange = None  # set by soccdpt_amd.dist.attach_training: callable(flat_grads, runs) -> averaged in place
        self.last_occ_bits = None        # packed union grid of the last forward with compute_occ (_finish_occupancy)
        self.last_occ_frame_bits = None  # its packed per-frame rows; None in union mode
        self._warned_uncalibrated = False
        # ---- training step state ----
        self.train_amp = False      # the reference's `amp` sweep parameter: False | True / "bf16" | "f16" (with a GradScaler) | "x3"
        self._train_state = {}      # id(engine) -> bound pointers, the flat gradient buffer and its views (_bind_for_training)
        self._train_x = None        # (engine, input) of the train_forward that backward() belongs to
        self._train_generation = 0  # counts train-mode forwards: the library keeps one tape per handle
        self._last_grad_runs = None  # (engine, flat gradients, runs) of the last backward (utils/optim.py GradScaler)
        self._autograd_anchor = None  # a plain tensor attribute: never a parameter or buffer, so state_dict() does not see it

    # -- engine plumbing --
    def _engine_backbone(self) -> str:
        return self.backbone if (self.backbone in SWIN_ARCHS or self.backbone in SWIN1_ARCHS or self.backbone in HYBRID_ARCHS or self.backbone in VIT_ARCHS) else "swin2t16_256"

    def _sigmoid_flag(self) -> bool:
        return True

    def _engine(self, device: torch.device) -> Engine:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("soccdpt_amd runs on MI355X only: move the model and inputs to a cuda device "
                               "(there is no CPU fallback)")
        key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
        eng = self._engines.get(key)
        if eng is None:
            cfg = make_config(self._engine_backbone(), self.num_classes, self.features, self._sigmoid_flag(),
                              bool(self.compute_occ), self.width, self.height, self.fx, self.fy, self.cx, self.cy,
                              self.grid_size, self.occupancy_shape, self.pc_scale, self.pc_shift, self.correction_angle,
                              precision=self.precision)
            eng = Engine(cfg, torch.device(key[0], key[1]))
            if self.streams > 1:
                eng.set_streams(self.streams)
            if self.graph:
                eng.set_graph(True)
            self._engines[key] = eng
        return eng

    def forward(self, x: torch.Tensor):
        assert False, "Not implemented, take input batch and produce inv_depth, segmentation and call " \
                      "self.get_semantic_occupancy(inv_depth, segmentation)"

    def _shape_outputs(self, inv_up, seg_up, points, occ):
        # .squeeze() quirk of model/SOccDPT.py:276-285: B == 1 -> segmentation loses its batch dim
        if seg_up.shape[0] == 1:
            seg_up = seg_up[0]
        return inv_up, seg_up, points, occ

    def _camera_outputs(self, B: int, dev: torch.device):
        """The camera-resolution outputs of one forward, uninitialised: inv_up [B,Hc,Wc], seg_up [B,C,Hc,Wc], points [B,Hc,Wc,3]."""
        Hc, Wc = self.height, self.width
        return (torch.empty((B, Hc, Wc), device=dev), torch.empty((B, self.num_classes, Hc, Wc), device=dev), torch.empty((B, Hc, Wc, 3), device=dev))

    def _project_outputs(self, eng: Engine, inv: torch.Tensor, seg: torch.Tensor):
        """Network outputs inv [B,h,w], seg [B,C,h,w] -> (inv_up, seg_up, points, packed union grid | None) by soccdpt_project.  The union grid is
        marked here in union mode only: with occupancy_per_frame it comes from the frame rows (_finish_occupancy)."""
        inv_up, seg_up, points = self._camera_outputs(inv.shape[0], inv.device)
        union = self.compute_occ and not self.occupancy_per_frame
        bits = torch.empty((eng.occ_words(),), dtype=torch.int32, device=inv.device) if union else None
        eng.project(inv, seg, inv_up, seg_up, points, bits, clear_bits=True)
        return inv_up, seg_up, points, bits

    def get_semantic_occupancy(self, inv_depth: torch.Tensor, segmentation: torch.Tensor):
        """inv_depth [B,h,w] (or [B,1,h,w]), segmentation [B,C,h,w] on a cuda device ->
        (inv_depth_up [B,Hc,Wc], seg_up [B,C,Hc,Wc] | [C,Hc,Wc], points [B,Hc,Wc,3], occupancy | None)."""
        if inv_depth.dim() == 4:
            inv_depth = inv_depth[:, 0]
        eng = self._engine(inv_depth.device)
        inv = inv_depth.detach().to(torch.float32).contiguous()
        seg = segmentation.detach().to(torch.float32).contiguous()
        inv_up, seg_up, points, bits = self._project_outputs(eng, inv, seg)
        occ = self._finish_occupancy(eng, inv.shape[0], bits, inv_up=inv_up, seg=seg) if self.compute_occ else None
        return self._shape_outputs(inv_up, seg_up, points, occ)

    def _finish_occupancy(self, eng: Engine, B: int, bits, inv_up=None, seg=None, occ=None, frame_bits=None):
        """The one way from the projection to the occupancy tensor [B,g0,g1,g2,C], and the only place that publishes last_occ_bits /
        last_occ_frame_bits.  bits: the packed union grid soccdpt_project / soccdpt_forward marked (None with occupancy_per_frame after
        _project_outputs: the frame rows are voxelised here from inv_up and seg).  occ / frame_bits: what the fused eng.forward /
        eng.forward_frames already wrote; those steps are then not repeated."""
        g, dev = self.grid_size, (bits if bits is not None else inv_up).device
        ex = self.occ_exchange   # multi-GPU: union over every rank's frames
        split = ex is not None and hasattr(ex, "start")
        if self.occupancy_per_frame:
            if frame_bits is None:
                # one grid per frame from the projection's clamped inverse depth and the network-resolution class maps (soccdpt_voxelise_frames),
                # dense rows from their own bits, the union of the rows as last_occ_bits
                frame_bits = torch.empty((B, eng.occ_words()), dtype=torch.int32, device=dev)
                eng.voxelise_frames(inv_up, seg, frame_bits, clear_bits=True)
                bits = torch.zeros((eng.occ_words(),), dtype=torch.int32, device=dev)
                eng.occ_or(bits, frame_bits, B)
                occ = torch.empty((B, g[0], g[1], g[2], self.num_classes), device=dev)
                eng.occ_expand_frames(frame_bits, B, occ)
            # the per-frame rows are rank-local and stay here; only the union goes through the exchange, as in union mode
            if ex is not None:
                bits = ex.finish(eng, bits, ex.start(bits)) if split else ex(eng, bits)
        elif occ is None:
            rows = 1 if self.share_occupancy_rows else B
            occ = torch.empty((rows, g[0], g[1], g[2], self.num_classes), device=dev)
            if split:
                # The all-gather of the packed grids runs on RCCL's stream while this stream writes the rows' zeros (the bulk of the
                # expansion's 25 MB per row); after the OR only the set voxels are written.
                ticket = ex.start(bits)
                eng.occ_zero(rows, occ)
                bits = ex.finish(eng, bits, ticket)
                eng.occ_set(bits, rows, occ)
            else:
                if ex is not None:
                    bits = ex(eng, bits)
                eng.occ_expand(bits, rows, occ)
            # opt-in: ONE dense row viewed B times (stride 0).  The reference writes the same union grid into every batch row
            # (/root/reference/SOccDPT/model/SOccDPT.py:449-455); a caller that only reads it saves (B - 1) x 25 MB of stores per step.
            if self.share_occupancy_rows:
                occ = occ.expand(B, -1, -1, -1, -1)
        self.last_occ_bits = bits
        self.last_occ_frame_bits = frame_bits
        return occ

    def _last_bits(self, frame, what: str) -> torch.Tensor:
        """The packed grid of the last forward: the union (frame=None) or frame b's own row; RuntimeError when there is none."""
        if frame is not None:
            rows = self.last_occ_frame_bits
            if not self.occupancy_per_frame or rows is None:
                raise RuntimeError(f"{what}(frame=...) needs a forward of a model built with compute_occ=True and occupancy_per_frame=True")
            return rows[int(frame)]
        if self.last_occ_bits is None:
            raise RuntimeError(f"{what}() needs a forward of a model built with compute_occ=True first")
        return self.last_occ_bits

    def occupancy_points(self, class_2_color=None, frame=None):
        """The last forward's occupancy grid as the reference's point list (utils/__init__.py:532-568 occupancy_grid_to_points on occupancy[0]):
        float64 [N,4] rows (x, y, z, class_id) in metres, class-major, straight from the packed bits `last_occ_bits` -- no dense grid is read,
        so it works the same with share_occupancy_rows=True and under occ_exchange.  With class_2_color also the [N,3] u8 colours.
        frame=None lists the union grid; frame=b (a model built with occupancy_per_frame=True) lists frame b's own grid from `last_occ_frame_bits`."""
        bits = self._last_bits(frame, "occupancy_points")
        from ..utils.occupancy import occupancy_bits_to_points
        res = occupancy_bits_to_points(bits, self.grid_size, self.scale, num_classes=self.num_classes, class_2_color=class_2_color)
        return res.points if class_2_color is None else (res.points, res.colors)

    def voxel_to_camera(self) -> np.ndarray:
        """3 x 4 float64: voxel-centre index (i + 0.5 per axis) of this model's grid -> camera coordinates in metres, composed on the host from the
        model's own constants: the inverse of p . Ra . Rb . Rc followed by / occupancy_shape * grid_size (model/SOccDPT.py:374-463 of the reference).
        The reference scales and shifts the first three POINTS of the cloud by pc_scale / pc_shift (an indexing quirk, :351-353, which the forward
        path reproduces); those three points are ignored here: pc_scale and pc_shift do not enter the matrix."""
        from ..lib import host_rotation_matrices
        from ..utils.occupancy_views import model_voxel_to_camera
        return model_voxel_to_camera(self.grid_size, self.occupancy_shape, host_rotation_matrices(self.correction_angle))

    def occupancy_view(self, frame=None, class_2_color=None, **kw) -> torch.Tensor:
        """utils.occupancy_views.bird_eye_view of the last forward's grid (`last_occ_bits`; frame=b: frame b's own grid, as in occupancy_points):
        u8 [1, g2 * zoom, g0 * zoom, 3].  Keywords of occupancy_view (axis=, from_high=, flip=, transpose=, ...) replace the bird's-eye defaults."""
        from ..utils.occupancy_views import BEV, occupancy_view
        bits = self._last_bits(frame, "occupancy_view")
        return occupancy_view(bits, self.grid_size, class_2_color or self._dataset_colors(), num_classes=self.num_classes, **{**BEV, **kw})

    def occupancy_overlay(self, frames_bgr, frame=None, class_2_color=None, **kw) -> torch.Tensor:
        """utils.occupancy_views.occupancy_overlay of the last forward's grid over camera frames u8 [H,W,3] / [1,H,W,3] (cuda), through
        voxel_to_camera() and the model's intrinsics: u8 [1, H, W, 3].  frame= as in occupancy_points."""
        from ..utils.occupancy_views import occupancy_overlay
        bits = self._last_bits(frame, "occupancy_overlay")
        return occupancy_overlay(bits, frames_bgr, self.voxel_to_camera(), (self.fx, self.fy, self.cx, self.cy), self.grid_size,
                                 class_2_color or self._dataset_colors(), num_classes=self.num_classes, **kw)

    def observed_voxels(self, depth, **kw) -> torch.Tensor:
        """utils.occupancy_rays.observed_voxels of a depth map [B,H,W] in camera metres (cuda) through voxel_to_camera() and the model's intrinsics:
        the voxel mask int32 [B, ceil(g0 g1 g2 / 32)] of the space a camera with that depth map saw in this model's grid, for
        occupancy_iou_observed / apply_observed.  Keywords: z_near=, max_depth=, step=, out=."""
        from ..utils.occupancy_rays import observed_voxels
        return observed_voxels(depth, self.voxel_to_camera(), (self.fx, self.fy, self.cx, self.cy), self.grid_size, **kw)

    def _dataset_colors(self):
        """The Bengaluru dataset's class colours, the default of the two pictures above; other class counts have to bring their own."""
        from ..datasets.bengaluru_driving_dataset import class_2_color
        if self.num_classes != len(class_2_color):
            raise ValueError(f"pass class_2_color: the default table has {len(class_2_color)} classes, the model {self.num_classes}")
        return class_2_color


class SOccDPT_V3(SOccDPT):
    def __init__(self, sigmoid=True, load_depth: str = DEPTH_l39icv3q, **kwargs):
        super().__init__(**kwargs)
        from .loader import load_model

        depth_model_weights = load_depth
        if depth_model_weights is None:
            depth_model_weights = default_depth_models[self.model_type]
        print("Loading depth net")
        self.depth_net = load_model(DPTDepthModel, dict(non_negative=True, return_features=True), cpu_device,
                                    depth_model_weights, self.model_type)
        self.depth_net.return_features = True
        self.pretrained = self.depth_net.pretrained  # same module registered twice, like the reference (:650)
        self.sigmoid = bool(sigmoid)
        activation = nn.Sigmoid() if sigmoid else ScaledTanh()
        self.seg_head = nn.Sequential(
            nn.Conv2d(self.features, self.features, kernel_size=3, padding=1, bias=False),
            nn.BatchNorm2d(self.features),
            nn.ReLU(True),
            nn.Dropout(0.1, False),
            nn.Conv2d(self.features, self.num_classes, kernel_size=1),
            Interpolate(scale_factor=2, mode="bilinear", align_corners=True),
            activation,
        )
        # Stochastic depth under net.train(): timm 0.6.12 builds SwinTransformerV2 with drop_path_rate = 0.1 and the reference's factory
        # (model/backbones/swin2.py:15-30) does not override it; vit_base_resnet50_384 defaults to 0.  Set it to 0.0 for deterministic parity runs.
        self.drop_path_rate = 0.1 if self.depth_net.backbone in SWIN_ARCHS else 0.0
        self.load_net(self.path)

    def _engine_backbone(self) -> str:
        return self.depth_net.backbone

    def _sigmoid_flag(self) -> bool:
        return self.sigmoid

    # -- weights -> library --
    def _apply(self, fn, *args, **kwargs):
        # .to()/.cuda()/.float() replace parameter storage: forget what was bound
        self._bound_versions.clear()
        self._weight_refs.clear()
        return super()._apply(fn, *args, **kwargs)

    def _live_tensors(self, eng: Engine):
        """-> ({key: LIVE parameter / buffer}, the engine's keys in its order), every consumed tensor checked to be contiguous f32 on the engine's device."""
        live = dict(self.named_parameters(remove_duplicate=False))
        live.update(dict(self.named_buffers(remove_duplicate=False)))
        keys = eng.weight_keys()
        for k in keys:
            t = live[k]
            if t.device != eng.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"weight {k} must be a contiguous float32 tensor on {eng.device} (got {t.device}, {t.dtype})")
        return live, keys

    def _sync_weights(self, eng: Engine):
        """(Re-)bind and re-prepare when any consumed tensor changed: in-place updates bump `_version` (optimizers, the fused
        Adam, load_state_dict), `p.data = ...` changes `data_ptr()`.  The LIVE parameters / buffers are watched, not a
        state_dict() snapshot."""
        refs = self._weight_refs.get(id(eng))
        if refs is not None:
            version = tuple((t._version, t.data_ptr()) for t in refs)
            if self._bound_versions.get(id(eng)) == version:
                return
        live, keys = self._live_tensors(eng)
        refs = [live[k] for k in keys]
        version = tuple((t._version, t.data_ptr()) for t in refs)
        for k, t in zip(keys, refs):
            eng.bind(k, t.detach())
        was_calibrated = self.precision == PREC_MIXED and eng.prec_map_source() == 1
        eng.prepare()
        if was_calibrated and eng.prec_map_source() == 3:
            # the library compared a fingerprint of the bound values with the one the calibration ran on (soccdpt_prepare)
            self._warned_uncalibrated = True
            print("soccdpt_amd: the weights changed since net.calibrate_precision() derived the precision map, so that map no longer carries its "
                  "within-tolerance claim: every GEMM / convolution runs x3 split-fp16 operands again until net.calibrate_precision(sample_frames) is re-run.")
        self._weight_refs[id(eng)] = refs
        self._bound_versions[id(eng)] = version
        if self.precision == PREC_MIXED and eng.prec_map_source() == 3 and not self._warned_uncalibrated:
            # printed, not raised: the reference's convention for checkpoint mismatches (model/base_model.py:30-34)
            self._warned_uncalibrated = True
            print("soccdpt_amd: these are not the weights the shipped precision map of the default arithmetic (SOCCDPT_PREC_MIXED) was derived on, so its "
                  "within-tolerance claim does not carry over: every GEMM / convolution runs x3 split-fp16 operands (f32-grade, about 1.7x the step) "
                  "until net.calibrate_precision(sample_frames, budget=5e-4) has derived a map for THIS checkpoint.")

    def forward(self, x: torch.Tensor):
        """x [B,3,S,S] f32 on cuda -> (inv_depth, segmentation, points, occupancy | None); see SOccDPT_V3.forward
        (/root/reference/SOccDPT/model/SOccDPT.py:681-685)."""
        if self.training:
            # train mode: the same 4-tuple with autograd attached, so the reference's loop body runs unchanged
            # (scripts/train_SOccDPT.py:365-393: net_patch(x), any criterion in torch ops, grad_scaler.scale(loss).backward())
            return self._forward_train(x)
        img = backbone_image_size(self._engine_backbone())
        assert x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == img and x.shape[3] == img, \
            f"expected x [B,3,{img},{img}], got {tuple(x.shape)}"
        eng = self._engine(x.device)
        self._sync_weights(eng)
        dev = x.device
        xin = x.detach().to(torch.float32).contiguous()
        B = xin.shape[0]
        inv_up, seg_up, points = self._camera_outputs(B, dev)
        occ = bits = frame_bits = None
        if self.compute_occ:
            g = self.grid_size
            bits = torch.empty((eng.occ_words(),), dtype=torch.int32, device=dev)
            # the fused calls write the dense rows themselves where every row is this rank's own: the per-frame rows always, the union rows
            # unless an exchange or the shared row comes in between (_finish_occupancy then expands the exchanged / the single row)
            if self.occupancy_per_frame or (self.occ_exchange is None and not self.share_occupancy_rows):
                occ = torch.empty((B, g[0], g[1], g[2], self.num_classes), device=dev)
        if self.compute_occ and self.occupancy_per_frame:
            frame_bits = torch.empty((B, eng.occ_words()), dtype=torch.int32, device=dev)
            eng.forward_frames(xin, inv_up, seg_up, points, occ, bits, frame_bits)
        else:
            eng.forward(xin, inv_up, seg_up, points, occ, bits)
        if self.compute_occ:
            occ = self._finish_occupancy(eng, B, bits, occ=occ, frame_bits=frame_bits)
        return self._shape_outputs(inv_up, seg_up, points, occ)

    def _forward_train(self, x: torch.Tensor):
        """SOccDPT_V3.forward under net.train(): train-mode network forward (batch-statistics BatchNorm, Dropout) -> bicubic + clamp / nearest
        up-sampling -> points (-> occupancy) exactly like the eval path, returned as autograd-tracked tensors.  loss.backward() on any torch
        expression of inv_depth / segmentation / points runs soccdpt_project_backward + soccdpt_train_backward and leaves the gradients in .grad of
        the parameters that have requires_grad (freeze / unfreeze-by-percentage / PatchWiseInplace work as with an nn.Module built from torch ops).
        The library keeps ONE tape per handle: backward belongs to the most recent train-mode forward."""
        if self._autograd_anchor is None or self._autograd_anchor.device != x.device:
            self._autograd_anchor = torch.zeros((), device=x.device, requires_grad=True)   # makes autograd record the node: the parameters are not inputs of it
        if not torch.is_grad_enabled():
            inv, seg = self.train_forward(x)
            return self.get_semantic_occupancy(inv, seg)
        out = _TrainForward.apply(self, x, self._autograd_anchor)
        return self._shape_outputs(out[0], out[1], out[2], out[3] if len(out) > 3 else None)   # (the B == 1 squeeze is a differentiable view)

    def _bind_for_training(self, eng: Engine):
        """Bind the LIVE parameters / buffers (the training step reads weights as bound: no prepare) and one gradient buffer per
        trainable parameter; frozen parameters (requires_grad False: model/loss.py:110-152) are unbound and their weight-gradient
        GEMMs skipped."""
        live, keys = self._live_tensors(eng)
        st = self._train_state.setdefault(id(eng), {"ptrs": {}, "grads": {}, "req": {}, "flat": None, "span": {}})
        if st["flat"] is None:
            # ONE flat f32 gradient buffer, a view per consumed tensor in the library's key order: a data-parallel job all-reduces contiguous runs
            # of it (soccdpt_amd.dist.attach_training) instead of one collective per tensor
            off = 0
            for k in keys:
                n = live[k].numel()
                st["span"][k] = (off, off + n)
                off += (n + 63) // 64 * 64          # 256-byte aligned views
            st["flat"] = torch.zeros(off, dtype=torch.float32, device=eng.device)
        for k in keys:
            t = live[k]
            if st["ptrs"].get(k) != t.data_ptr():
                eng.bind(k, t.detach())
                st["ptrs"][k] = t.data_ptr()
            req = bool(getattr(t, "requires_grad", False))
            if st["req"].get(k) != req:
                lo, hi = st["span"][k]
                st["grads"][k] = st["flat"][lo:hi].view(t.shape) if req else None
                eng.bind_grad(k, st["grads"][k])
                st["req"][k] = req
        # the eval path prepares from the same tensors: make it re-prepare after training touched them
        self._bound_versions.pop(id(eng), None)
        return live, keys, st

    def train_forward(self, x: torch.Tensor, seed: int = None):
        """Train-mode forward (model/SOccDPT.py:660-685 under nn.Module.train(): BatchNorm2d of the seg head on batch statistics with its
        running buffers updated, Dropout live) that keeps every activation the backward needs.  Returns (inv_depth [B,S,S],
        segmentation [B,C,S,S]) at network resolution -- what SOccDPT_V3.forward hands to the up-sampling / criterion.  Exact f32
        (precision=PREC_F32); follow it with backward(d_inv, d_seg)."""
        from ..lib import PREC_F32
        from .spec import FORWARD_ONLY_BACKBONES, train_refusal
        if self._engine_backbone() in FORWARD_ONLY_BACKBONES:   # before anything is bound or allocated for a step that does not exist
            raise RuntimeError(train_refusal(self._engine_backbone()))
        if self.precision != PREC_F32:
            raise RuntimeError("the training step is built for precision=PREC_F32 (exact-f32 MFMA); construct the model with it")
        img = backbone_image_size(self._engine_backbone())
        assert x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == img and x.shape[3] == img, f"expected x [B,3,{img},{img}], got {tuple(x.shape)}"
        eng = self._engine(x.device)
        live, keys, st = self._bind_for_training(eng)
        eng.train_set_amp(self.train_amp)
        eng.train_set_drop_path(float(self.drop_path_rate))
        xin = x.detach().to(torch.float32).contiguous()
        B = xin.shape[0]
        inv = torch.empty((B, img, img), device=x.device)
        seg = torch.empty((B, self.num_classes, img, img), device=x.device)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
            # data-parallel replicas seed torch identically (train_net: manual_seed(0)); the Dropout / DropPath masks hash (seed, block, LOCAL sample
            # index), so without the rank in the seed every rank would drop the same pattern on its shard (masks correlated over the global batch: ADVICE r3)
            import torch.distributed as _dist
            if _dist.is_available() and _dist.is_initialized() and _dist.get_world_size() > 1:
                seed = (seed + 0x9E3779B1 * (_dist.get_rank() + 1)) & 0x7FFFFFFF
        eng.train_forward(xin, inv, seg, dropout_p=float(self.seg_head[3].p), seed=seed)
        # BatchNorm bookkeeping that lives on the host side of nn.BatchNorm2d
        bn = self.seg_head[1]
        if self.grad_exchange is not None:
            self.grad_exchange.average_buffers([bn.running_mean, bn.running_var])   # keep the BatchNorm running buffers identical on every rank
        torch._C._increment_version([bn.running_mean, bn.running_var])
        bn.num_batches_tracked += 1
        self._train_x = (eng, xin)
        return inv, seg

    def backward(self, d_inv: torch.Tensor, d_seg: torch.Tensor):
        """d loss / d (inv_depth, segmentation) of the last train_forward -> .grad of every trainable parameter, accumulated like
        autograd does when .grad is already populated (no zero_grad since the previous backward).  Replaces loss.backward() of scripts/train_SOccDPT.py:390."""
        if self._train_x is None:
            raise RuntimeError("backward() needs a train_forward() first")
        eng, xin = self._train_x
        live, keys, st = self._bind_for_training(eng)
        # the library WRITES its gradient buffers: a parameter whose .grad still is that buffer (no zero_grad since the last backward: gradient
        # accumulation over micro-batches) keeps its old value aside so that the new gradient can be added like autograd does
        carried = []
        for k in keys:
            g = st["grads"].get(k)
            pg = live[k].grad
            # "still the library's buffer" is decided by STORAGE, not object identity: _bind_for_training makes a new view of the same span whenever
            # requires_grad toggles (PatchWiseInplace does on every patch), and an old view left in .grad aliases the memory the library overwrites
            if g is not None and pg is not None and pg.data_ptr() == g.data_ptr():
                carried.append((g, g.clone()))
        eng.train_backward(xin, d_inv.detach().to(torch.float32).contiguous(), d_seg.detach().to(torch.float32).contiguous())
        # contiguous runs of this step's trainable tensors in the flat gradient buffer (data-parallel exchange, GradScaler.unscale_)
        runs = []
        for k in keys:
            if st["req"].get(k):
                lo, hi = st["span"][k]
                hi = (hi + 63) // 64 * 64
                if runs and runs[-1][1] == lo:
                    runs[-1][1] = hi
                else:
                    runs.append([lo, hi])
        self._last_grad_runs = (eng, st["flat"], runs)
        if self.grad_exchange is not None:
            # data parallel: average the gradients over the ranks, one collective per run
            self.grad_exchange(st["flat"], runs)
        for g, prev in carried:
            g.add_(prev)
        seen = set()
        for k in keys:
            g = st["grads"].get(k)
            p = live[k]
            if g is None or id(p) in seen:
                continue
            seen.add(id(p))
            if p.grad is None or p.grad.data_ptr() == g.data_ptr():
                p.grad = g                      # (an alias of the same span already holds old + new: see `carried`)
            else:
                p.grad.add_(g)
        self._train_x = None

    def calibrate_precision(self, x: torch.Tensor, budget: float = 5e-4, holdout: int = None, headroom: float = 0.85, per_pixel_p999: float = None) -> dict:
        """Derive the precision map of the default arithmetic (SOCCDPT_PREC_MIXED) on the weights this model holds NOW, from sample frames
        x [B,3,S,S] on the model's device: per launch-site group fp16 or x3 operands such that every hooked feature map, path_1, inverse depth and
        the class logits stay within `budget` (relative L2) of the library's exact-f32 arithmetic on the same weights -- what the reference computes
        in (model/loader.py:126-139; model/base_model.py:5-37 loads whatever checkpoint it is given).  Call it once after load_net / load_state_dict
        of a real checkpoint; the shipped map was derived on the synthetic weights of the tests.  Returns the measured report (soccdpt_calib_report).
        Of the B sample frames the last `holdout` (default B // 3) take no part in the selection and must come in under `budget`; the others are held
        to headroom x budget (default 0.85: the error moves a few per cent from frame to frame).  per_pixel_p999 adds a bound on the 99.9th
        percentile over pixels of the inverse depth's relative error (the budget itself is a relative-L2 statement).  Six frames (4 + 2) are a good sample."""
        assert self.precision == PREC_MIXED, "only the mixed arithmetic has a precision map"
        eng = self._engine(x.device)
        self._sync_weights(eng)
        rep = eng.calibrate_precision(x.detach().to(torch.float32).contiguous(), budget, holdout, headroom, per_pixel_p999)
        self._warned_uncalibrated = True
        return rep

    def precision_map_source(self, device=None) -> str:
        """'shipped' | 'calibrated' | 'edited' | 'uncalibrated-all-x3' | 'n/a' for the engine of `device` (default: the parameters' device)."""
        from ..lib import PREC_SOURCE_NAMES
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        eng = self._engine(dev)
        self._sync_weights(eng)
        return PREC_SOURCE_NAMES.get(eng.prec_map_source(), "n/a")

    def network(self, x: torch.Tensor):
        """Stage-level: encoder + decoder + heads only -> (inv_depth [B,S,S], segmentation [B,C,S,S])."""
        # soccdpt_network reads and writes at the handle's image size whatever the tensor's: checked before the engine exists, so on a CPU tensor too
        img = backbone_image_size(self._engine_backbone())
        assert x.dim() == 4 and x.shape[1] == 3 and x.shape[2] == img and x.shape[3] == img, \
            f"expected x [B,3,{img},{img}], got {tuple(x.shape)}"
        eng = self._engine(x.device)
        self._sync_weights(eng)
        B, S = x.shape[0], x.shape[2]
        inv = torch.empty((B, S, S), device=x.device)
        seg = torch.empty((B, self.num_classes, S, S), device=x.device)
        eng.network(x.detach().to(torch.float32).contiguous(), inv, seg)
        return inv, seg


class _TrainForward(torch.autograd.Function):
    """Autograd node of the train-mode SOccDPT_V3.forward: forward = soccdpt_train_forward + soccdpt_project, backward =
    soccdpt_project_backward + soccdpt_train_backward (parameter gradients land in .grad as a side effect, like any leaf accumulation)."""

    @staticmethod
    def forward(ctx, net, x, anchor):
        ctx.set_materialize_grads(False)
        inv, seg = net.train_forward(x)
        net._train_generation += 1
        eng = net._engine(x.device)
        inv_up, seg_up, points, bits = net._project_outputs(eng, inv, seg)
        ctx.net, ctx.generation, ctx.hw = net, net._train_generation, (inv.shape[1], inv.shape[2])
        ctx.save_for_backward(inv_up)
        if net.compute_occ:
            occ = net._finish_occupancy(eng, inv.shape[0], bits, inv_up=inv_up, seg=seg)
            ctx.mark_non_differentiable(occ)
            return inv_up, seg_up, points, occ
        return inv_up, seg_up, points

    @staticmethod
    def backward(ctx, g_inv, g_seg, g_pts, *g_rest):
        net = ctx.net
        if ctx.generation != net._train_generation:
            raise RuntimeError("SOccDPT_V3: backward through a train-mode forward that is not the most recent one (the library keeps one tape per handle: "
                               "call loss.backward() before the next net(x))")
        (inv_up,) = ctx.saved_tensors
        eng = net._engine(inv_up.device)
        d_inv, d_seg = eng.project_backward(inv_up, g_inv, g_seg, g_pts, ctx.hw[0], ctx.hw[1])
        net.backward(d_inv, d_seg)
        return None, None, None


def _not_in_scope(version):
    class _Unavailable(SOccDPT):
        def __init__(self, *a, **k):
            raise NotImplementedError(
                f"SOccDPT_V{version} is outside the MI355X hot path (SURVEY.md §2: V1 = two full DPTs, V2 raises in the "
                "reference); use version 3")
    _Unavailable.__name__ = f"SOccDPT_V{version}"
    return _Unavailable


SOccDPT_V1 = _not_in_scope(1)
SOccDPT_V2 = _not_in_scope(2)

SOccDPT_versions = {1: SOccDPT_V1, 2: SOccDPT_V2, 3: SOccDPT_V3}


class DepthNet:
    def __init__(self, net: Type[SOccDPT]) -> None:
        self.net = net

    def __call__(self, x: torch.Tensor):
        y_disp_pred, _, _, _ = self.net(x)
        return y_disp_pred

    def eval(self):
        self.net.eval()

    def train(self):
        self.net.train()


class SegNet:
    def __init__(self, net: Type[SOccDPT]) -> None:
        self.net = net

    def __call__(self, x: torch.Tensor):
        _, y_seg_pred, _, _ = self.net(x)
        return y_seg_pred

    def eval(self):
        self.net.eval()

    def train(self):
        self.net.train()
