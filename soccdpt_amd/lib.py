"""ctypes binding of libsoccdpt_hip.so (include/soccdpt_hip.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If the
shared object is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOCCDPT_LIB_PATH") or os.path.join(_HERE, "libsoccdpt_hip.so")   # override: A/B of two builds in one GPU call (tools/ab_bench.sh)

ABI_VERSION = 13
BACKBONE_IDS = {"swin2t16_256": 0, "swin2b24_384": 1, "vitb_rn50_384": 2, "swin2l24_384": 3, "swinl12_384": 5}   # 4 is reserved for vitl16_384
PREC_BF16 = 0
PREC_F32 = 1
PREC_F16 = 2
PREC_F16X3 = 3
PREC_MIXED = 4   # fp16 operands, x3 where the precision map says so (include/soccdpt_hip.h)
PREC_F16X2W = 5  # a precision-map value: fp16 activations, x3 weight pairs (two MFMAs per product)


class SoccdptConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("backbone", ctypes.c_int32),
        ("num_classes", ctypes.c_int32),
        ("features", ctypes.c_int32),
        ("sigmoid", ctypes.c_int32),
        ("compute_occ", ctypes.c_int32),
        ("precision", ctypes.c_int32),
        ("cam_width", ctypes.c_int32),
        ("cam_height", ctypes.c_int32),
        ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
        ("grid", ctypes.c_int32 * 3),
        ("occupancy_shape", ctypes.c_float * 3),
        ("pc_scale", ctypes.c_float * 3),
        ("pc_shift", ctypes.c_float * 3),
        ("rot", ctypes.c_float * 27),
    ]


class KernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("launches", ctypes.c_int32), ("ms", ctypes.c_double),
                ("flops", ctypes.c_double), ("bytes", ctypes.c_double)]


class CalibReport(ctypes.Structure):
    """soccdpt_calib_report (include/soccdpt_hip.h): what soccdpt_prec_calibrate measured."""
    _fields_ = [("n_groups", ctypes.c_int32), ("n_x3", ctypes.c_int32), ("n_x2w", ctypes.c_int32), ("n_x3_shipped", ctypes.c_int32), ("n_x2w_shipped", ctypes.c_int32), ("forwards", ctypes.c_int32),
                ("met_budget", ctypes.c_int32), ("shipped_met_budget", ctypes.c_int32), ("budget", ctypes.c_float),
                ("worst_calibrated", ctypes.c_float), ("worst_shipped", ctypes.c_float), ("worst_all_fp16", ctypes.c_float), ("worst_all_x3", ctypes.c_float),
                ("err_calibrated", ctypes.c_float * 7), ("err_shipped", ctypes.c_float * 7),
                ("cost_us_calibrated", ctypes.c_float), ("cost_us_shipped", ctypes.c_float),
                # ABI 5
                ("calib_frames", ctypes.c_int32), ("holdout_frames", ctypes.c_int32), ("met_headroom", ctypes.c_int32), ("met_holdout", ctypes.c_int32),
                ("headroom", ctypes.c_float), ("worst_holdout", ctypes.c_float), ("worst_holdout_shipped", ctypes.c_float), ("err_holdout", ctypes.c_float * 7),
                ("per_pixel_budget", ctypes.c_float), ("inv_p999_calibrated", ctypes.c_float), ("inv_max_calibrated", ctypes.c_float),
                ("inv_p999_holdout", ctypes.c_float), ("inv_max_holdout", ctypes.c_float), ("inv_p999_all_fp16", ctypes.c_float), ("inv_p999_all_x3", ctypes.c_float)]


class CalibOptions(ctypes.Structure):
    """soccdpt_calib_options (include/soccdpt_hip.h)."""
    _fields_ = [("struct_bytes", ctypes.c_int32), ("holdout", ctypes.c_int32), ("budget", ctypes.c_float), ("headroom", ctypes.c_float), ("per_pixel_p999", ctypes.c_float)]


CALIB_QUANTITIES = ("feat0", "feat1", "feat2", "feat3", "path1", "inv", "seg_logits")
PREC_SOURCE_NAMES = {0: "shipped", 1: "calibrated", 2: "edited", 3: "uncalibrated-all-x3", -1: "n/a"}


class IgemmArgs(ctypes.Structure):
    _fields_ = [
        ("x", ctypes.c_void_p), ("wt", ctypes.c_void_p),
        ("M", ctypes.c_int32), ("N", ctypes.c_int32), ("Cin", ctypes.c_int32), ("taps", ctypes.c_int32),
        ("ldx", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32),
        ("bias", ctypes.c_void_p), ("res1", ctypes.c_void_p), ("res2", ctypes.c_void_p),
        ("act", ctypes.c_int32), ("out_f32", ctypes.c_void_p), ("act_on_f32", ctypes.c_int32),
        ("out_bf16", ctypes.c_void_p), ("out_halo", ctypes.c_int32),
        ("dot_w", ctypes.c_void_p), ("dot_b", ctypes.c_float), ("out_dot", ctypes.c_void_p),
        ("tune", ctypes.c_int32), ("precision", ctypes.c_int32),
        ("splitk", ctypes.c_int32), ("sk_part", ctypes.c_void_p), ("sk_count", ctypes.c_void_p),
        ("sk_part_floats", ctypes.c_size_t), ("sk_count_words", ctypes.c_size_t),
        ("conv_general", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32), ("in_halo", ctypes.c_int32),
        ("Hi", ctypes.c_int32), ("Wi", ctypes.c_int32), ("gather1", ctypes.c_int32),
        ("grp_rows", ctypes.c_int32), ("grp_off", ctypes.c_int32), ("seg2_k", ctypes.c_int32), ("seg2_off", ctypes.c_int32),
        ("grp_stride", ctypes.c_int64),
        ("gn_stats", ctypes.c_void_p), ("gn_part", ctypes.c_void_p), ("gn_count", ctypes.c_void_p),
        ("gn_cpg", ctypes.c_int32), ("gn_hw", ctypes.c_int32), ("gn_part_floats", ctypes.c_size_t), ("gn_count_words", ctypes.c_size_t),
        ("stamps", ctypes.c_void_p), ("sk_defer", ctypes.c_int32),
        # ABI 6: the fused epilogues (sampled residual, LayerNorm, three-class classifier, cross-format operand stores)
        ("res2_h", ctypes.c_int32), ("res2_w", ctypes.c_int32),
        ("ln_g", ctypes.c_void_p), ("ln_b", ctypes.c_void_p), ("ln_xf", ctypes.c_void_p), ("ln_halo", ctypes.c_void_p),
        ("ln_residual", ctypes.c_int32), ("dot3", ctypes.c_int32), ("out_fmt", ctypes.c_int32), ("halo_fmt", ctypes.c_int32),
    ]


class TrainLayerBwdArgs(ctypes.Structure):
    """soccdpt_train_layer_bwd_args (include/soccdpt_hip.h)."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("B", ctypes.c_int32), ("M", ctypes.c_int32), ("r", ctypes.c_int32), ("Hi", ctypes.c_int32), ("Ho", ctypes.c_int32),
        ("N", ctypes.c_int32), ("C", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
        ("stage_weight", ctypes.c_int32), ("defer", ctypes.c_int32), ("reuse_xt", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("dY", ctypes.c_void_p), ("X", ctypes.c_void_p), ("W", ctypes.c_void_p), ("dX_res", ctypes.c_void_p),
        ("dX", ctypes.c_void_p), ("dW", ctypes.c_void_p), ("db", ctypes.c_void_p),
    ]


class TrainAuxArgs(ctypes.Structure):
    """soccdpt_train_aux_args (include/soccdpt_hip.h): what dim / f / in / out mean is listed there per kind."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("flags", ctypes.c_int32), ("dim", ctypes.c_int64 * 6), ("f", ctypes.c_float * 3), ("seed", ctypes.c_uint32),
        ("inp", ctypes.c_void_p * 6), ("out", ctypes.c_void_p * 6),
    ]


class FwdAuxArgs(ctypes.Structure):
    """soccdpt_fwd_aux_args (include/soccdpt_hip.h): what flags / dim / f / in / out mean is listed there per kind."""
    _fields_ = [
        ("kind", ctypes.c_int32), ("flags", ctypes.c_int32), ("dim", ctypes.c_int64 * 6), ("f", ctypes.c_float * 3), ("reserved", ctypes.c_uint32),
        ("inp", ctypes.c_void_p * 6), ("out", ctypes.c_void_p * 6),
    ]


# SOCCDPT_FWD_* (include/soccdpt_hip.h), in the header's order
FWD_KINDS = ("patch_embed", "ln_residual", "merge_gather", "bilinear", "seg_tail", "cvt", "conv_w", "bn_fold", "qkv_bias", "logit_scale", "cpb_table", "ws_conv_w",
             "stem_im2col", "gn_relu_maxpool", "vit_tokens_ln", "ln_rows", "pos_embed_resize")
FWD = {name: i for i, name in enumerate(FWD_KINDS)}
# SOCCDPT_FWD_PATH_*
FWD_PATH_BILINEAR = {1: "generic", 2: "halo8", 3: "halo8_x3"}
FWD_PATH_SEG = {1: "f32", 2: "16bit"}
FWD_PATH_LN_SCALAR, FWD_PATH_LN_V4 = 0x100, 0x200

# SOCCDPT_AUX_* (include/soccdpt_hip.h), in the header's order
AUX_KINDS = ("ln_bwd", "colsum", "colsum2", "bn_fwd", "bn_bwd", "gn_bwd", "ws_bwd", "bilinear_bwd", "maxpool_bwd", "depth_tail", "smallk", "gelu_bwd", "relu_bwd",
             "relu_bwd_halo", "seg_act_bwd", "merge_scatter", "scale_rows", "unscale_check", "drop_path_fill")
AUX = {name: i for i, name in enumerate(AUX_KINDS)}

LAYER_LINEAR, LAYER_CONV3, LAYER_CONV_GEN = 0, 1, 2
# SOCCDPT_ROUTE_* (include/soccdpt_hip.h): which way one layer backward went
ROUTE_BITS = {"fmt_f32": 0x1, "fmt_bf16": 0x2, "fmt_f16": 0x4, "fmt_x3": 0x8, "wgrad_tn": 0x10, "wgrad_x3shift": 0x20, "wgrad_im2colT": 0x40,
              "wgrad_haloshift": 0x80, "wgrad_transpose": 0x100, "wgrad_big_tile": 0x200, "wgrad_sk_defer": 0x400, "dgrad_splitk": 0x800,
              "w_staged": 0x1000, "w_fallback": 0x2000, "sum_deferred": 0x4000, "sum_immediate": 0x8000}
ROUTE_ALL = 0xffff

_lib = None


# Translation units (and the headers they share) that DEFINE OR SEQUENCE the forward path's kernels.  capi.cpp / internal.h (entry points,
# handle bookkeeping), the training step (train*), the criterion, optimiser, metrics, GT-occupancy and input-transform kernels launch
# nothing inside soccdpt_forward, so editing them does not invalidate PMC counters collected for the forward's kernels.
FORWARD_SOURCES = ("Makefile", "attention.hip", "attention_body.h", "attention_qkv.hip", "conv8p.hip", "depth_tail.hip", "elementwise.hip", "gelu.h", "half16.h", "hybrid.hip", "igemm.h",
                   "igemm.hip", "igemm_kernel.h", "kernels.h", "launch.h", "ln_body.h", "mlp_fused.hip", "model.cpp", "projection.hip", "resample.h",
                   "swin1.hip", "vit_attention.hip", "wino.hip")


def csrc_sha() -> str:
    """Short hash of the sources the FORWARD path's kernels are built from (FORWARD_SOURCES).  profiles/*_pmc_traffic.json carry it, so that
    bench.py -- and tests/test_profiles_current.py -- can tell whether the committed PMC counters still describe the current kernels."""
    import hashlib
    h = hashlib.sha1()
    d = os.path.join(_HERE, "csrc")
    for name in FORWARD_SOURCES:
        h.update(name.encode())
        h.update(open(os.path.join(d, name), "rb").read())
    return h.hexdigest()[:16]


def _prototypes() -> dict:
    """symbol -> (restype, argtypes) for every function include/soccdpt_hip.h declares, in the header's order.  tests/test_capi_symbols.py holds
    this table against the header's prototypes (names, parameter counts, pointer / integer / float class and width of every position)."""
    vp, ci, cs, cf, cd, cstr = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_double, ctypes.c_char_p
    P = ctypes.POINTER
    return {
        # ---- lifetime ----
        "soccdpt_create": (ci, [P(SoccdptConfig), P(vp)]),
        "soccdpt_destroy": (None, [vp]),
        "soccdpt_last_error": (cstr, [vp]),
        "soccdpt_abi_version": (ci, []),
        "soccdpt_sizeof": (cs, [ci]),
        # ---- precision map ----
        "soccdpt_prec_map_set": (ci, [vp, cstr, ci]),
        "soccdpt_prec_map_get": (ci, [vp, cstr, ci]),
        # ---- calibration of the precision map ----
        "soccdpt_prec_calibrate_scratch_bytes": (cs, [vp, ci]),
        "soccdpt_prec_calibrate": (ci, [vp, vp, ci, cf, vp, cs, vp, cs, vp, cs, P(CalibReport), vp]),
        "soccdpt_prec_calibrate_ex": (ci, [vp, vp, ci, P(CalibOptions), vp, cs, vp, cs, vp, cs, P(CalibReport), vp]),
        "soccdpt_prec_map_source": (ci, [vp]),
        # ---- weights ----
        "soccdpt_bind_weight": (ci, [vp, cstr, vp, ci, P(ctypes.c_int64), ci]),
        "soccdpt_num_weights": (ci, [vp]),
        "soccdpt_weight_key": (cstr, [vp, ci]),
        "soccdpt_prepared_bytes": (cs, [vp]),
        "soccdpt_workspace_bytes": (cs, [vp, ci]),
        "soccdpt_workspace_invalidate": (ci, [vp]),
        "soccdpt_workspace_zero_fills": (ci, [vp]),
        "soccdpt_prepare": (ci, [vp, vp, cs, vp]),
        # ---- the hot path ----
        "soccdpt_forward": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, vp, cs, vp]),
        "soccdpt_set_streams": (ci, [vp, ci]),
        "soccdpt_set_graph": (ci, [vp, ci]),
        # ---- stage-level entry points ----
        "soccdpt_network": (ci, [vp, vp, ci, vp, vp, vp, cs, vp]),
        "soccdpt_project": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp, ci, vp]),
        "soccdpt_project_backward_scratch_bytes": (cs, [vp, ci, ci]),
        "soccdpt_project_backward": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, cs, vp]),
        "soccdpt_occ_or": (ci, [vp, vp, vp, ci, vp]),
        "soccdpt_occ_expand": (ci, [vp, vp, ci, vp, vp]),
        "soccdpt_occ_zero": (ci, [vp, ci, vp, vp]),
        "soccdpt_occ_set": (ci, [vp, vp, ci, vp, vp]),
        "soccdpt_occ_words": (cs, [vp]),
        # ---- per-frame occupancy grids ----
        "soccdpt_voxelise_frames": (ci, [vp, vp, vp, ci, ci, ci, vp, ci, vp]),
        "soccdpt_occ_expand_frames": (ci, [vp, vp, ci, vp, vp]),
        "soccdpt_forward_frames": (ci, [vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, cs, vp]),
        # ---- occupancy evaluation ----
        "soccdpt_occ_pack": (ci, [vp, ci, ci, cs, cf, ci, vp, vp]),
        "soccdpt_occ_points_scratch_bytes": (cs, [ci, cs, ci]),
        "soccdpt_occ_points_count": (ci, [vp, ci, cs, ci, vp, cs, vp, vp, vp]),
        "soccdpt_occ_points_write": (ci, [vp, ci, P(ctypes.c_int32), ci, P(cf), vp, cs, cs, vp, vp, vp, vp]),
        "soccdpt_occ_iou_counts": (ci, [vp, ci, vp, ci, cs, ci, vp, vp]),
        "soccdpt_last_launch_count": (ci, [vp]),
        "soccdpt_launch_counter": (ctypes.c_ulonglong, []),
        # ---- evaluation metrics ----
        "soccdpt_metrics_scratch_bytes": (cs, [ci, ci]),
        "soccdpt_metrics_depth": (ci, [vp, vp, vp, ci, cs, vp, vp, vp]),
        "soccdpt_metrics_iou": (ci, [vp, vp, ci, ci, cs, vp, vp, vp]),
        # ---- per-kernel device time ----
        "soccdpt_profile_enable": (ci, [vp, ci]),
        "soccdpt_profile_collect": (ci, [vp, P(KernelStat), ci, P(ci)]),
        # ---- training criterion ----
        "soccdpt_loss_scratch_bytes": (cs, [ci, ci, ci, ci, ci]),
        "soccdpt_training_loss": (ci, [ci, ci, ci, ci, ci, ci, ci, cf, cf, cf, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        # ---- ground-truth occupancy generator ----
        "soccdpt_gt_occupancy": (ci, [ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, vp, vp]),
        "soccdpt_op_mlp_ln": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
        # ---- input transform ----
        "soccdpt_input_transform_u8": (ci, [vp, ci, ci, ci, ci, ci, P(cd), P(cd), vp, vp]),
        "soccdpt_adam_step": (ci, [ci, vp, vp, vp, vp, vp, cd, cd, cd, cd, cd, ci, vp]),
        # ---- in-network tile tuning ----
        "soccdpt_profile_sites": (ci, [vp, ci]),
        "soccdpt_site_count": (ci, [vp]),
        "soccdpt_site_get": (ci, [vp, ci, P(ci), P(ci), P(ci), P(ci), P(ci), P(ci)]),
        "soccdpt_tune_set": (ci, [vp, ci, ci, ci, ci, ci]),
        "soccdpt_tune_clear": (ci, [vp]),
        # ---- kernel-level entry points ----
        "soccdpt_op_igemm": (ci, [P(IgemmArgs), vp]),
        "soccdpt_op_depth_tail": (ci, [vp, vp, vp, vp, cf, vp, ci, ci, ci, ci, vp]),
        "soccdpt_op_seg_tail": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, ci, vp]),
        "soccdpt_op_gn_finish": (ci, [vp, vp, ci, ci, ci, ci, ci, cf, vp]),
        "soccdpt_op_gn_apply": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, cs, ci, ci, ci, ci, cf, vp]),
        "soccdpt_op_gn_apply_halo": (ci, [vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, ci, ci, ci, cs, ci, ci, ci, ci, cf, vp]),
        "soccdpt_op_vit_attention": (ci, [vp, vp, ci, ci, ci, ci, vp]),
        "soccdpt_op_vit_attention_out": (ci, [vp, vp, ci, ci, ci, ci, ci, vp]),
        "soccdpt_op_wgrad_tn": (ci, [vp, ctypes.c_long, vp, ctypes.c_long, cs, ci, ci, ci, ci, ci, vp, cs, vp, vp]),
        "soccdpt_op_train_layer_bwd_scratch_bytes": (cs, [P(TrainLayerBwdArgs)]),
        "soccdpt_op_train_layer_bwd": (ci, [vp, P(TrainLayerBwdArgs), vp, cs, P(ctypes.c_uint32), vp]),
        "soccdpt_op_train_aux_scratch_bytes": (cs, [P(TrainAuxArgs)]),
        "soccdpt_op_train_aux": (ci, [P(TrainAuxArgs), vp, cs, vp]),
        "soccdpt_op_fwd_aux": (ci, [P(FwdAuxArgs), P(ctypes.c_uint32), vp]),
        "soccdpt_op_attention_bwd": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
        "soccdpt_op_attention_bwd_slots": (ci, [ci]),
        "soccdpt_op_vit_attention_bwd": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
        "soccdpt_op_attn_param_grads": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]),
        "soccdpt_op_qv_bias_grad": (ci, [vp, vp, vp, ci, vp]),
        "soccdpt_op_window_attention": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
        "soccdpt_op_window_attention_qkv": (ci, [vp, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp]),
        "soccdpt_op_wino_weights": (ci, [vp, vp, vp, ci, ci, ci, vp]),
        "soccdpt_op_wino_conv": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, ci, vp, vp]),
        # ---- training step ----
        "soccdpt_bind_grad": (ci, [vp, cstr, vp]),
        "soccdpt_train_set_amp": (ci, [vp, ci]),
        "soccdpt_train_set_drop_path": (ci, [vp, cf]),
        "soccdpt_train_unscale": (ci, [vp, cs, cf, vp, vp]),
        "soccdpt_train_workspace_bytes": (cs, [vp, ci]),
        "soccdpt_train_forward": (ci, [vp, vp, ci, vp, vp, vp, cs, cf, ctypes.c_uint32, vp]),
        "soccdpt_train_backward": (ci, [vp, vp, ci, vp, vp, vp, cs, vp]),
        "soccdpt_train_backward_encoder": (ci, [vp, ci, P(vp), vp, cs, vp]),
        "soccdpt_train_workspace_tensor": (ci, [vp, ci, cstr, P(cs), P(cs)]),
        "soccdpt_workspace_tensor": (ci, [vp, ci, cstr, P(cs), P(cs), P(ci), P(ci), P(ci), P(ci)]),
    }


PROTOTYPES = _prototypes()


def _vis_prototypes() -> dict:
    """The same table for include/soccdpt_vis.h (the evaluation pictures, csrc/visualise.hip), in that header's order; tests/test_visualise_cpu.py
    holds it against the header.  A second header and a second table: soccdpt_hip.h and its ABI version do not change for these."""
    vp, ci, cs, i32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)
    return {
        "soccdpt_vis_minmax_scratch_bytes": (cs, [ci, cs]),
        "soccdpt_vis_minmax": (ci, [vp, ci, cs, vp, vp, cs, vp]),
        "soccdpt_vis_colorize": (ci, [vp, vp, vp, ci, ci, ci, vp, cs, cs, cs, cs, vp]),
        "soccdpt_vis_color_masks": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, cs, cs, cs, cs, vp]),
        "soccdpt_vis_resize_taps": (ci, [ci, ci, i32]),
        "soccdpt_vis_resize": (ci, [vp, ci, ci, ci, vp, vp, ci, ci, vp, cs, cs, cs, cs, vp]),
        "soccdpt_vis_half_size": (ci, [ci, ci, i32, i32]),
        "soccdpt_vis_shrink_half": (ci, [vp, ci, ci, ci, ci, vp, vp]),
    }


VIS_PROTOTYPES = _vis_prototypes()


def _data_prototypes() -> dict:
    """The same table for include/soccdpt_data.h (the targets of a batch, csrc/batch_targets.hip), in that header's order; tests/test_bdd_dataset_cpu.py
    holds it against the header.  A third header and a third table: soccdpt_hip.h and its ABI version do not change for these."""
    vp, ci = ctypes.c_void_p, ctypes.c_int
    return {
        "soccdpt_data_targets": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
        "soccdpt_data_resize_u8c1": (ci, [vp, ci, ci, ci, vp, vp, ci, ci, vp, vp]),
    }


DATA_PROTOTYPES = _data_prototypes()
DATA_U8, DATA_U16, DATA_F32 = 0, 1, 2   # SOCCDPT_DATA_* (include/soccdpt_data.h)
DATA_MAX_CLASSES = 8


def _pack_prototypes() -> dict:
    """The same table for include/soccdpt_pack.h (targets from palette-indexed labels, csrc/frame_pack.hip), in that header's order;
    tests/test_frame_pack_cpu.py holds it against the header.  A fourth header and a fourth table: soccdpt_hip.h and its ABI version do not change."""
    vp, ci, cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    return {
        "soccdpt_pack_targets": (ci, [vp, ci, cs, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp]),
        "soccdpt_pack_expand": (ci, [vp, ci, cs, vp, ci, ci, ci, ci, vp, vp]),
    }


PACK_PROTOTYPES = _pack_prototypes()


def _swin1_prototypes() -> dict:
    """The same table for include/soccdpt_swin1.h (the Swin-V1 block's kernels on caller-supplied tensors, csrc/swin1.hip), in that header's order;
    tests/test_swin1_large_cpu.py holds it against the header.  A fifth header and a fifth table: soccdpt_hip.h and its ABI version do not change."""
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    return {
        "soccdpt_swin1_window_attention": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp]),
        "soccdpt_swin1_ln_rows": (ci, [vp, vp, vp, vp, ci, ci, ci, cf, vp]),
        "soccdpt_swin1_merge_ln": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp]),
    }


SWIN1_PROTOTYPES = _swin1_prototypes()


def _occ_view_prototypes() -> dict:
    """The same table for include/soccdpt_occ_view.h (pictures of the packed occupancy grid, csrc/occ_view.hip), in that header's order;
    tests/test_occ_view_cpu.py holds it against the header.  A sixth header and a sixth table: soccdpt_hip.h and its ABI version do not change."""
    vp, ci, cs, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    i32, u8, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(cd)
    return {
        "soccdpt_occ_view_columns": (ci, [vp, ci, i32, ci, ci, ci, vp, vp, vp, vp, vp]),
        "soccdpt_occ_view_paint": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, u8, ci, ci, ci, ci, ci, vp, cs, cs, cs, cs, vp]),
        "soccdpt_occ_view_iou2d": (ci, [vp, ci, vp, ci, cs, ci, vp, vp]),
        "soccdpt_occ_view_splat": (ci, [vp, ci, i32, ci, f64, f64, cd, ci, cd, ci, ci, vp, vp]),
        "soccdpt_occ_view_resolve": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, vp, cs, cs, cs, cs, vp]),
    }


OCC_VIEW_PROTOTYPES = _occ_view_prototypes()


def _occ_rays_prototypes() -> dict:
    """The same table for include/soccdpt_occ_rays.h (observed space by ray casting and the 3-D IoU over it, csrc/occ_rays.hip), in that header's
    order; tests/test_occ_rays_cpu.py holds it against the header.  A seventh header and a seventh table: soccdpt_hip.h and its ABI version do not change."""
    vp, ci, cs, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_double
    i32, f64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(cd)
    return {
        "soccdpt_occ_rays_observed": (ci, [vp, ci, ci, ci, i32, f64, f64, cd, cd, ci, ci, vp, vp]),
        "soccdpt_occ_iou_counts_masked": (ci, [vp, ci, vp, ci, cs, ci, vp, ci, ci, vp, vp, vp]),
    }


OCC_RAYS_PROTOTYPES = _occ_rays_prototypes()
PACK_INDEX_BITS = (1, 2, 4, 8)   # k of include/soccdpt_pack.h


def load_library() -> ctypes.CDLL:
    """Load libsoccdpt_hip.so; fail loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C soccdpt_amd/csrc).  The SOccDPT MI355X path has no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for table in (PROTOTYPES, VIS_PROTOTYPES, DATA_PROTOTYPES, PACK_PROTOTYPES, SWIN1_PROTOTYPES, OCC_VIEW_PROTOTYPES, OCC_RAYS_PROTOTYPES):
        for symbol, (restype, argtypes) in table.items():
            fn = getattr(L, symbol)
            fn.restype, fn.argtypes = restype, argtypes
    if L.soccdpt_abi_version() != ABI_VERSION:
        raise RuntimeError("libsoccdpt_hip.so ABI version mismatch; rebuild the library")
    # the ctypes mirrors of the public structs must have the layout the library was compiled with (include/soccdpt_hip.h)
    for which, cls in ((0, SoccdptConfig), (1, IgemmArgs), (2, KernelStat), (3, CalibReport), (4, CalibOptions), (5, TrainLayerBwdArgs), (6, TrainAuxArgs), (7, FwdAuxArgs)):
        if L.soccdpt_sizeof(which) != ctypes.sizeof(cls):
            raise RuntimeError(f"libsoccdpt_hip.so: sizeof mismatch for {cls.__name__}: library {L.soccdpt_sizeof(which)}, binding {ctypes.sizeof(cls)}")
    _lib = L
    return L


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_contiguous(), "device tensors handed to libsoccdpt_hip must be contiguous"
    return t.data_ptr()


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _call(symbol: str, *args, device: torch.device, guard: bool = True):
    """One handle-less entry point (op_*, occupancy evaluation, evaluation pictures, metrics, criterion, Adam, ground-truth occupancy, input transform) on the current
    stream of `device`, which goes last in every such prototype; guard=False leaves the current device alone, as the kernel-level op_* entries do."""
    L = load_library()
    fn = getattr(L, symbol)
    if guard:
        with torch.cuda.device(device):
            rc = fn(*args, _stream_ptr(device))
    else:
        rc = fn(*args, _stream_ptr(device))
    if rc != 0:
        raise RuntimeError(f"{symbol} failed: {L.soccdpt_last_error(None).decode()}")



def host_rotation_matrices(angles: Sequence[float]) -> np.ndarray:
    """Ra, Rb, Rc as 27 f32 values, computed on the host CPU with the same torch ops
    as rotate_points (/root/reference/SOccDPT/model/SOccDPT.py:74-111)."""
    a, b, c = [torch.deg2rad(torch.tensor(float(v), dtype=torch.float32)) for v in angles]
    ra = torch.tensor([[1, 0, 0], [0, torch.cos(a), -torch.sin(a)], [0, torch.sin(a), torch.cos(a)]], dtype=torch.float32)
    rb = torch.tensor([[torch.cos(b), 0, torch.sin(b)], [0, 1, 0], [-torch.sin(b), 0, torch.cos(b)]], dtype=torch.float32)
    rc = torch.tensor([[torch.cos(c), -torch.sin(c), 0], [torch.sin(c), torch.cos(c), 0], [0, 0, 1]], dtype=torch.float32)
    return torch.cat([ra.reshape(-1), rb.reshape(-1), rc.reshape(-1)]).numpy().astype(np.float32)


def make_config(backbone: str, num_classes: int, features: int, sigmoid: bool, compute_occ: bool,
                cam_width: int, cam_height: int, fx: float, fy: float, cx: float, cy: float,
                grid_size, occupancy_shape, pc_scale, pc_shift, correction_angle,
                precision: int = PREC_BF16) -> SoccdptConfig:
    if backbone not in BACKBONE_IDS:
        raise AssertionError(f"Backbone '{backbone}' not implemented on the MI355X path")
    cfg = SoccdptConfig()
    cfg.abi_version = ABI_VERSION
    cfg.backbone = BACKBONE_IDS[backbone]
    cfg.num_classes = int(num_classes)
    cfg.features = int(features)
    cfg.sigmoid = 1 if sigmoid else 0
    cfg.compute_occ = 1 if compute_occ else 0
    cfg.precision = int(precision)
    cfg.cam_width = int(cam_width)
    cfg.cam_height = int(cam_height)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy = [float(np.float32(v)) for v in (fx, fy, cx, cy)]
    for i in range(3):
        cfg.grid[i] = int(grid_size[i])
        cfg.occupancy_shape[i] = float(np.float32(occupancy_shape[i]))
        cfg.pc_scale[i] = float(np.float32(pc_scale[i]))
        cfg.pc_shift[i] = float(np.float32(pc_shift[i]))
    rot = host_rotation_matrices(correction_angle)
    for i in range(27):
        cfg.rot[i] = float(rot[i])
    return cfg


def x3_encode(t: torch.Tensor) -> torch.Tensor:
    """float tensor -> the x3 split-fp16 operand bytes (csrc/half16.h; SOCCDPT_PREC_F16X3) as a flat fp16 tensor of 2 * numel on the same
    device: every aligned group of 8 elements is 8 hi values (RN fp16 of a) + 8 lo values (RN fp16 of (a - hi) * 2048), hi first in even
    groups, lo first in odd ones.  numel (and every row length) must be a multiple of 16."""
    f = t.detach().to(torch.float32).contiguous().reshape(-1, 8)
    assert f.shape[0] % 2 == 0, "x3 tensors are multiples of 16 elements"
    hi = f.clamp(-65504.0, 65504.0).to(torch.float16)
    lo = ((f - hi.float()) * 2048.0).clamp(-65504.0, 65504.0).to(torch.float16)
    odd = (torch.arange(f.shape[0], device=f.device) & 1).bool()[:, None]
    return torch.stack([torch.where(odd, lo, hi), torch.where(odd, hi, lo)], dim=1).reshape(-1)


def x3_decode(raw: torch.Tensor, shape) -> torch.Tensor:
    """Inverse of x3_encode: flat fp16 (or raw bytes) of an x3 tensor -> float64 tensor of `shape` (hi + lo / 2048, exact)."""
    r = raw.view(torch.float16) if raw.dtype != torch.float16 else raw
    r = r.reshape(-1, 2, 8).double()
    odd = (torch.arange(r.shape[0], device=r.device) & 1).bool()[:, None]
    hi = torch.where(odd, r[:, 1], r[:, 0])
    lo = torch.where(odd, r[:, 0], r[:, 1])
    return (hi + lo / 2048.0).reshape(shape)


class Engine:
    """One handle of libsoccdpt_hip.so bound to one GPU (one per rank)."""

    def __init__(self, cfg: SoccdptConfig, device: torch.device):
        if not torch.cuda.is_available():
            raise RuntimeError("soccdpt_amd needs a ROCm GPU (MI355X); there is no CPU fallback")
        self.L = load_library()
        self.cfg = cfg
        self.device = torch.device(device)
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.L.soccdpt_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != 0:
            raise RuntimeError("soccdpt_create failed: " + self.L.soccdpt_last_error(None).decode())
        self._prepared: Optional[torch.Tensor] = None
        self._workspace: Optional[torch.Tensor] = None
        self._train_ws: Optional[torch.Tensor] = None
        self._bound = {}
        self._grads = {}

    def close(self):
        if getattr(self, "_h", None):   # __del__ also runs when __init__ raised before the handle existed
            self.L.soccdpt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _fail(self, symbol: str):
        raise RuntimeError(f"{symbol} failed: {self.L.soccdpt_last_error(self._h).decode()}")

    def _call(self, symbol: str, *args, stream: bool = False):
        """One entry point that takes the handle first.  stream=True: it launches, so it runs under this engine's device with the device's current
        stream as its last argument; the others (setters, queries) take neither."""
        fn = getattr(self.L, symbol)
        if stream:
            with torch.cuda.device(self.device):
                rc = fn(self._h, *args, _stream_ptr(self.device))
        else:
            rc = fn(self._h, *args)
        if rc != 0:
            self._fail(symbol)

    # ---- weights ----
    def weight_keys(self):
        n = self.L.soccdpt_num_weights(self._h)
        return [self.L.soccdpt_weight_key(self._h, i).decode() for i in range(n)]

    def bind(self, key: str, t: torch.Tensor) -> bool:
        """Bind one device tensor under its state-dict key; False if the key is not consumed."""
        assert t.device.type == "cuda" and t.dtype == torch.float32 and t.is_contiguous(), key
        shape = (ctypes.c_int64 * t.dim())(*t.shape)
        rc = self.L.soccdpt_bind_weight(self._h, key.encode(), t.data_ptr(), 0, shape, t.dim())
        if rc == 2:
            return False
        if rc != 0:
            self._fail("soccdpt_bind_weight")
        self._bound[key] = t  # keep alive
        return True

    def _prepared_arena(self) -> int:
        """Grow the arena of prepared weights to what the library asks for now -> that byte count (the arena itself only grows)."""
        nbytes = self.L.soccdpt_prepared_bytes(self._h)
        if self._prepared is None or self._prepared.numel() < nbytes:
            self._prepared = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        return nbytes

    def prepare(self):
        nbytes = self._prepared_arena()
        self._call("soccdpt_prepare", self._prepared.data_ptr(), nbytes, stream=True)

    # ---- precision map (PREC_MIXED handles) ----
    def prec_map(self) -> dict:
        """{group: PREC_F16 | PREC_F16X3} in launch order (uniform-precision handles report their one format for every group)."""
        n = self.L.soccdpt_prec_map_get(self._h, None, 0)
        buf = ctypes.create_string_buffer(n + 1)
        self.L.soccdpt_prec_map_get(self._h, buf, n + 1)
        return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split())}

    def prec_map_set(self, group: str, fmt: int) -> int:
        """Set one group ('s2.b0.attn'), a prefix ('s2.*') or everything ('*') to PREC_F16 / PREC_F16X3; re-prepares the weights."""
        n = self.L.soccdpt_prec_map_set(self._h, group.encode(), int(fmt))
        if n < 0:
            self._fail("soccdpt_prec_map_set")
        if self._bound:
            self.prepare()
        return n

    def prec_map_source(self) -> int:
        """0 shipped map on the weights it was derived from, 1 calibrated on the bound weights, 2 edited, 3 other weights and no calibration yet (the
        library runs every group in x3 until one has run), -1 not a PREC_MIXED handle / not prepared (soccdpt_prec_map_source)."""
        return int(self.L.soccdpt_prec_map_source(self._h))

    def calibrate_precision(self, x: torch.Tensor, budget: float = 5e-4, holdout: int = None, headroom: float = 0.85, per_pixel_p999: float = None) -> dict:
        """soccdpt_prec_calibrate_ex: derive the precision map on the BOUND weights from the sample frames x [B,3,S,S] (against the library's exact-f32
        arithmetic on the same weights); the handle keeps the calibrated map, prepared.  The last `holdout` frames (default: a third of them when
        B >= 3) only verify the map (<= budget); the others select it and are held to headroom x budget.  per_pixel_p999: optional bound on the
        99.9th-percentile per-pixel relative error of the inverse depth.  Returns the report as a dict."""
        assert x.device == self.device and x.dtype == torch.float32 and x.is_contiguous()
        B = x.shape[0]
        if holdout is None:
            holdout = B // 3
        opt = CalibOptions(ctypes.sizeof(CalibOptions), int(holdout), float(budget), float(headroom), float(per_pixel_p999 or 0.0))
        nb = self.L.soccdpt_prec_calibrate_scratch_bytes(self._h, B)
        if nb == 0:
            raise RuntimeError("soccdpt_prec_calibrate: only SOCCDPT_PREC_MIXED handles have a precision map to calibrate")
        scratch = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._prepared_arena()
        ws = self.workspace(B)
        rep = CalibReport()
        self._call("soccdpt_prec_calibrate_ex", x.data_ptr(), B, ctypes.byref(opt), self._prepared.data_ptr(), self._prepared.numel(), ws.data_ptr(), ws.numel(),
                   scratch.data_ptr(), nb, ctypes.byref(rep), stream=True)
        out = {k: getattr(rep, k) for k, _ in CalibReport._fields_ if not k.startswith("err_")}
        out["err_holdout"] = dict(zip(CALIB_QUANTITIES, (float(v) for v in rep.err_holdout))) if rep.holdout_frames else None
        out["err_calibrated"] = dict(zip(CALIB_QUANTITIES, (float(v) for v in rep.err_calibrated)))
        out["err_shipped"] = dict(zip(CALIB_QUANTITIES, (float(v) for v in rep.err_shipped)))
        out["x3_groups"] = sorted(g for g, f in self.prec_map().items() if f == PREC_F16X3)
        out["x2w_groups"] = sorted(g for g, f in self.prec_map().items() if f == PREC_F16X2W)
        return out

    def workspace(self, B: int) -> torch.Tensor:
        """Per-forward scratch.  The library zero-fills it itself whenever (buffer, B, streams) changes (include/soccdpt_hip.h,
        workspace contract), so any allocation will do; the buffer only grows."""
        nbytes = self.L.soccdpt_workspace_bytes(self._h, B)
        if self._workspace is None or self._workspace.numel() < nbytes:
            self._workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
            self.L.soccdpt_workspace_invalidate(self._h)   # a freed buffer's address may be handed out again
        return self._workspace

    def workspace_zero_fills(self) -> int:
        return int(self.L.soccdpt_workspace_zero_fills(self._h))

    def occ_words(self) -> int:
        return int(self.L.soccdpt_occ_words(self._h))

    # ---- stage-level calls ----
    def project(self, inv: torch.Tensor, seg: torch.Tensor, inv_up, seg_up, points, occ_bits, clear_bits: bool = True):
        B, h, w = inv.shape
        self._call("soccdpt_project", _ptr(inv), _ptr(seg), B, h, w, _ptr(inv_up), _ptr(seg_up), _ptr(points), _ptr(occ_bits), 1 if clear_bits else 0, stream=True)

    def project_backward(self, inv_up: torch.Tensor, d_inv_up, d_seg_up, d_points, in_h: int, in_w: int):
        """Gradients of the projection stage's differentiable outputs w.r.t. the network outputs (soccdpt_project_backward):
        -> (d_inv [B,in_h,in_w], d_seg [B,C,in_h,in_w])."""
        B = inv_up.shape[0]
        C = self.cfg.num_classes
        d_inv = torch.empty((B, in_h, in_w), device=self.device)
        d_seg = torch.empty((B, C, in_h, in_w), device=self.device)
        nbytes = self.L.soccdpt_project_backward_scratch_bytes(self._h, B, in_h)
        scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        prep = lambda t: None if t is None else t.detach().to(torch.float32).contiguous()
        a, b, c = prep(d_inv_up), prep(d_seg_up), prep(d_points)
        self._call("soccdpt_project_backward", _ptr(inv_up.contiguous()), _ptr(a), _ptr(b), _ptr(c), B, in_h, in_w, _ptr(d_inv), _ptr(d_seg),
                   scratch.data_ptr(), scratch.numel(), stream=True)
        return d_inv, d_seg

    # ---- in-network tile tuning (tools/autotune_network.py) ----
    def profile_sites(self, on: bool):
        self._call("soccdpt_profile_sites", int(bool(on)))

    def sites(self):
        out = []
        for i in range(self.L.soccdpt_site_count(self._h)):
            v = [ctypes.c_int() for _ in range(6)]
            self._call("soccdpt_site_get", i, *[ctypes.byref(x) for x in v])
            out.append(dict(site=f"site{i:03d}", M=v[0].value, N=v[1].value, K=v[2].value, taps=v[3].value, cfg=v[4].value, launches=v[5].value))
        return out

    def tune_set(self, M: int, N: int, K: int, taps: int, cfg: int):
        self._call("soccdpt_tune_set", M, N, K, taps, cfg)

    def tune_clear(self):
        self._call("soccdpt_tune_clear")

    def occ_or(self, dst_bits: torch.Tensor, src_bits: torch.Tensor, n_sets: int):
        self._call("soccdpt_occ_or", _ptr(dst_bits), _ptr(src_bits), n_sets, stream=True)

    def occ_expand(self, bits: torch.Tensor, B: int, occ: torch.Tensor):
        self._call("soccdpt_occ_expand", _ptr(bits), B, _ptr(occ), stream=True)

    # ---- per-frame occupancy grids (include/soccdpt_hip.h: soccdpt_voxelise_frames / soccdpt_occ_expand_frames / soccdpt_forward_frames) ----
    def voxelise_frames(self, inv_up: torch.Tensor, seg: torch.Tensor, frame_bits: torch.Tensor, clear_bits: bool = True):
        """inv_up [B,Hc,Wc] (the clamped inverse depth `project` wrote) + seg [B,C,h,w] at network resolution -> frame_bits [B, occ_words()] int32:
        row b is the grid of frame b alone (ORed into the buffer; cleared first with clear_bits)."""
        B, h, w = seg.shape[0], seg.shape[2], seg.shape[3]
        assert tuple(inv_up.shape) == (B, self.cfg.cam_height, self.cfg.cam_width) and inv_up.dtype == torch.float32 and seg.dtype == torch.float32
        assert frame_bits.dtype == torch.int32 and frame_bits.numel() == B * self.occ_words()
        self._call("soccdpt_voxelise_frames", _ptr(inv_up), _ptr(seg), B, h, w, _ptr(frame_bits), 1 if clear_bits else 0, stream=True)

    def occ_expand_frames(self, frame_bits: torch.Tensor, B: int, occ: torch.Tensor):
        """frame_bits [B, occ_words()] -> occ [B,g0,g1,g2,C] f32, row b from row b."""
        assert frame_bits.dtype == torch.int32 and frame_bits.numel() == B * self.occ_words() and occ.dtype == torch.float32
        self._call("soccdpt_occ_expand_frames", _ptr(frame_bits), B, _ptr(occ), stream=True)

    def forward_frames(self, x: torch.Tensor, inv_up, seg_up, points, occ, occ_bits, frame_bits):
        """`forward` with per-frame occupancy rows: occ (optional) and frame_bits [B, occ_words()] hold frame b's grid in row b, occ_bits (optional)
        the union as `forward` writes it.  Always eager (no hipGraph replay)."""
        B = x.shape[0]
        ws = self.workspace(B)
        self._call("soccdpt_forward_frames", _ptr(x), B, _ptr(inv_up), _ptr(seg_up), _ptr(points), _ptr(occ), _ptr(occ_bits), _ptr(frame_bits),
                   ws.data_ptr(), ws.numel(), stream=True)

    def occ_zero(self, B: int, occ: torch.Tensor):
        self._call("soccdpt_occ_zero", B, _ptr(occ), stream=True)

    def occ_set(self, bits: torch.Tensor, B: int, occ: torch.Tensor):
        self._call("soccdpt_occ_set", _ptr(bits), B, _ptr(occ), stream=True)

    def network(self, x: torch.Tensor, inv256: torch.Tensor, seg256: torch.Tensor):
        B = x.shape[0]
        ws = self.workspace(B)
        self._call("soccdpt_network", _ptr(x), B, _ptr(inv256), _ptr(seg256), ws.data_ptr(), ws.numel(), stream=True)

    # ---- training step (include/soccdpt_hip.h: soccdpt_train_*) ----
    def bind_grad(self, key: str, g: Optional[torch.Tensor]):
        """Gradient destination of one weight (written by train_backward); None freezes the weight."""
        if g is not None:
            assert g.device.type == "cuda" and g.dtype == torch.float32 and g.is_contiguous(), key
        self._call("soccdpt_bind_grad", key.encode(), _ptr(g))
        self._grads[key] = g  # keep alive

    def train_set_amp(self, mode):
        """0 / False: f32; 1 / True / "bf16": bf16 operands for the gradient GEMMs; 2 / "f16": fp16 operands (use a GradScaler);
        3 / "x3" / "f16x3": split-fp16 operands (three fp16 MFMAs per product): f32-grade gradients, no loss scaling needed."""
        code = {False: 0, True: 1, 0: 0, 1: 1, 2: 2, 3: 3, "bf16": 1, "f16": 2, "fp16": 2, "x3": 3, "f16x3": 3, None: 0}[mode]
        self._call("soccdpt_train_set_amp", code)

    def train_set_drop_path(self, rate: float):
        """Stochastic-depth rate of the Swin-V2 encoder's train-mode forward (timm drop_path_rate; 0 = off)."""
        self._call("soccdpt_train_set_drop_path", float(rate))

    def train_unscale(self, grads: torch.Tensor, inv_scale: float, found_inf: torch.Tensor):
        assert grads.is_contiguous() and grads.dtype == torch.float32 and found_inf.dtype == torch.int32
        _call("soccdpt_train_unscale", grads.data_ptr(), grads.numel(), float(inv_scale), found_inf.data_ptr(), device=self.device)

    def train_workspace(self, B: int) -> torch.Tensor:
        nbytes = self.L.soccdpt_train_workspace_bytes(self._h, B)
        if self._train_ws is None or self._train_ws.numel() < nbytes:
            self._train_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        return self._train_ws

    def train_backward_encoder(self, B: int, d_feats):
        """Encoder backward alone from the gradients of the four hooked feature maps ([B * r^2, C] f32 each, finest first)."""
        ws = self.train_workspace(B)
        keep = [t.detach().to(torch.float32).contiguous() for t in d_feats]
        arr = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in keep])
        self._call("soccdpt_train_backward_encoder", B, arr, ws.data_ptr(), ws.numel(), stream=True)

    def _train_bytes(self, B: int, name: str, elem_bytes: int) -> torch.Tensor:
        """The bytes of one named buffer of the training workspace (soccdpt_train_workspace_tensor gives its offset and element count)."""
        off, n = ctypes.c_size_t(), ctypes.c_size_t()
        if self.L.soccdpt_train_workspace_tensor(self._h, B, name.encode(), ctypes.byref(off), ctypes.byref(n)) != 0:
            raise KeyError(name)
        return self.train_workspace(B)[off.value: off.value + elem_bytes * n.value]

    def train_tensor(self, B: int, name: str, channels: int) -> torch.Tensor:
        """A saved activation / gradient of the training workspace as an f32 [pixels, channels] view (see soccdpt_train_workspace_tensor)."""
        return self._train_bytes(B, name, 4).view(torch.float32).view(-1, channels)

    def train_bytes(self, B: int, name: str, channels: int) -> torch.Tensor:
        """A uint8 buffer of the training workspace ("seg_keep", "hy.pool_idx") as a [pixels, channels] view."""
        return self._train_bytes(B, name, 1).view(-1, channels)

    def train_forward(self, x: torch.Tensor, inv: torch.Tensor, seg: torch.Tensor, dropout_p: float = 0.1, seed: int = 0):
        B = x.shape[0]
        ws = self.train_workspace(B)
        self._call("soccdpt_train_forward", _ptr(x), B, _ptr(inv), _ptr(seg), ws.data_ptr(), ws.numel(), float(dropout_p), int(seed) & 0xFFFFFFFF, stream=True)

    def train_backward(self, x: torch.Tensor, d_inv: torch.Tensor, d_seg: torch.Tensor):
        B = x.shape[0]
        ws = self.train_workspace(B)
        assert d_inv.is_contiguous() and d_seg.is_contiguous() and d_inv.dtype == torch.float32 and d_seg.dtype == torch.float32
        self._call("soccdpt_train_backward", _ptr(x), B, _ptr(d_inv), _ptr(d_seg), ws.data_ptr(), ws.numel(), stream=True)

    def forward(self, x: torch.Tensor, inv_up, seg_up, points, occ, occ_bits):
        B = x.shape[0]
        ws = self.workspace(B)
        self._call("soccdpt_forward", _ptr(x), B, _ptr(inv_up), _ptr(seg_up), _ptr(points), _ptr(occ), _ptr(occ_bits), ws.data_ptr(), ws.numel(), stream=True)

    def set_streams(self, n: int):
        """Deal each batch to n concurrent sub-batches (see soccdpt_set_streams); invalidates the workspace."""
        with torch.cuda.device(self.device):
            self._call("soccdpt_set_streams", int(n))
        self._workspace = None

    def set_graph(self, on: bool = True):
        self._call("soccdpt_set_graph", 1 if on else 0)

    def profile_enable(self, on: bool = True):
        self._call("soccdpt_profile_enable", 1 if on else 0)

    def profile_collect(self):
        """-> {family: dict(launches, ms, flops, bytes)} summed over everything recorded since enable/collect."""
        buf = (KernelStat * 64)()
        n = ctypes.c_int(0)
        self._call("soccdpt_profile_collect", buf, 64, ctypes.byref(n))
        return {buf[i].name.decode(): dict(launches=buf[i].launches, ms=buf[i].ms, flops=buf[i].flops, bytes=buf[i].bytes)
                for i in range(n.value)}

    def launch_count(self) -> int:
        return int(self.L.soccdpt_last_launch_count(self._h))

    def workspace_tensor(self, B: int, name: str):
        """View of a named intermediate of the last soccdpt_network(B) call (diagnostics / parity tests).
        Returns an NHWC float32 tensor [B,H,W,C] (halo stripped, bf16 widened)."""
        off, n = ctypes.c_size_t(), ctypes.c_size_t()
        kind, H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self.L.soccdpt_workspace_tensor(self._h, B, name.encode(), ctypes.byref(off), ctypes.byref(n), ctypes.byref(kind),
                                             ctypes.byref(H), ctypes.byref(W), ctypes.byref(C))
        if rc == 2:
            raise KeyError(f"{name}: not materialised in this mode (the seg head's classifier is part of the convolution's launch; SOCCDPT_SEG_DOT3_OFF=1 restores the map)")
        if rc != 0:
            raise KeyError(name)
        raw = self._workspace[off.value:]
        if "@" in name:  # one concurrent sub-batch of a multi-stream layout: its frame count follows from the element count
            halo = kind.value in (2, 3, 5, 7)
            B = n.value // ((H.value + 2 * halo) * (W.value + 2 * halo) * C.value)
        if kind.value == 0:
            return raw[: n.value * 4].view(torch.float32).reshape(B, H.value, W.value, C.value).clone()
        if kind.value == 3:
            t = raw[: n.value * 4].view(torch.float32).reshape(B, H.value + 2, W.value + 2, C.value)[:, 1:-1, 1:-1]
            return t.clone()
        if kind.value == 7:   # zero-halo NHWC in the x3 split-fp16 format (SOCCDPT_PREC_F16X3)
            t = x3_decode(raw[: n.value * 4], (B, H.value + 2, W.value + 2, C.value))[:, 1:-1, 1:-1]
            return t.float()
        t = raw[: n.value * 2].view(torch.float16 if kind.value in (4, 5) else torch.bfloat16)
        if kind.value in (2, 5):
            t = t.reshape(B, H.value + 2, W.value + 2, C.value)[:, 1:-1, 1:-1]
        else:
            t = t.reshape(B, H.value, W.value, C.value)
        return t.float()


def op_igemm(x, wt, M, N, Cin, taps=1, ldx=0, H=0, W=0, bias=None, res1=None, res2=None, act=0, out_f32=None,
             act_on_f32=0, out_bf16=None, out_halo=0, dot_w=None, dot_b=0.0, out_dot=None, tune=-1, f32=0, precision=None, splitk=1, sk_part=None, sk_count=None,
             conv=None, gather1=0, grp_rows=0, grp_off=0, grp_stride=0, seg2_k=0, seg2_off=0, gn_stats=None, gn_part=None, gn_count=None, gn_cpg=0, gn_hw=0,
             stamps=None, sk_defer=0, res2_h=0, res2_w=0, ln_g=None, ln_b=None, ln_xf=None, ln_halo=None, ln_residual=1, dot3=0, out_fmt=-1,
             halo_fmt=-1):
    """Kernel-level entry (tests): one implicit-GEMM launch on the current stream.  conv = dict(stride, pad, in_halo, Hi, Wi) selects
    the generalised convolution addressing.  res2_h / res2_w: res2 is a low-res map sampled bilinearly; ln_*: the LayerNorm epilogue; dot3: the
    three-class classifier epilogue; out_fmt / halo_fmt: -1 = the launch's format, 1 = fp16 (x3 launch), 3 = x3 (fp16 launch) -- see
    include/soccdpt_hip.h soccdpt_igemm_args."""
    c = conv or {}
    a = IgemmArgs(_ptr(x), _ptr(wt), M, N, Cin, taps, ldx, H, W, _ptr(bias), _ptr(res1), _ptr(res2), act, _ptr(out_f32),
                  act_on_f32, _ptr(out_bf16), out_halo, _ptr(dot_w), float(dot_b), _ptr(out_dot), tune,
                  int(precision) if precision is not None else (PREC_F32 if f32 else PREC_BF16), int(splitk), _ptr(sk_part), _ptr(sk_count),
                  0 if sk_part is None else sk_part.numel(), 0 if sk_count is None else sk_count.numel(),
                  1 if conv else 0, c.get("stride", 1), c.get("pad", 1), c.get("in_halo", 1), c.get("Hi", 0), c.get("Wi", 0), int(gather1),
                  int(grp_rows), int(grp_off), int(seg2_k), int(seg2_off), int(grp_stride),
                  _ptr(gn_stats), _ptr(gn_part), _ptr(gn_count), int(gn_cpg), int(gn_hw),
                  0 if gn_part is None else gn_part.numel(), 0 if gn_count is None else gn_count.numel(), _ptr(stamps), int(sk_defer),
                  int(res2_h), int(res2_w), _ptr(ln_g), _ptr(ln_b), _ptr(ln_xf), _ptr(ln_halo), int(ln_residual), int(dot3), int(out_fmt),
                  int(halo_fmt))
    _call("soccdpt_op_igemm", ctypes.byref(a), device=x.device, guard=False)


def op_depth_tail(d1, wt, bias, w4, b4, out, B, h, w, precision=PREC_BF16):
    """Kernel-level entry (tests): the fused depth tail (soccdpt_op_depth_tail) on the current stream: d1 [B][h][w][128] and wt [32][9*128]
    16-bit (bf16 / fp16 by precision), bias / w4 [32] f32 -> out [B][2h][2w] f32."""
    _call("soccdpt_op_depth_tail", _ptr(d1), _ptr(wt), _ptr(bias), _ptr(w4), float(b4), _ptr(out), int(precision), int(B), int(h), int(w),
          device=d1.device, guard=False)


def op_seg_tail(part, nplanes, bias, tmp, out, B, h, w, sigmoid):
    """Kernel-level entry (tests): finish of a dot3 launch (soccdpt_op_seg_tail) on the current stream: part [nplanes][B*h*w][4] + bias [3] ->
    tmp [B*h*w][3] logits and out [B][3][2h][2w] = sigmoid / ScaledTanh of their x2 bilinear (align_corners) up-sampling."""
    _call("soccdpt_op_seg_tail", _ptr(part), int(nplanes), _ptr(bias), _ptr(tmp), _ptr(out), int(B), int(h), int(w), 1 if sigmoid else 0,
          device=part.device, guard=False)


def op_gn_finish(part, stats, B, tps, groups, hw, cpg, eps=1e-5):
    """Kernel-level entry (tests): per-tile GroupNorm partials -> {mean, rstd} (soccdpt_op_gn_finish) on the current stream."""
    _call("soccdpt_op_gn_finish", _ptr(part), _ptr(stats), int(B), int(tps), int(groups), int(hw), int(cpg), float(eps), device=part.device, guard=False)


def op_gn_apply(raw, stats, gamma, beta, hw, w, cpg, part=None, tps=0, raw2=None, stats2=None, part2=None, tps2=0, gamma2=None, beta2=None, res=None,
                out_f32=None, out_op=None, out_halo=None, out_format=PREC_F32, relu=True, eps=1e-5, halo_format=None):
    """Kernel-level entry (tests): GroupNorm apply (+ shortcut) (+ ReLU) of raw [M][C] (soccdpt_op_gn_apply) on the current stream.  halo_format (a PREC_*
    operand format): out_halo in a format of its own, out_op stays in out_format (soccdpt_op_gn_apply_halo, the SOCCDPT_PREC_MIXED form)."""
    M, C = raw.shape
    head = (_ptr(raw), _ptr(stats), _ptr(part), int(tps), _ptr(gamma), _ptr(beta), _ptr(raw2), _ptr(stats2), _ptr(part2), int(tps2),
            _ptr(gamma2), _ptr(beta2), _ptr(res), _ptr(out_f32), _ptr(out_op), _ptr(out_halo), int(out_format))
    tail = (1 if relu else 0, M, int(hw), int(w), int(C), int(cpg), float(eps))
    if halo_format is None:
        _call("soccdpt_op_gn_apply", *head, *tail, device=raw.device, guard=False)
    else:
        _call("soccdpt_op_gn_apply_halo", *head, int(halo_format), *tail, device=raw.device, guard=False)


def op_vit_attention(qkv, out, B, N, heads, precision=PREC_BF16, out_x3=False):
    """Kernel-level entry (tests): softmax(q k^T / 8) v of one ViT block on the current stream; out_x3 (PREC_F16): `out` as x3 operand pairs."""
    if out_x3:
        _call("soccdpt_op_vit_attention_out", _ptr(qkv), _ptr(out), int(precision), 1, B, N, heads, device=qkv.device, guard=False)
    else:
        _call("soccdpt_op_vit_attention", _ptr(qkv), _ptr(out), int(precision), B, N, heads, device=qkv.device, guard=False)


def op_input_transform_u8(frames: torch.Tensor, Hd: int, Wd: int, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)) -> torch.Tensor:
    """uint8 [B,Hs,Ws,3] device frames -> float32 [B,3,Hd,Wd] network input (soccdpt_input_transform_u8) on the current stream."""
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_cuda
    B, Hs, Ws, _ = frames.shape
    out = torch.empty((B, 3, Hd, Wd), dtype=torch.float32, device=frames.device)
    m, s = (ctypes.c_double * 3)(*mean), (ctypes.c_double * 3)(*std)
    _call("soccdpt_input_transform_u8", _ptr(frames), B, Hs, Ws, Hd, Wd, m, s, _ptr(out), device=frames.device)
    return out


_DATA_DTYPES = {torch.uint8: DATA_U8, torch.uint16: DATA_U16, torch.float32: DATA_F32}


def op_data_targets(seg: torch.Tensor, colors: torch.Tensor, disp: Optional[torch.Tensor] = None, flip: bool = False, want_onehot: bool = True,
                    want_class_map: bool = False, want_y_disp: Optional[bool] = None, want_unmatched: bool = True) -> dict:
    """uint8 [B,H,W,3] label frames + uint8 [C,3] class colours (+ [B,H,W] uint8 / uint16 / float32 disparity), all cuda -> the requested ones of
    onehot f32 [B,C,H,W], class_map i32 [B,H,W], y_disp f32 [B,H,W], unmatched int64 [B] in one launch on the current stream (soccdpt_data_targets)."""
    assert seg.is_cuda and seg.dtype == torch.uint8 and seg.dim() == 4 and seg.shape[3] == 3, "seg must be a cuda uint8 [B,H,W,3] tensor"
    assert colors.is_cuda and colors.dtype == torch.uint8 and colors.dim() == 2 and colors.shape[1] == 3, "colors must be a cuda uint8 [C,3] tensor"
    B, H, W, _ = seg.shape
    C = colors.shape[0]
    dev = seg.device
    dtype = 0
    if disp is not None:
        assert disp.is_cuda and tuple(disp.shape) == (B, H, W), "disp must be a cuda [B,H,W] tensor"
        if disp.dtype not in _DATA_DTYPES:
            raise TypeError(f"op_data_targets: disparity of dtype {disp.dtype} (uint8, uint16 or float32)")
        dtype = _DATA_DTYPES[disp.dtype]
    if want_y_disp is None:
        want_y_disp = disp is not None
    out = dict(
        onehot=torch.empty((B, C, H, W), dtype=torch.float32, device=dev) if want_onehot else None,
        class_map=torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_class_map else None,
        y_disp=torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_y_disp else None,
        unmatched=torch.empty((B,), dtype=torch.int64, device=dev) if want_unmatched else None)     # u64 counts below 2^63
    _call("soccdpt_data_targets", _ptr(seg), _ptr(colors), C, _ptr(disp), dtype, B, H, W, 1 if flip else 0, _ptr(out["onehot"]), _ptr(out["class_map"]),
          _ptr(out["y_disp"]), _ptr(out["unmatched"]), device=dev)
    return out


def op_data_resize_u8c1(src: torch.Tensor, Hd: int, Wd: int, ytaps: Optional[torch.Tensor] = None, xtaps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,Hs,Ws] (cuda) -> [B,Hd,Wd]: the integer bilinear of soccdpt_vis_resize for one channel (soccdpt_data_resize_u8c1) on the current stream;
    ytaps / xtaps: int32 [Hd,3] / [Wd,3] device tables of soccdpt_vis_resize_taps (not needed when the size stays)."""
    assert src.is_cuda and src.dtype == torch.uint8 and src.dim() == 3, "src must be a cuda uint8 [B,H,W] tensor"
    B = src.shape[0]
    out = torch.empty((B, int(Hd), int(Wd)), dtype=torch.uint8, device=src.device)
    _call("soccdpt_data_resize_u8c1", _ptr(src), B, src.shape[1], src.shape[2], _ptr(ytaps), _ptr(xtaps), int(Hd), int(Wd), _ptr(out), device=src.device)
    return out


def _packed_args(idx: torch.Tensor, k: int, palette: torch.Tensor, H: int, W: int):
    assert idx.is_cuda and idx.dim() == 2 and idx.element_size() == 4 and not idx.dtype.is_floating_point, "idx must be a cuda [B,words] tensor of 32-bit words"
    assert palette.is_cuda and palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3, "palette must be a cuda uint8 [P,3] tensor"
    return _ptr(idx), int(k), int(idx.shape[1]), _ptr(palette), int(palette.shape[0])


def op_pack_targets(idx: torch.Tensor, k: int, palette: torch.Tensor, colors: torch.Tensor, H: int, W: int, disp: Optional[torch.Tensor] = None,
                    flip: bool = False, want_onehot: bool = True, want_class_map: bool = False, want_y_disp: Optional[bool] = None,
                    want_unmatched: bool = True) -> dict:
    """op_data_targets for label frames kept as palette indices (soccdpt_pack_targets, include/soccdpt_pack.h): idx [B,words] 32-bit words (cuda), k bits
    per pixel, palette uint8 [P,3] -> the same dictionary, bit for bit what op_data_targets gives for palette[idx]."""
    assert colors.is_cuda and colors.dtype == torch.uint8 and colors.dim() == 2 and colors.shape[1] == 3, "colors must be a cuda uint8 [C,3] tensor"
    B, C, dev = idx.shape[0], colors.shape[0], idx.device
    H, W = int(H), int(W)
    dtype = 0
    if disp is not None:
        assert disp.is_cuda and tuple(disp.shape) == (B, H, W), "disp must be a cuda [B,H,W] tensor"
        if disp.dtype not in _DATA_DTYPES:
            raise TypeError(f"op_pack_targets: disparity of dtype {disp.dtype} (uint8, uint16 or float32)")
        dtype = _DATA_DTYPES[disp.dtype]
    if want_y_disp is None:
        want_y_disp = disp is not None
    out = dict(
        onehot=torch.empty((B, C, H, W), dtype=torch.float32, device=dev) if want_onehot else None,
        class_map=torch.empty((B, H, W), dtype=torch.int32, device=dev) if want_class_map else None,
        y_disp=torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_y_disp else None,
        unmatched=torch.empty((B,), dtype=torch.int64, device=dev) if want_unmatched else None)     # u64 counts below 2^63
    _call("soccdpt_pack_targets", *_packed_args(idx, k, palette, H, W), _ptr(colors), C, _ptr(disp), dtype, B, H, W, 1 if flip else 0, _ptr(out["onehot"]),
          _ptr(out["class_map"]), _ptr(out["y_disp"]), _ptr(out["unmatched"]), device=dev)
    return out


def op_pack_expand(idx: torch.Tensor, k: int, palette: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Palette-indexed label frames (as op_pack_targets takes them) -> uint8 [B,H,W,3] (soccdpt_pack_expand) on the current stream."""
    out = torch.empty((idx.shape[0], int(H), int(W), 3), dtype=torch.uint8, device=idx.device)
    _call("soccdpt_pack_expand", *_packed_args(idx, k, palette, H, W), idx.shape[0], int(H), int(W), _ptr(out), device=idx.device)
    return out


def op_mlp_ln(x_op, x_f32, w1, b1, w2, b2, ln_g, ln_b, x_op_out=None, halo=None, precision=PREC_BF16, H=0, W=0, merge=False):
    """Kernel-level entry (tests): x_f32 += LN(fc2(GELU(fc1(x_op)))) in one launch (soccdpt_op_mlp_ln) on the current stream.  merge: x_op_out [M / 4][4C] in the
    PatchMerging operand layout (include/soccdpt_hip.h)."""
    M, C = x_op.shape
    _call("soccdpt_op_mlp_ln", _ptr(x_op), _ptr(x_f32), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(ln_g), _ptr(ln_b), _ptr(x_op_out), _ptr(halo),
          int(precision), M, C, int(H), int(W), 1 if merge else 0, device=x_op.device, guard=False)


def op_wgrad_tn(a, lda, b, ldb, K, Nout, C, taps=1, rp=0, precision=PREC_BF16, b_row0=0):
    """Kernel-level entry (tests): weight gradient out [Nout][taps * C] from operands as stored (include/soccdpt_hip.h soccdpt_op_wgrad_tn).  a, b: flat device
    tensors (bf16 / fp16, or x3 bytes from x3_encode); b_row0: element offset of row 0 of b inside its tensor (margins in front for taps == 9)."""
    out = torch.empty((Nout, taps * C), dtype=torch.float32, device=a.device)
    scratch = torch.empty((64 * Nout * taps * C,), dtype=torch.float32, device=a.device)
    es = 4 if precision == PREC_F16X3 else 2
    _call("soccdpt_op_wgrad_tn", _ptr(a), lda, b.data_ptr() + b_row0 * es, ldb, K, Nout, C, taps, rp, int(precision), _ptr(scratch), scratch.numel(), _ptr(out),
          device=a.device, guard=False)
    return out


def op_train_layer_bwd_scratch_bytes(args: TrainLayerBwdArgs) -> int:
    """Bytes of scratch soccdpt_op_train_layer_bwd needs for `args`; bad arguments raise."""
    L = load_library()
    n = L.soccdpt_op_train_layer_bwd_scratch_bytes(ctypes.byref(args))
    if n == 0:
        raise RuntimeError(f"soccdpt_op_train_layer_bwd_scratch_bytes failed: {L.soccdpt_last_error(None).decode()}")
    return n


def op_train_layer_bwd(engine: "Engine", args: TrainLayerBwdArgs, scratch: torch.Tensor) -> int:
    """Kernel-level entry (tests): one linear_bwd / conv3_bwd / conv_gen_bwd of the training step on caller-supplied tensors, in the operand format of
    Engine.train_set_amp, on the current stream (include/soccdpt_hip.h soccdpt_op_train_layer_bwd) -> the SOCCDPT_ROUTE_* bits of the route taken."""
    path = ctypes.c_uint32(0)
    engine._call("soccdpt_op_train_layer_bwd", ctypes.byref(args), scratch.data_ptr(), scratch.numel() * scratch.element_size(), ctypes.byref(path), stream=True)
    return int(path.value)


def op_train_aux_scratch_bytes(args: TrainAuxArgs) -> int:
    """Bytes of scratch soccdpt_op_train_aux needs for `args`; bad arguments raise.  Launches nothing."""
    L = load_library()
    n = L.soccdpt_op_train_aux_scratch_bytes(ctypes.byref(args))
    if n == 0:
        raise RuntimeError(f"soccdpt_op_train_aux_scratch_bytes failed: {L.soccdpt_last_error(None).decode()}")
    return n


def op_train_aux(args: TrainAuxArgs, scratch: torch.Tensor) -> None:
    """Kernel-level entry (tests): one non-GEMM launcher of the training step (or the step's composition of a few) on caller-supplied tensors, on the current
    stream of the scratch's device (include/soccdpt_hip.h soccdpt_op_train_aux)."""
    _call("soccdpt_op_train_aux", ctypes.byref(args), scratch.data_ptr(), scratch.numel() * scratch.element_size(), device=scratch.device, guard=False)


def op_fwd_aux(args: FwdAuxArgs, device: torch.device) -> int:
    """Kernel-level entry (tests): one non-GEMM launcher of the forward path on caller-supplied tensors, on the current stream of `device`
    (include/soccdpt_hip.h soccdpt_op_fwd_aux) -> the SOCCDPT_FWD_PATH_* of the kernel the launcher chose."""
    path = ctypes.c_uint32(0)
    _call("soccdpt_op_fwd_aux", ctypes.byref(args), ctypes.byref(path), device=device, guard=False)
    return int(path.value)


def op_attention_bwd_slots(ws: int) -> int:
    """d scale partials per (window, head) that op_attention_bwd writes (0: the window size is not instantiated)."""
    return int(load_library().soccdpt_op_attention_bwd_slots(int(ws)))


def op_attention_bwd(qkv, attn_out, dout, cpb_table, scale, ds, rowstat, dscale_part, dqkv, B, res, ws, shift, heads, precision=PREC_F32):
    """Kernel-level entry (tests): the Swin-V2 window attention backward of the training step on caller-supplied f32 tensors
    (include/soccdpt_hip.h soccdpt_op_attention_bwd); precision = the operand format of the dP, dq / dk and dv products."""
    _call("soccdpt_op_attention_bwd", _ptr(qkv), _ptr(attn_out), _ptr(dout), _ptr(cpb_table), _ptr(scale), _ptr(ds), _ptr(rowstat), _ptr(dscale_part), _ptr(dqkv),
          B, res, ws, shift, heads, int(precision), device=dqkv.device, guard=False)


def op_vit_attention_bwd(qkv, attn_out, dout, rowstat, dqkv, B, N, heads, precision=PREC_F32):
    """Kernel-level entry (tests): the ViT attention backward of the hybrid's training step (soccdpt_op_vit_attention_bwd)."""
    _call("soccdpt_op_vit_attention_bwd", _ptr(qkv), _ptr(attn_out), _ptr(dout), _ptr(rowstat), _ptr(dqkv), B, N, heads, int(precision), device=dqkv.device, guard=False)


def op_attn_param_grads(ds, dscale_part, cpb_table, logit_scale, w0, b0, w2, dtable, dt, hid, dls, dw0, db0, dw2, nwin, ws, pws, heads):
    """Kernel-level entry (tests): dS and the d scale partials -> the gradients of logit_scale and the CPB MLP (soccdpt_op_attn_param_grads); dls / dw0 / db0 /
    dw2 may be None, dtable / dt / hid are the caller's scratch."""
    _call("soccdpt_op_attn_param_grads", _ptr(ds), _ptr(dscale_part), _ptr(cpb_table), _ptr(logit_scale), _ptr(w0), _ptr(b0), _ptr(w2), _ptr(dtable), _ptr(dt),
          _ptr(hid), _ptr(dls), _ptr(dw0), _ptr(db0), _ptr(dw2), nwin, ws, pws, heads, device=logit_scale.device, guard=False)


def op_qv_bias_grad(dqkv_bias, dq, dv, C):
    """Kernel-level entry (tests): q_bias / v_bias gradients from the qkv bias gradient [3C] (soccdpt_op_qv_bias_grad); dq or dv may be None."""
    _call("soccdpt_op_qv_bias_grad", _ptr(dqkv_bias), _ptr(dq), _ptr(dv), C, device=dqkv_bias.device, guard=False)


def op_window_attention(qkv, cpb_table, scale, out, B, res, ws, shift, heads, precision=PREC_BF16):
    nt = (ws * ws + 31) // 32
    scratch = torch.empty((heads * nt * nt * 1024,), dtype=torch.float32, device=qkv.device)
    _call("soccdpt_op_window_attention", _ptr(qkv), _ptr(cpb_table), _ptr(scale), _ptr(out), _ptr(scratch), B, res, ws, shift,
          heads, int(precision), device=qkv.device, guard=False)


def op_window_attention_qkv(x, wqkv, qkv_bias, cpb_table, scale, out, B, res, ws, shift, heads, precision=PREC_F16, out_x3=False, stamps=None):
    """soccdpt_op_window_attention_qkv: one Swin-V2 block's qkv projection + window attention as ONE launch (csrc/attention_qkv.hip)."""
    nt = (ws * ws + 31) // 32
    scratch = torch.empty((heads * nt * nt * 1024,), dtype=torch.float32, device=x.device)
    _call("soccdpt_op_window_attention_qkv", _ptr(x), _ptr(wqkv), _ptr(qkv_bias), _ptr(cpb_table), _ptr(scale), _ptr(out), _ptr(scratch), B, res, ws, shift,
          heads, int(precision), 1 if out_x3 else 0, _ptr(stamps), device=x.device, guard=False)


def op_wino_weights(w, scale=None, precision=PREC_F16):
    """soccdpt_op_wino_weights: [N][C][3][3] f32 -> the Winograd-domain weights U = G g G^T, 16-bit [C/32][16][N][32] (csrc/wino.hip)."""
    N, C = w.shape[0], w.shape[1]
    u = torch.empty((16 * N * C,), dtype=torch.float16 if precision == PREC_F16 else torch.bfloat16, device=w.device)
    _call("soccdpt_op_wino_weights", _ptr(w), _ptr(scale), _ptr(u), N, C, int(precision), device=w.device, guard=False)
    return u


def op_wino_conv(x_halo, u, B, H, W, C, N, bias=None, res1=None, res2=None, res2_hw=(0, 0), relu=False, act_on_f32=False, out_f32=None, out_op=None, out_halo=False,
                 out_x3=False, precision=PREC_F16, stamps=None):
    """soccdpt_op_wino_conv: 3x3 stride-1 convolution over a zero-halo NHWC image in the Winograd F(2x2, 3x3) form, igemm's epilogue options."""
    _call("soccdpt_op_wino_conv", _ptr(x_halo), _ptr(u), B, H, W, C, N, _ptr(bias), _ptr(res1), _ptr(res2), int(res2_hw[0]), int(res2_hw[1]), 1 if relu else 0,
          1 if act_on_f32 else 0, _ptr(out_f32), _ptr(out_op), 1 if out_halo else 0, 1 if out_x3 else 0, int(precision), _ptr(stamps),
          device=x_halo.device, guard=False)


def op_swin1_window_attention(qkv, table, out, B, res, ws, shift, heads, precision=PREC_BF16, out_x3=False):
    """soccdpt_swin1_window_attention (include/soccdpt_swin1.h): Swin-V1 scaled dot-product window attention, table = relative_position_bias_table."""
    nt = (ws * ws + 31) // 32 if ws > 0 else 1
    scratch = torch.empty((max(heads, 1) * nt * nt * 1024,), dtype=torch.float32, device=out.device)
    _call("soccdpt_swin1_window_attention", _ptr(qkv), _ptr(table), _ptr(out), _ptr(scratch), B, res, ws, shift, heads, int(precision), 1 if out_x3 else 0,
          device=out.device, guard=False)


def op_swin1_ln_rows(xf, g, beta, out, rows, C, precision=PREC_BF16, eps=1e-5):
    """soccdpt_swin1_ln_rows: out = LayerNorm(xf) g + beta per row in the operand format `precision`; xf is read only."""
    _call("soccdpt_swin1_ln_rows", _ptr(xf), _ptr(g), _ptr(beta), _ptr(out), int(precision), rows, C, float(eps), device=out.device, guard=False)


def op_swin1_merge_ln(xf, g, beta, out, B, R, C, precision=PREC_BF16, eps=1e-5):
    """soccdpt_swin1_merge_ln: Swin-V1 PatchMerging up to its reduction, [B][R][R][C] f32 -> [B (R/2)^2][4C] in the operand format `precision`."""
    _call("soccdpt_swin1_merge_ln", _ptr(xf), _ptr(g), _ptr(beta), _ptr(out), int(precision), B, R, C, float(eps), device=out.device, guard=False)
