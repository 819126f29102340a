"""Mask-pinned float64 gradient oracle for the training backward (tests/test_train_backward_pinned_gpu.py, tests/test_pinned_backward.py).

A whole-network gradient comparison of two f32 implementations is floored by the ReLU masks they disagree on: a pre-activation within rounding
of zero takes the other side in one of them, which is an O(1) local difference.  Here the masks the HIP train-mode forward actually took (every
ReLU, the seg head's Dropout keep pattern, the stem max-pool's argmax) are read back out of the training workspace and handed to the oracle
(oracle/soccdpt_ref.py, `pinned_masks`).  Both sides then differentiate the same piecewise-linear function, and what separates the HIP
gradient from the float64 one is kernel arithmetic alone.

Metrics (relative to the float64 gradient `ref` of the pinned oracle):
  rel(got)        ||got - ref|| / ||ref|| over the tensor
  block_max(got)  max over blocks of ||d_block|| / (||ref|| * sqrt(|block| / n)) -- blocks of 64 output channels for parameter gradients,
                  64 pixel rows x all channels for activation gradients ([pixels][C], NHWC).  Normalised by the tensor's RMS, so a masked-out
                  (all-zero) block does not divide by zero, and a single wrong tile of a 256-channel gradient shows at full size instead of
                  diluted by sqrt(tiles).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch

from oracle import soccdpt_ref as R

SCR = "depth_net.scratch."
RN = "depth_net.pretrained.model.patch_embed.backbone."
BLOCK = 64

# model type -> (backbone, image size, hooked encoder channels)
MODELS = {
    "dpt_swin2_tiny_256": ("swin2t16_256", 256, (96, 192, 384, 768)),
    "dpt_swin2_base_384": ("swin2b24_384", 384, (128, 256, 512, 1024)),
    "dpt_hybrid_384": ("vitb_rn50_384", 384, (256, 512, 768, 768)),
}


def fres(img: int, l: int) -> int:
    return (img // 4) >> l


def plain(t: torch.Tensor, B: int, r: int, C: int) -> torch.Tensor:
    """[B*r*r][C] (NHWC) -> NCHW."""
    return t.reshape(B, r, r, C).permute(0, 3, 1, 2)


def strip_halo(t: torch.Tensor, B: int, r: int, C: int) -> torch.Tensor:
    """zero-halo [B][r+2][r+2][C] -> NCHW [B][C][r][r] (the border must be zero: it is what the convolutions read as padding)."""
    h = t.reshape(B, r + 2, r + 2, C)
    border = torch.cat([h[:, 0].reshape(-1), h[:, -1].reshape(-1), h[:, :, 0].reshape(-1), h[:, :, -1].reshape(-1)])
    assert bool((border == 0).all()), "halo border is not zero"
    return h[:, 1:-1, 1:-1].permute(0, 3, 1, 2)


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def rn_blocks(arch: R.HybridArch = R.HYBRID) -> List[Tuple[str, int, int, int, int]]:
    """(key prefix, mid, cout, r_in, r_out) of the ResNetV2 bottlenecks in HyTape::blk order."""
    out, r = [], arch.img // 4
    for s, depth in enumerate(arch.layers):
        cout = 256 << s
        for j in range(depth):
            ro = r // 2 if (s > 0 and j == 0) else r
            out.append((f"{RN}stages.{s}.blocks.{j}.", cout // 4, cout, r, ro))
            r = ro
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------------
# reading the HIP masks
# ----------------------------------------------------------------------------------------------------------------------------------------------
def read_forward(eng, model_type: str, B: int, inv: torch.Tensor, dropout_p: float, F: int = 256) -> Tuple[Dict[str, object], Dict[str, torch.Tensor]]:
    """Right after train_forward: (masks by oracle site, forward tensors for a sanity check).  Masks are CPU bool / float64 NCHW."""
    backbone, img, fdims = MODELS[model_type]
    masks: Dict[str, object] = {}
    fwd: Dict[str, torch.Tensor] = {}
    for l in range(4):
        r = fres(img, l)
        rb = f"{SCR}refinenet{l + 1}."
        fwd[f"feat{l}"] = strip_halo(eng.train_tensor(B, f"feat{l}", fdims[l]).cpu(), B, r, fdims[l])
        lrn_raw = plain(eng.train_tensor(B, f"lrn_raw{l}", F).cpu(), B, r, F)
        lrn_relu = strip_halo(eng.train_tensor(B, f"lrn_relu{l}", F).cpu(), B, r, F)
        assert torch.equal(lrn_relu, lrn_raw.clamp_min(0)), f"lrn_relu{l} is not relu(lrn_raw{l})"
        if l < 3:
            fused_raw = plain(eng.train_tensor(B, f"fused_raw{l}", F).cpu(), B, r, F)
            fused_relu = strip_halo(eng.train_tensor(B, f"fused_relu{l}", F).cpu(), B, r, F)
            assert torch.equal(fused_relu, fused_raw.clamp_min(0)), f"fused_relu{l} is not relu(fused_raw{l})"
            masks[rb + "resConfUnit1.relu1"] = lrn_raw > 0
            masks[rb + "resConfUnit1.relu2"] = strip_halo(eng.train_tensor(B, f"rcu1_mid{l}", F).cpu(), B, r, F) > 0
            masks[rb + "resConfUnit2.relu1"] = fused_raw > 0
        else:
            masks[rb + "resConfUnit2.relu1"] = lrn_raw > 0
        masks[rb + "resConfUnit2.relu2"] = strip_halo(eng.train_tensor(B, f"rcu2_mid{l}", F).cpu(), B, r, F) > 0
    r0, r1 = img, img // 2
    masks[SCR + "output_conv.3"] = plain(eng.train_tensor(B, "depth_conv2", 32).cpu(), B, r0, 32) > 0
    masks[SCR + "output_conv.5"] = (inv.detach().cpu() > 0).unsqueeze(1)
    act = plain(eng.train_tensor(B, "seg_act", F).cpu(), B, r1, F)
    keep = plain(eng.train_bytes(B, "seg_keep", F).cpu(), B, r1, F) != 0
    assert bool(((act > 0) <= keep).all()), "a dropped seg-head activation is non-zero"
    masks["seg_head.2"] = ((act > 0).double() / (1.0 - dropout_p), keep)     # ReLU x Dropout; flips counted where the element was kept
    if backbone == "vitb_rn50_384":
        for i, (p, mid, cout, ri, ro) in enumerate(rn_blocks()):
            masks[p + "norm1"] = strip_halo(eng.train_tensor(B, f"hy.blk{i}.t1", mid).cpu(), B, ri, mid) > 0
            masks[p + "norm2"] = plain(eng.train_tensor(B, f"hy.blk{i}.t2", mid).cpu(), B, ro, mid) > 0
            masks[p + "act3"] = plain(eng.train_tensor(B, f"hy.blk{i}.out", cout).cpu(), B, ro, cout) > 0
        fwd["stem_pool"] = plain(eng.train_tensor(B, "hy.stem_pool", 64).cpu(), B, img // 4, 64).clone()
    return masks, fwd


def read_backward(eng, model_type: str, B: int, masks: Dict[str, object], fwd: Dict[str, torch.Tensor], F: int = 256) -> Dict[str, torch.Tensor]:
    """After the backward: d_path1 and d_feat<l> ([pixels][C] copies); for the hybrid the max-pool argmax joins `masks`, with the stem ReLU's
    mask at the selected pixels (the only ones the pool's gradient reaches) taken from the pooled value HIP computed."""
    backbone, img, fdims = MODELS[model_type]
    out = {"d_path1": eng.train_tensor(B, "d_path1", F).cpu().clone()}
    for l in range(4):
        out[f"d_feat{l}"] = eng.train_tensor(B, f"d_feat{l}", fdims[l]).cpu().clone()
    if backbone == "vitb_rn50_384":
        H1, H2 = img // 2, img // 4
        idx = plain(eng.train_bytes(B, "hy.pool_idx", 64).cpu(), B, H2, 64).long()
        assert int(idx.max()) <= 8, "pool_idx out of range"
        oy = torch.arange(H2).view(1, 1, H2, 1)
        ox = torch.arange(H2).view(1, 1, 1, H2)
        iy, ix = 2 * oy + idx // 3, 2 * ox + idx % 3
        assert int(iy.max()) < H1 and int(ix.max()) < H1, "the max-pool picked a padding position"
        flat = (iy * H1 + ix).reshape(B, 64, -1)
        relu = torch.ones(B, 64, H1 * H1, dtype=torch.bool)
        relu.scatter_(2, flat, (fwd["stem_pool"] > 0).reshape(B, 64, -1))
        sel = torch.zeros(B, 64, H1 * H1, dtype=torch.bool)
        sel.scatter_(2, flat, torch.ones_like(flat, dtype=torch.bool))
        masks[RN + "stem.norm"] = (relu.view(B, 64, H1, H1), sel.view(B, 64, H1, H1))
        masks[RN + "stem.pool"] = idx
    return out


def read_drop_path(eng, B: int, backbone: str) -> Dict[Tuple[int, int], Tuple[torch.Tensor, torch.Tensor]]:
    arch = R.ARCHS[backbone]
    dp = {}
    for s, depth in enumerate(arch.depths):
        for j in range(depth):
            t = eng.train_tensor(B, f"drop_path.{s}.{j}", B).cpu().clone()
            dp[(s, j)] = (t[0], t[1])
    return dp


# ----------------------------------------------------------------------------------------------------------------------------------------------
# the pinned oracle
# ----------------------------------------------------------------------------------------------------------------------------------------------
def pinned_oracle(sd, x, a, b, masks, model_type: str, dtype, sigmoid: bool, dropout_p: float = 0.0, drop_path=None):
    """Autograd over the mask-pinned oracle network: loss = <inv, a> + <seg, b>.  Returns (param grads, activation grads keyed like
    read_backward ([pixels][C]), forward tensors, MaskPins)."""
    backbone = MODELS[model_type][0]
    sd_o = {}
    for k, v in sd.items():
        t = v.clone()
        if t.is_floating_point():
            t = t.to(dtype)
            if "running_" not in k:
                t.requires_grad_(True)
        sd_o[k] = t
    with R.pinned_masks(masks) as pins:
        xo = x.to(dtype)
        if backbone == "vitb_rn50_384":
            layers = R.hybrid_encoder(sd_o, xo)
        else:
            dp = None if drop_path is None else {k: (s1.to(dtype), s2.to(dtype)) for k, (s1, s2) in drop_path.items()}
            layers = R.swin_encoder(sd_o, xo, R.ARCHS[backbone], drop_path=dp)
        # d_feat<l> is the decoder's gradient w.r.t. hooked map l (what soccdpt_train_backward leaves in the workspace); the hybrid's stage
        # outputs also feed the next stage, so the decoder runs on detached copies and the encoder is differentiated from their gradients
        dec_in = [t.detach().requires_grad_(True) for t in layers]
        inv, p1 = R.dpt_decoder(sd_o, dec_in)
        p1.retain_grad()
        seg = R.seg_head(sd_o, p1, sigmoid, training=True, dropout_p=dropout_p)
        ((inv * a.to(dtype)).sum() + (seg * b.to(dtype)).sum()).backward()
        torch.autograd.backward(layers, [t.grad for t in dec_in])
    layers = dec_in
    grads = {k: v.grad for k, v in sd_o.items() if isinstance(v, torch.Tensor) and v.requires_grad and v.grad is not None}
    acts = {"d_path1": nhwc(p1.grad)}
    for l, t in enumerate(layers):
        acts[f"d_feat{l}"] = nhwc(t.grad)
    fwd = {f"feat{l}": t.detach() for l, t in enumerate(layers)}
    fwd["inv"], fwd["seg"] = inv.detach(), seg.detach()
    return grads, acts, fwd, pins


# ----------------------------------------------------------------------------------------------------------------------------------------------
# metrics and bounds
# ----------------------------------------------------------------------------------------------------------------------------------------------
def rel(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def block_max(got: torch.Tensor, ref: torch.Tensor) -> float:
    """Worst 64-row block (rows = output channels of a parameter gradient, pixels of a [pixels][C] activation gradient), RMS-normalised."""
    g = got.double().reshape(got.shape[0], -1) if got.dim() > 1 else got.double().reshape(-1, 1)
    r = ref.double().reshape(g.shape)
    n = r.numel()
    tot = float(r.norm())
    if tot == 0.0:
        return 0.0 if float(g.norm()) == 0.0 else math.inf
    worst = 0.0
    for i in range(0, g.shape[0], BLOCK):
        d = g[i:i + BLOCK] - r[i:i + BLOCK]
        worst = max(worst, float(d.norm()) / (tot * math.sqrt(d.numel() / n)))
    return worst


class Bounds:
    """per tensor: err <= max(c * err_f32, floor); median over tensors <= max(1.5 * median_f32, med_floor);
    block-local maximum: blk <= max(c_blk * blk_f32, blk_floor).  `scalar` / `scalar_blk`: plain bounds for the Swin encoder's attention
    vectors (attn.logit_scale, attn.q_bias; see ATTENTION_SCALARS) instead of the above."""

    def __init__(self, c: float, floor: float, med_floor: float, c_blk: float, blk_floor: float, scalar: Optional[float] = None,
                 scalar_blk: Optional[float] = None):
        self.c, self.floor, self.med_floor, self.c_blk, self.blk_floor = c, floor, med_floor, c_blk, blk_floor
        self.scalar, self.scalar_blk = scalar, scalar_blk


# attn.logit_scale (heads elements) and attn.q_bias (C elements) of a Swin block: the gradient of each element is a sum over every token (and,
# for the logit scale, over every attention entry of every window) of random-sign terms that cancel to ~1e-3 of their magnitude, so the
# summation order alone moves it by 1e-4 .. 8e-4 relative (measured; torch's f32 autograd lands 2-14x closer with its own order).  They keep
# the bound test_swin_encoder_backward_exact holds them to (1e-3 against torch f32), with the float64 truth: 1.5e-3 per tensor.
ATTENTION_SCALARS = ("attn.logit_scale", "attn.q_bias")

# The bounds the GPU tests hold the HIP backward to (tests/test_train_backward_pinned_gpu.py states the measurements they come from); the
# fault-injection tests of tests/test_pinned_backward.py check that these constants reject kernel-shaped faults.
SWIN = Bounds(c=3.0, floor=2e-4, med_floor=8e-5, c_blk=3.0, blk_floor=3e-4, scalar=1.5e-3, scalar_blk=3e-3)
HYBRID = Bounds(c=2.0, floor=8e-4, med_floor=5e-4, c_blk=2.0, blk_floor=5e-4)


def compare(got: Dict[str, torch.Tensor], ref64: Dict[str, torch.Tensor], ref32: Dict[str, torch.Tensor], bounds: Bounds,
            label: str = "", verbose: bool = True) -> List[str]:
    """Failures (empty = pass) of every tensor in ref64; `got` and `ref32` must hold the same keys."""
    fails, rows = [], []
    for k, r in ref64.items():
        if k not in got or got[k] is None:
            fails.append(f"{k}: no gradient")
            continue
        g = got[k]
        if tuple(g.shape) != tuple(r.shape):
            g = g.reshape(r.shape)
        if not bool(torch.isfinite(g).all()):
            fails.append(f"{k}: non-finite")
            continue
        if float(r.norm()) == 0.0:
            if float(g.norm()) != 0.0:
                fails.append(f"{k}: reference is zero, got norm {float(g.norm()):.3e}")
            continue
        e, e32 = rel(g, r), rel(ref32[k].reshape(r.shape), r)
        b, b32 = block_max(g, r), block_max(ref32[k].reshape(r.shape), r)
        rows.append((k, e, e32, b, b32))
        if bounds.scalar is not None and k.endswith(ATTENTION_SCALARS):
            if not e <= bounds.scalar:
                fails.append(f"{k}: rel {e:.3e} > {bounds.scalar:g}")
            if not b <= bounds.scalar_blk:
                fails.append(f"{k}: block-local {b:.3e} > {bounds.scalar_blk:g}")
            continue
        if not e <= max(bounds.c * e32, bounds.floor):
            fails.append(f"{k}: rel {e:.3e} > max({bounds.c} x torch f32 {e32:.3e}, {bounds.floor:g})")
        if not b <= max(bounds.c_blk * b32, bounds.blk_floor):
            fails.append(f"{k}: block-local {b:.3e} > max({bounds.c_blk} x torch f32 {b32:.3e}, {bounds.blk_floor:g})")
    if rows:
        med = sorted(r[1] for r in rows)[len(rows) // 2]
        med32 = sorted(r[2] for r in rows)[len(rows) // 2]
        if not med <= max(1.5 * med32, bounds.med_floor):
            fails.append(f"median {med:.3e} > max(1.5 x torch f32 {med32:.3e}, {bounds.med_floor:g})")
        if verbose:
            w = max(rows, key=lambda r: r[1])
            wb = max(rows, key=lambda r: r[3])
            print(f"{label}: {len(rows)} tensors vs the pinned float64 oracle: HIP median {med:.2e} worst {w[1]:.2e} ({w[0]}), block-local max "
                  f"{wb[3]:.2e} ({wb[0]}); torch f32 median {med32:.2e} worst {max(r[2] for r in rows):.2e} block-local max {max(r[4] for r in rows):.2e}")
    return fails
