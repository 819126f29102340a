"""Float64 references of the training step's layer backward routines (csrc/train_step.cpp linear_bwd / conv3_bwd, csrc/train_hybrid_step.cpp
conv_gen_bwd), written from the definitions, plus the helpers tests/test_train_layer_bwd_gpu.py shares: operand rounding, the zero-bordered image
layout, the tap-major weight layout and the slices on which errors are measured.

Every reference takes a dtype: float64 is the reference proper, float32 is torch's own CPU result of the same operation -- the yardstick the f32
operand format is held to (3 x its error, floor 2e-6: the factor tests/pinned_backward.py uses over the same yardstick).

Slices.  A staging mistake is local -- one tap, the border ring of one image, the rows behind the last full 64-row block -- and a whole-tensor
relative L2 averages it away, so every gradient is also measured on
  * dW of a 3x3 convolution: each of the 9 taps;
  * dX of a convolution: per image, the one-pixel border ring and the interior;
  * dX of a linear layer: the rows of the last partial 64-row block (what masked edge tiles and zero-row fills touch) and the rows before it.
A linear layer's dW and db sum over ALL rows, so the last block's contribution to them has no slice of its own: leaving it out moves the whole
tensor by about sqrt(rows in the block / M) (4e-2 for one row of 577), four orders above the bounds the whole tensor is held to.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle.soccdpt_ref import pad_same

FORMATS = ("f32", "x3", "bf16", "f16")
AMP_CODE = {"f32": 0, "bf16": 1, "f16": 2, "x3": 3}                     # soccdpt_train_set_amp
BOUND = {"bf16": 2e-5, "f16": 2e-5, "x3": 2e-6}                          # what test_wgrad_tn_linear / _conv3x3 hold the inner GEMM to; the staging adds no arithmetic
F32_FACTOR, F32_FLOOR = 3.0, 2e-6


def round_to(fmt: str, t: torch.Tensor) -> torch.Tensor:
    """f32 tensor whose values are exactly representable in the 16-bit format of `fmt` (round to nearest even); "f32" / "x3": t itself as f32."""
    t = t.to(torch.float32)
    if fmt == "bf16":
        return t.to(torch.bfloat16).to(torch.float32)
    if fmt == "f16":
        return t.to(torch.float16).to(torch.float32)
    assert fmt in ("f32", "x3"), fmt
    return t


def operand(fmt: str, shape, gen: torch.Generator) -> torch.Tensor:
    """randn operand of one test: pre-rounded for the 16-bit formats (the library's conversion is then exact); fp16 values stay inside the
    format's normal range (2^-10 <= |v| <= 2^10)."""
    t = torch.randn(shape, generator=gen)
    if fmt == "f16":
        t = torch.where(t < 0, -1.0, 1.0) * t.abs().clamp(2.0 ** -10, 2.0 ** 10)
    return round_to(fmt, t)


# ---------------- layouts ----------------
def halo(t: torch.Tensor) -> torch.Tensor:
    """NHWC [B][H][W][C] -> the zero-bordered image [B][H+2][W+2][C]."""
    return F.pad(t, (0, 0, 1, 1, 1, 1)).contiguous()


def nhwc(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t: torch.Tensor) -> torch.Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def to_tap_major(w: torch.Tensor) -> torch.Tensor:
    """[N][C][3][3] -> [N][9][C], tap = 3 ky + kx."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], 9, w.shape[1]).contiguous()


def from_tap_major(wt: torch.Tensor) -> torch.Tensor:
    """[N][9][C] -> [N][C][3][3]."""
    return wt.reshape(wt.shape[0], 3, 3, wt.shape[2]).permute(0, 3, 1, 2).contiguous()


# ---------------- references ----------------
def linear_bwd_ref(dY, X, W, res=None, dtype=torch.float64):
    """y = x W^T + b: dY [M][N], X [M][K], W [N][K] -> dX = dY W (+ res), dW = dY^T X, db = column sums of dY."""
    dY, X, W = dY.to(dtype), X.to(dtype), W.to(dtype)
    dX = dY @ W
    if res is not None:
        dX = dX + res.to(dtype)
    return {"dX": dX, "dW": dY.t() @ X, "db": dY.sum(0)}


def _conv_autograd(fwd, dY, X, W, dtype):
    x = nchw(X).detach().to(dtype).clone().requires_grad_(True)      # fresh leaves: the caller's tensors are left alone
    w = W.detach().to(dtype).clone().requires_grad_(True)
    fwd(x, w).backward(nchw(dY).detach().to(dtype))
    return nhwc(x.grad), w.grad.detach(), dY.detach().to(dtype).sum((0, 1, 2))


def conv3_bwd_ref(dY, X, W, res=None, dtype=torch.float64):
    """nn.Conv2d(C, N, 3, padding=1): dY [B][r][r][N], X [B][r][r][C] (both NHWC), W [N][C][3][3] -> dX NHWC (+ res), dW [N][C][3][3], db [N]."""
    dX, dW, db = _conv_autograd(lambda x, w: F.conv2d(x, w, None, 1, 1), dY, X, W, dtype)
    if res is not None:
        dX = dX + res.to(dtype)
    return {"dX": dX, "dW": dW, "db": db}


def conv_gen_forward(x, w, stride: int, pad: int):
    """The hybrid's 3x3 convolutions as oracle/soccdpt_ref.py runs them: pad 1 = static padding (std_conv_same at stride 1, the reassemble
    convolution act_postprocess4[4] at stride 2), pad 0 = timm's dynamic 'SAME' padding (std_conv_same at stride 2)."""
    if pad == 1:
        return F.conv2d(x, w, None, stride, 1)
    return F.conv2d(pad_same(x, 3, stride), w, None, stride, 0)


def conv_gen_bwd_ref(dY, X, Wtap, stride: int, pad: int, dtype=torch.float64):
    """dY [B][Ho][Ho][N], X [B][Hi][Hi][C] NHWC, Wtap [N][9][C] -> dX NHWC, dW tap-major [N][9][C], db [N]."""
    dX, dW, db = _conv_autograd(lambda x, w: conv_gen_forward(x, w, stride, pad), dY, X, from_tap_major(Wtap), dtype)
    return {"dX": dX, "dW": to_tap_major(dW), "db": db}


# ---------------- slices ----------------
def dw_tap_slices(dW: torch.Tensor, tap_major: bool):
    """('tap k', view) for the 9 taps of a 3x3 weight gradient ([N][C][3][3], or [N][9][C] when tap_major)."""
    for k in range(9):
        yield f"tap{k}", (dW[:, k, :] if tap_major else dW[:, :, k // 3, k % 3])


def dx_image_slices(dX: torch.Tensor):
    """('img b ring' | 'img b interior', 1-D values) of an NHWC gradient: the one-pixel border ring and the interior of every image."""
    B, H, Wd, _ = dX.shape
    ring = torch.ones(H, Wd, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    for b in range(B):
        yield f"img{b}.ring", dX[b][ring]
        if H > 2 and Wd > 2:
            yield f"img{b}.interior", dX[b][~ring]


def linear_row_slices(dX: torch.Tensor):
    """('last partial block' | 'full blocks', rows) of a linear layer's dX: the rows behind the last full 64-row block, and the rest."""
    M = dX.shape[0]
    full = M // 64 * 64
    if full < M:
        yield "rows.last_partial_block", dX[full:]
    if full:
        yield "rows.full_blocks", dX[:full]


def slices(kind: str, name: str, t: torch.Tensor):
    """Every (label, values) a gradient `name` of a `kind` layer is measured on; the whole tensor first."""
    yield "whole", t
    if name == "dW" and kind != "linear":
        yield from dw_tap_slices(t, tap_major=(kind == "conv_gen"))
    elif name == "dX":
        yield from (linear_row_slices(t) if kind == "linear" else dx_image_slices(t))


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    ref = ref.double()
    return float((got.double() - ref).norm() / ref.norm())
