"""Float64 references of the training step's non-GEMM backward kernels (csrc/train.hip tr_*, csrc/train_hybrid.hip th_*), written from the
definitions in the kernels' layouts (NHWC rows; tap-major [Cout][Kpad] for weight standardisation), plus what tests/test_train_aux_gpu.py shares:
the case tables, the input builders, the slices errors are measured on and the description of every soccdpt_op_train_aux call (`spec`).

Per kind there are up to three functions:
  build_<kind>(case)         -> dict of f32 host tensors and parameters (deterministic: seeded by the case)
  ref_<kind>(inp, dtype)     -> dict of outputs from the plain formulas; float64 is the reference, float32 the yardstick where torch has no single op
  torch_<kind>(inp, dtype)   -> the same outputs from torch autograd of the reference project's own operation (F.layer_norm, F.group_norm,
                                F.batch_norm(training=True), timm StdConv2dSame's standardisation, F.interpolate(bilinear, align_corners=True),
                                F.max_pool2d over the 'SAME'-padded input, F.gelu); float64 checks ref_<kind> (tests/test_train_aux_refs.py, 1e-12),
                                float32 is the yardstick of the GPU test: 3 x its error against float64, floor 2e-6.

Margins.  The ReLU / clamp kernels recompute a mask; one flipped element is an O(1) difference that no tolerance describes.  The builders therefore
leave no pre-activation within MARGIN = 1e-3 of zero in float64: GroupNorm and BatchNorm inputs are nudged (and the statistics recomputed) until that
holds, the depth tail keeps only rows whose sum and elements clear it.  The GPU tests exclude no element.  Max-pool: a window whose best and second
best value lie within POOL_GAP = 1e-4 (and that is not all zero) may legitimately resolve either way; the builders keep their share <= 0.1 %.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from oracle.soccdpt_ref import pad_same

MARGIN = 1e-3
POOL_GAP = 1e-4
POOL_VALUE_TOL = 1e-5
POOL_AMBIGUOUS_SHARE = 1e-3
F32_FACTOR, F32_FLOOR = 3.0, 2e-6

# SOCCDPT_AUX_* (include/soccdpt_hip.h)
KINDS = ("ln_bwd", "colsum", "colsum2", "bn_fwd", "bn_bwd", "gn_bwd", "ws_bwd", "bilinear_bwd", "maxpool_bwd", "depth_tail", "smallk", "gelu_bwd", "relu_bwd",
         "relu_bwd_halo", "seg_act_bwd", "merge_scatter", "scale_rows", "unscale_check", "drop_path_fill")
KIND = {k: i for i, k in enumerate(KINDS)}


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(hash_key(key))


def hash_key(key) -> int:
    h = 1469598103934665603
    for ch in repr(key).encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 63)
    return h


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    ref = ref.double()
    n = float(ref.norm())
    d = float((got.double() - ref).norm())
    if n == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / n


# ---------------- case tables ----------------
# LayerNorm backward: name -> (M, C, eps, variant); variants: full | alias (dy = dout, xhat, no parameter gradients) | bare (no xhat, no parameter gradients)
# | shifted (row mean 50, spread 0.5).  C <= 64 leaves lanes idle, C = 100 a partial last lane round, M % 4 != 0 the row >= M exit.
LN_CASES = {
    "1x96": (1, 96, 1e-5, "full"), "5x96": (5, 96, 1e-6, "full"), "259x192": (259, 192, 1e-5, "full"), "64x100": (64, 100, 1e-6, "full"),
    "33x24": (33, 24, 1e-5, "full"), "130x768": (130, 768, 1e-6, "full"), "7x1024": (7, 1024, 1e-5, "full"),
    "130x768_shifted": (130, 768, 1e-5, "shifted"), "259x192_alias": (259, 192, 1e-5, "alias"), "33x24_bare": (33, 24, 1e-6, "bare"),
}
# colsum / colsum2: (M, N).  (16, 63): one full unrolled round; (17, 65): the 4-row tail and a second column block of one column; (4099, 288): 102 chunks of 41
# rows, the last one partial; (2063, 2304): 14 chunks, 36 column blocks
COLSUM_SHAPES = [(1, 64), (15, 1), (16, 63), (17, 65), (1000, 96), (4099, 288), (2063, 2304)]
# BatchNorm (M, C, offset, spread): (2, 5) and (100, 128) have more chunks (128) than rows
BN_CASES = {"2x5": (2, 5, 0.0, 1.0), "100x128": (100, 128, 0.0, 1.0), "128x64": (128, 64, 0.0, 1.0), "129x128": (129, 128, 0.0, 1.0),
            "4099x128": (4099, 128, 0.0, 1.0), "3072x200": (3072, 200, 0.0, 1.0), "129x128_shifted": (129, 128, 30.0, 0.1),
            "8209x130": (8209, 130, 0.0, 1.0)}      # 1 067 170 elements: past the 4096-block cap of the element-wise kernels, the grid-stride loop
# GroupNorm backward (B, HW, C, cpg, relu) and the variant: full | alias (dx = dout) | no_dx | no_param
GN_CASES = {
    "1x9x64": ((1, 9, 64, 2, 1), "full"), "2x49x256": ((2, 49, 256, 8, 1), "full"), "4x36x1024": ((4, 36, 1024, 32, 1), "full"),
    "5x577x512": ((5, 577, 512, 16, 0), "full"), "3x100x96": ((3, 100, 96, 3, 1), "full"), "1x16x32": ((1, 16, 32, 1, 0), "full"),
    "8x16x1024": ((8, 16, 1024, 32, 1), "full"), "40x4x1024": ((40, 4, 1024, 32, 1), "full"),     # 512 / (16 * 40) = 0 chunks, clamped to 1
    "5x577x1024": ((5, 577, 1024, 32, 1), "full"),                                                # 11 540 blocks of gn_bwd_apply: past train_hybrid.hip's 8192-block cap
    "2x49x256_alias": ((2, 49, 256, 8, 1), "alias"), "3x100x96_no_dx": ((3, 100, 96, 3, 1), "no_dx"), "5x577x512_no_param": ((5, 577, 512, 16, 0), "no_param"),
}
# weight standardisation (Cout, Cin, k, Kpad): Kpad = Cin k k as train_hybrid_step.cpp passes it, the stem's 147 padded to 160
WS_CASES = {"stem": (64, 3, 7, 160), "1x1": (8, 64, 1, 64), "3x3_288": (5, 32, 3, 288), "3x3_4608": (3, 512, 3, 4608)}
WS_EPS = 1e-8
# bilinear (B, h, w, H, W, C): C % 4 == 0 takes bilinear_bwd4_kernel
BILINEAR_SHAPES = [(1, 1, 1, 2, 2, 4), (2, 2, 3, 4, 6, 3), (1, 8, 8, 16, 16, 128), (3, 12, 12, 24, 24, 3), (1, 5, 7, 10, 14, 6), (2, 16, 16, 32, 32, 256), (1, 4, 4, 7, 9, 8)]
# max-pool (B, Hi, C, cpg)
MAXPOOL_SHAPES = [(1, 4, 64, 2), (2, 6, 64, 2), (1, 10, 32, 1), (3, 16, 96, 3)]
# depth tail (K, M): K = 32 the float4 kernels (M * 8 / 256 > 4096 blocks at M = 262181: the grid-stride loop), other K the generic ones
DEPTH_TAIL_SHAPES = [(32, 1), (32, 37), (32, 4096), (32, 262181), (8, 37), (8, 1000), (33, 37), (33, 1000)]
SMALLK_SHAPES = [(37, 128, 3), (1000, 100, 4), (5, 64, 1)]


# ---------------- what one call looks like ----------------
@dataclass
class Spec:
    """One soccdpt_op_train_aux call: ins / outs name the tensors of the slots (None = NULL); out shapes / dtypes for the harness."""
    kind: str
    dim: list
    flags: int = 0
    f: tuple = (0.0, 0.0, 0.0)
    seed: int = 0
    ins: list = field(default_factory=list)          # names into the inputs dict, or None
    outs: list = field(default_factory=list)         # (name, shape, torch dtype) or None
    alias: dict = field(default_factory=dict)        # out name -> in name: the output IS that input buffer (pre-filled with the input)
    preset: dict = field(default_factory=dict)       # out name -> inputs-dict name whose values the output buffer holds on entry (accumulate, in/out)


def _o(name, shape, dtype=torch.float32):
    return (name, tuple(shape), dtype)


# ---------------- LayerNorm ----------------
def build_ln(case):
    M, C, eps, variant = LN_CASES[case]
    g = _gen("ln", case)
    y = torch.randn(M, C, generator=g)
    if variant == "shifted":
        y = 50.0 + 0.5 * y
    return {"y": y, "g": 0.5 + torch.rand(C, generator=g), "dout": torch.randn(M, C, generator=g), "eps": eps, "variant": variant}


def spec_ln(case):
    M, C, eps, variant = LN_CASES[case]
    outs = [_o("dy", (M, C)), _o("xhat", (M, C)), _o("dgamma", (C,)), _o("dbeta", (C,))]
    if variant == "alias":
        outs[2] = outs[3] = None
    if variant == "bare":
        outs[1] = outs[2] = outs[3] = None
    return Spec("ln_bwd", [M, C], f=(eps, 0.0, 0.0), ins=["y", "g", "dout"], outs=outs, alias={"dy": "dout"} if variant == "alias" else {})


def ref_ln(inp, dtype=torch.float64):
    y, g, dout = inp["y"].to(dtype), inp["g"].to(dtype), inp["dout"].to(dtype)
    mean = y.mean(1, keepdim=True)
    var = ((y - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + inp["eps"])
    xhat = (y - mean) * rstd
    gd = g * dout
    dy = rstd * (gd - gd.mean(1, keepdim=True) - xhat * (gd * xhat).mean(1, keepdim=True))
    return {"dy": dy, "xhat": xhat, "dgamma": (dout * xhat).sum(0), "dbeta": dout.sum(0)}


def torch_ln(inp, dtype=torch.float64):
    y = inp["y"].to(dtype).clone().requires_grad_(True)
    g = inp["g"].to(dtype).clone().requires_grad_(True)
    b = torch.zeros_like(g, requires_grad=True)
    C = y.shape[1]
    F.layer_norm(y, (C,), g, b, inp["eps"]).backward(inp["dout"].to(dtype))
    return {"dy": y.grad, "xhat": F.layer_norm(y.detach(), (C,), None, None, inp["eps"]), "dgamma": g.grad, "dbeta": b.grad}


# ---------------- column sums ----------------
def build_colsum(shape, with_b, accumulate, two):
    M, N = shape
    g = _gen("colsum", shape, with_b, accumulate, two)
    return {"a": torch.randn(M, N, generator=g), "b": torch.randn(M, N, generator=g) if with_b else None, "out0": torch.randn(N, generator=g) * 3.0,
            "accumulate": accumulate}


def spec_colsum(shape, with_b, accumulate, two):
    M, N = shape
    if two:
        return Spec("colsum2", [M, N], ins=["a", "b" if with_b else None], outs=[_o("out_ab", (N,)), _o("out_a", (N,))])
    return Spec("colsum", [M, N], flags=int(accumulate), ins=["a", "b" if with_b else None], outs=[_o("out", (N,))], preset={"out": "out0"} if accumulate else {})


def ref_colsum(inp, dtype=torch.float64):
    a = inp["a"].to(dtype)
    ab = (a * inp["b"].to(dtype) if inp["b"] is not None else a).sum(0)
    return {"out": ab + inp["out0"].to(dtype) if inp["accumulate"] else ab, "out_ab": ab, "out_a": a.sum(0)}


# ---------------- nudging pre-activations away from zero ----------------
def _clear_margin(x, pre_of, solve, target=5.0 * MARGIN, rounds=50):
    """x (f32) changed in place until no pre-activation pre_of(x) (float64, of the f32 values) lies within 2 * MARGIN of zero: an offending element is
    moved to where its pre-activation is +- target under the current statistics (solve(x64, want) -> x values), then everything is recomputed."""
    for _ in range(rounds):
        pre = pre_of(x.double())
        off = pre.abs() < 2.0 * MARGIN
        if not bool(off.any()):
            return x
        want = torch.where(pre >= 0, target, -target)
        x[off] = solve(x.double(), want)[off].float()
    raise AssertionError("the margin could not be cleared")


# ---------------- BatchNorm (train) + ReLU + Dropout ----------------
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _bn_stats(x64):
    mean = x64.mean(0)
    var = ((x64 - mean) ** 2).mean(0)
    return mean, var


def build_bn(case):
    M, C, offset, spread = BN_CASES[case]
    g = _gen("bn", case)
    x = offset + spread * torch.randn(M, C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    g64, b64 = gamma.double(), beta.double()

    def pre_of(x64):
        mean, var = _bn_stats(x64)
        return (x64 - mean) / torch.sqrt(var + BN_EPS) * g64 + b64

    def solve(x64, want):
        mean, var = _bn_stats(x64)
        return mean + (want - b64) / g64 * torch.sqrt(var + BN_EPS)

    _clear_margin(x, pre_of, solve)
    return {"x": x, "gamma": gamma, "beta": beta, "dout": torch.randn(M, C, generator=g), "rmean0": torch.randn(C, generator=g), "rvar0": 0.5 + torch.rand(C, generator=g),
            "pre64": pre_of(x.double())}


def spec_bn_fwd(case, p=0.0, seed=0):
    M, C = BN_CASES[case][:2]
    return Spec("bn_fwd", [M, C], f=(BN_EPS, BN_MOMENTUM, p), seed=seed, ins=["x", "gamma", "beta"],
                outs=[_o("stats", (C, 2)), _o("rmean", (C,)), _o("rvar", (C,)), _o("y", (M, C)), _o("keep", (M, C), torch.uint8)], preset={"rmean": "rmean0", "rvar": "rvar0"})


def spec_bn_bwd(case, p=0.0):
    M, C = BN_CASES[case][:2]
    return Spec("bn_bwd", [M, C], f=(0.0, 0.0, p), ins=["dout", "y", "keep", "x", "stats", "gamma"], outs=[_o("dbeta", (C,)), _o("dgamma", (C,)), _o("dx", (M, C))])


def ref_bn(inp, dtype=torch.float64, keep=None, p=0.0):
    """Forward and backward; keep (uint8 [M][C]) pins the Dropout mask the kernel returned."""
    x, gamma, beta, dout = (inp[k].to(dtype) for k in ("x", "gamma", "beta", "dout"))
    M = x.shape[0]
    mean, var = _bn_stats(x)
    invstd = 1.0 / torch.sqrt(var + BN_EPS)
    xhat = (x - mean) * invstd
    pre = xhat * gamma + beta
    scale = torch.ones_like(x) if keep is None else keep.to(dtype) / (1.0 - p)
    y = torch.clamp(pre, min=0.0) * scale
    dz = dout * scale * (pre > 0).to(dtype)
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M)
    unbiased = var * M / max(M - 1, 1)
    return {"stats": torch.stack([mean, invstd], 1), "rmean": (1 - BN_MOMENTUM) * inp["rmean0"].to(dtype) + BN_MOMENTUM * mean,
            "rvar": (1 - BN_MOMENTUM) * inp["rvar0"].to(dtype) + BN_MOMENTUM * unbiased, "y": y, "dbeta": dbeta, "dgamma": dgamma, "dx": dx}


def torch_bn(inp, dtype=torch.float64):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    gamma = inp["gamma"].to(dtype).clone().requires_grad_(True)
    beta = inp["beta"].to(dtype).clone().requires_grad_(True)
    rmean, rvar = inp["rmean0"].to(dtype).clone(), inp["rvar0"].to(dtype).clone()
    y = F.relu(F.batch_norm(x, rmean, rvar, gamma, beta, True, BN_MOMENTUM, BN_EPS))
    y.backward(inp["dout"].to(dtype))
    mean, var = _bn_stats(x.detach())
    return {"stats": torch.stack([mean, 1.0 / torch.sqrt(var + BN_EPS)], 1), "rmean": rmean, "rvar": rvar, "y": y.detach(), "dbeta": beta.grad, "dgamma": gamma.grad,
            "dx": x.grad}


# ---------------- GroupNorm backward ----------------
GN_EPS = 1e-5


def _gn_stats(x64, cpg):
    """x [B][HW][C] -> mean, var [B][1][G][1] of the view [B][HW][G][cpg]."""
    B, HW, C = x64.shape
    v = x64.reshape(B, HW, C // cpg, cpg)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    return mean, var


def _gn_pre(x64, gamma64, beta64, cpg):
    B, HW, C = x64.shape
    mean, var = _gn_stats(x64, cpg)
    xhat = ((x64.reshape(B, HW, C // cpg, cpg) - mean) / torch.sqrt(var + GN_EPS)).reshape(B, HW, C)
    return xhat, xhat * gamma64 + beta64


def gn_stats_f32(x, cpg):
    """The statistics the kernels are handed: float64 mean / rstd of the f32 input, rounded to f32, [B][G][2]."""
    mean, var = _gn_stats(x.double(), cpg)
    return torch.stack([mean[:, 0, :, 0], 1.0 / torch.sqrt(var[:, 0, :, 0] + GN_EPS)], -1).float().contiguous()


def _gn_inputs(g, B, HW, C, cpg, relu):
    x = 0.5 + 1.5 * torch.randn(B, HW, C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    g64, b64 = gamma.double(), beta.double()
    if relu:
        def solve(x64, want):
            mean, var = _gn_stats(x64, cpg)
            xh = ((want - b64) / g64).reshape(B, HW, C // cpg, cpg)
            return (mean + xh * torch.sqrt(var + GN_EPS)).reshape(B, HW, C)
        _clear_margin(x, lambda x64: _gn_pre(x64, g64, b64, cpg)[1], solve)
    return x, gamma, beta


def build_gn(case):
    (B, HW, C, cpg, relu), variant = GN_CASES[case]
    g = _gen("gn", (B, HW, C, cpg, relu))          # variants of one shape share its inputs
    x, gamma, beta = _gn_inputs(g, B, HW, C, cpg, relu)
    return {"x": x, "gamma": gamma, "beta": beta, "dout": torch.randn(B, HW, C, generator=g), "stats": gn_stats_f32(x, cpg), "cpg": cpg, "relu": relu,
            "pre64": _gn_pre(x.double(), gamma.double(), beta.double(), cpg)[1], "variant": variant}


def spec_gn(case):
    (B, HW, C, cpg, relu), variant = GN_CASES[case]
    outs = [_o("dx", (B, HW, C)), _o("dgamma", (C,)), _o("dbeta", (C,))]
    if variant == "no_dx":
        outs[0] = None
    if variant == "no_param":
        outs[1] = outs[2] = None
    return Spec("gn_bwd", [B, HW, C, cpg], flags=relu, ins=["dout", "x", "stats", "gamma", "beta"], outs=outs, alias={"dx": "dout"} if variant == "alias" else {})


def ref_gn(inp, dtype=torch.float64):
    x, gamma, beta, dout = (inp[k].to(dtype) for k in ("x", "gamma", "beta", "dout"))
    cpg = inp["cpg"]
    B, HW, C = x.shape
    mean, var = _gn_stats(x, cpg)
    rstd = 1.0 / torch.sqrt(var + GN_EPS)
    xhat = ((x.reshape(B, HW, C // cpg, cpg) - mean) * rstd).reshape(B, HW, C)
    dy = dout * ((xhat * gamma + beta) > 0).to(dtype) if inp["relu"] else dout
    gdy = (gamma * dy).reshape(B, HW, C // cpg, cpg)
    m1 = gdy.mean((1, 3), keepdim=True)
    m2 = (gdy * xhat.reshape(B, HW, C // cpg, cpg)).mean((1, 3), keepdim=True)
    dx = (rstd * (gdy - m1 - xhat.reshape(B, HW, C // cpg, cpg) * m2)).reshape(B, HW, C)
    return {"dx": dx, "dgamma": (dy * xhat).sum((0, 1)), "dbeta": dy.sum((0, 1))}


def torch_gn(inp, dtype=torch.float64):
    x = inp["x"].to(dtype).permute(0, 2, 1).contiguous().requires_grad_(True)       # [B][C][HW]
    gamma = inp["gamma"].to(dtype).clone().requires_grad_(True)
    beta = inp["beta"].to(dtype).clone().requires_grad_(True)
    y = F.group_norm(x, x.shape[1] // inp["cpg"], gamma, beta, GN_EPS)
    if inp["relu"]:
        y = F.relu(y)
    y.backward(inp["dout"].to(dtype).permute(0, 2, 1))
    return {"dx": x.grad.permute(0, 2, 1).contiguous(), "dgamma": gamma.grad, "dbeta": beta.grad}


# ---------------- weight standardisation backward ----------------
def ws_to_tap_major(w, Kpad, fill=float("nan")):
    """[Cout][Cin][k][k] -> [Cout][Kpad], index tap * Cin + ci; the columns behind the fan-in hold `fill` (the kernels must not read them)."""
    Cout, Cin, k, _ = w.shape
    out = torch.full((Cout, Kpad), fill, dtype=w.dtype)
    out[:, : Cin * k * k] = w.permute(0, 2, 3, 1).reshape(Cout, -1)
    return out


def _ws_hat(w, dtype):
    w = w.to(dtype)
    flat = w.reshape(w.shape[0], -1)
    mean = flat.mean(1, keepdim=True)
    var = ((flat - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + WS_EPS)
    return ((flat - mean) * rstd), rstd


def build_ws(case):
    Cout, Cin, k, Kpad = WS_CASES[case]
    g = _gen("ws", case)
    w = 0.05 * torch.randn(Cout, Cin, k, k, generator=g) + 0.01
    dwh_param = torch.randn(Cout, Cin, k, k, generator=g)
    wh = _ws_hat(w, torch.float64)[0].reshape(w.shape).float()                    # what the forward saved: the float64 value rounded to f32
    return {"w": w, "dwh_param": dwh_param, "dwh": ws_to_tap_major(dwh_param, Kpad), "wh": ws_to_tap_major(wh, Kpad)}


def spec_ws(case):
    Cout, Cin, k, Kpad = WS_CASES[case]
    return Spec("ws_bwd", [Cout, Cin, k, Kpad], f=(WS_EPS, 0.0, 0.0), ins=["dwh", "wh", "w"], outs=[_o("dw", (Cout, Cin, k, k))])


def ref_ws(inp, dtype=torch.float64):
    w = inp["w"]
    what, rstd = _ws_hat(w, dtype)
    dh = inp["dwh_param"].to(dtype).reshape(w.shape[0], -1)
    dw = rstd * (dh - dh.mean(1, keepdim=True) - what * (dh * what).mean(1, keepdim=True))
    return {"dw": dw.reshape(w.shape)}


def torch_ws(inp, dtype=torch.float64):
    w = inp["w"].to(dtype).clone().requires_grad_(True)
    wh = F.batch_norm(w.reshape(1, w.shape[0], -1), None, None, training=True, momentum=0.0, eps=WS_EPS).reshape_as(w)    # timm StdConv2dSame.forward
    wh.backward(inp["dwh_param"].to(dtype))
    return {"dw": w.grad}


# ---------------- bilinear align_corners=True backward ----------------
def build_bilinear(shape, accumulate):
    B, h, w, H, W, C = shape
    g = _gen("bilinear", shape)
    return {"dhi": torch.randn(B, H, W, C, generator=g), "dlo0": torch.randn(B, h, w, C, generator=g), "accumulate": accumulate, "shape": shape}


def spec_bilinear(shape, accumulate):
    B, h, w, H, W, C = shape
    return Spec("bilinear_bwd", list(shape), flags=int(accumulate), ins=["dhi"], outs=[_o("dlo", (B, h, w, C))], preset={"dlo": "dlo0"} if accumulate else {})


def _interp_matrix(n_lo, n_hi, dtype):
    """[n_hi][n_lo]: row Y holds the two weights with which high-res position Y samples the low-res axis (align_corners=True)."""
    A = torch.zeros(n_hi, n_lo, dtype=dtype)
    for Y in range(n_hi):
        src = Y * (n_lo - 1) / (n_hi - 1) if n_hi > 1 else 0.0
        y0 = min(int(math.floor(src)), n_lo - 1)
        y1 = min(y0 + 1, n_lo - 1)
        l = src - y0
        A[Y, y0] += 1.0 - l
        A[Y, y1] += l
    return A


def ref_bilinear(inp, dtype=torch.float64):
    B, h, w, H, W, C = inp["shape"]
    dlo = torch.einsum("Yy,Xx,bYXc->byxc", _interp_matrix(h, H, dtype), _interp_matrix(w, W, dtype), inp["dhi"].to(dtype))
    return {"dlo": dlo + inp["dlo0"].to(dtype) if inp["accumulate"] else dlo}


def torch_bilinear(inp, dtype=torch.float64):
    B, h, w, H, W, C = inp["shape"]
    lo = torch.zeros(B, C, h, w, dtype=dtype, requires_grad=True)
    F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True).backward(inp["dhi"].to(dtype).permute(0, 3, 1, 2))
    dlo = lo.grad.permute(0, 2, 3, 1).contiguous()
    return {"dlo": dlo + inp["dlo0"].to(dtype) if inp["accumulate"] else dlo}


# ---------------- stem max-pool backward ----------------
def _pool_windows(A):
    """A [B][Hi][Hi][C] -> window values [B][Ho][Ho][C][9] (tap = 3 ky + kx), -inf where TF 'SAME' pads (behind the image: Hi even)."""
    B, Hi, _, C = A.shape
    assert Hi % 2 == 0
    P = F.pad(A.permute(0, 3, 1, 2), (0, 1, 0, 1), value=float("-inf"))
    win = P.unfold(2, 3, 2).unfold(3, 3, 2)                       # [B][C][Ho][Ho][3][3]
    return win.reshape(B, C, Hi // 2, Hi // 2, 9).permute(0, 2, 3, 1, 4).contiguous()


def pool_activation(inp, dtype=torch.float64):
    x, gamma, beta = (inp[k].to(dtype) for k in ("raw", "gamma", "beta"))
    B, Hi, _, C = x.shape
    _, pre = _gn_pre(x.reshape(B, Hi * Hi, C), gamma, beta, inp["cpg"])
    return torch.clamp(pre, min=0.0).reshape(B, Hi, Hi, C)


def pool_scatter(dpool, idx, Hi, dtype=torch.float64):
    """dA [B][Hi][Hi][C] = dpool scattered to window position idx (uint8, 3 ky + kx) of every window."""
    B, Ho, _, C = dpool.shape
    dA = torch.zeros(B, Hi + 1, Hi + 1, C, dtype=dtype)
    idx = idx.long()
    oy = torch.arange(Ho).view(1, Ho, 1, 1)
    ox = torch.arange(Ho).view(1, 1, Ho, 1)
    iy = (2 * oy + idx // 3).reshape(-1)
    ix = (2 * ox + idx % 3).reshape(-1)
    b = torch.arange(B).view(B, 1, 1, 1).expand_as(idx).reshape(-1)
    c = torch.arange(C).view(1, 1, 1, C).expand_as(idx).reshape(-1)
    dA.index_put_((b, iy, ix, c), dpool.to(dtype).reshape(-1), accumulate=True)
    return dA[:, :Hi, :Hi].contiguous()


def pool_classes(win64):
    """-> (argmax [..] first in scan order, decided [..] bool: gap above POOL_GAP or the window all zero, wmax [..])."""
    top2 = win64.topk(2, dim=-1).values
    wmax = top2[..., 0]
    all_zero = (torch.where(torch.isinf(win64), torch.zeros_like(win64), win64) == 0).all(-1)
    decided = ((top2[..., 0] - top2[..., 1]) > POOL_GAP) | all_zero
    first = (win64 == wmax.unsqueeze(-1)).to(torch.uint8).argmax(-1)          # first maximum in scan order
    return first, decided, wmax


def build_maxpool(shape):
    B, Hi, C, cpg = shape
    for attempt in range(64):
        g = _gen("maxpool", shape, attempt)
        raw, gamma, beta = _gn_inputs(g, B, Hi * Hi, C, cpg, relu=False)
        inp = {"raw": raw.reshape(B, Hi, Hi, C), "gamma": gamma, "beta": beta, "stats": gn_stats_f32(raw, cpg), "cpg": cpg,
               "dpool": torch.randn(B, Hi // 2, Hi // 2, C, generator=g)}
        _, decided, _ = pool_classes(_pool_windows(pool_activation(inp)))
        if float((~decided).float().mean()) <= 0.5 * POOL_AMBIGUOUS_SHARE:
            return inp
    raise AssertionError("no input with few enough ambiguous windows")


def spec_maxpool(shape):
    B, Hi, C, cpg = shape
    return Spec("maxpool_bwd", list(shape), ins=["dpool", "raw", "stats", "gamma", "beta"], outs=[_o("idx", (B, Hi // 2, Hi // 2, C), torch.uint8), _o("dA", (B, Hi, Hi, C))])


def ref_maxpool(inp, dtype=torch.float64):
    A = pool_activation(inp, dtype)
    idx, _, _ = pool_classes(_pool_windows(A))
    return {"idx": idx.to(torch.uint8), "dA": pool_scatter(inp["dpool"], idx, A.shape[1], dtype)}


def torch_maxpool(inp, dtype=torch.float64):
    A = pool_activation(inp, dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    F.max_pool2d(pad_same(A, 3, 2, value=float("-inf")), 3, 2).backward(inp["dpool"].to(dtype).permute(0, 3, 1, 2))
    return {"dA": A.grad.permute(0, 2, 3, 1).contiguous()}


# ---------------- depth tail ----------------
def build_depth_tail(shape):
    K, M = shape
    g = _gen("depth_tail", shape)
    w4 = torch.randn(K, generator=g) / math.sqrt(K)
    b4 = torch.tensor([0.05])
    rows, have = [], 0
    while have < M:
        e = torch.randn(M + M // 4 + 64, K, generator=g)
        s = torch.clamp(e.double(), min=0.0) @ w4.double() + b4.double()
        ok = (s.abs() > 2.0 * MARGIN) & (e.abs() > 2.0 * MARGIN).all(1)
        rows.append(e[ok])
        have += int(ok.sum())
    e = torch.cat(rows)[:M].contiguous()
    return {"e": e, "w4": w4, "b4": b4, "dinv": torch.randn(M, generator=g), "s64": torch.clamp(e.double(), min=0.0) @ w4.double() + b4.double()}


def spec_depth_tail(shape):
    K, M = shape
    return Spec("depth_tail", [M, K], ins=["e", "w4", "b4", "dinv"], outs=[_o("inv", (M,)), _o("de", (M, K)), _o("rowterm", (M, K + 1))])


def ref_depth_tail(inp, dtype=torch.float64):
    e, w4, b4, dinv = (inp[k].to(dtype) for k in ("e", "w4", "b4", "dinv"))
    s = torch.clamp(e, min=0.0) @ w4 + b4
    dz = dinv * (s > 0).to(dtype)
    return {"inv": torch.clamp(s, min=0.0), "de": dz[:, None] * w4 * (e > 0).to(dtype), "rowterm": torch.cat([dz[:, None] * torch.clamp(e, min=0.0), dz[:, None]], 1)}


def torch_depth_tail(inp, dtype=torch.float64):
    e = inp["e"].to(dtype).clone().requires_grad_(True)
    w4 = inp["w4"].to(dtype).clone().requires_grad_(True)
    b4 = inp["b4"].to(dtype).clone().requires_grad_(True)
    inv = F.relu(F.relu(e) @ w4 + b4)
    inv.backward(inp["dinv"].to(dtype))
    return {"inv": inv.detach(), "de": e.grad, "dw4": w4.grad, "db4": b4.grad}


# ---------------- small-K 1x1 convolution ----------------
def build_smallk(shape):
    M, C, K = shape
    g = _gen("smallk", shape)
    return {"dl": torch.randn(M, K, generator=g), "w": torch.randn(K, C, generator=g), "x": torch.randn(M, C, generator=g)}


def spec_smallk(shape):
    M, C, K = shape
    return Spec("smallk", [M, C, K], ins=["dl", "w", "x"], outs=[_o("dx", (M, C)), _o("dw", (K, C))])


def ref_smallk(inp, dtype=torch.float64):
    dl, w, x = (inp[k].to(dtype) for k in ("dl", "w", "x"))
    return {"dx": dl @ w, "dw": dl.t() @ x}


def torch_smallk(inp, dtype=torch.float64):
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    w = inp["w"].to(dtype).clone().requires_grad_(True)
    F.linear(x, w).backward(inp["dl"].to(dtype))
    return {"dx": x.grad, "dw": w.grad}


# ---------------- element-wise and permutation kernels ----------------
GELU_LINSPACE, GELU_RANDOM = 4097, 1100001
RELU_N = 1100003       # past the 4096-block cap: the grid-stride loop


def build_gelu():
    g = _gen("gelu")
    pre = torch.cat([torch.linspace(-12.0, 12.0, GELU_LINSPACE), 3.0 * torch.randn(GELU_RANDOM, generator=g)])      # past the 4096-block cap
    return {"pre": pre, "dy": torch.randn(pre.numel(), generator=g)}


def ref_gelu(inp, dtype=torch.float64):
    x, dy = inp["pre"].to(dtype), inp["dy"].to(dtype)
    cdf = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return {"dx": dy * (cdf + x * pdf)}


def torch_gelu(inp, dtype=torch.float64):
    x = inp["pre"].to(dtype).clone().requires_grad_(True)
    F.gelu(x).backward(inp["dy"].to(dtype))
    return {"dx": x.grad}


def build_relu(with_add, halo=None):
    g = _gen("relu", with_add, halo)
    shape = halo if halo else (RELU_N,)
    ref = torch.randn(shape, generator=g)
    ref[ref.abs() < 0.05] = 0.0                                    # exact zeros: the mask is ref > 0
    return {"dy": torch.randn(shape, generator=g), "ref": ref, "add": torch.randn(shape, generator=g) if with_add else None,
            "ref_halo": F.pad(ref, (0, 0, 1, 1, 1, 1), value=1.0).contiguous() if halo else None}      # a border of ones: reading it instead of the pixel shows


def ref_relu(inp, dtype=torch.float64):
    dx = inp["dy"].to(dtype) * (inp["ref"] > 0).to(dtype)
    return {"dx": dx + inp["add"].to(dtype) if inp["add"] is not None else dx}


def torch_relu(inp, dtype=torch.float64):
    ref = inp["ref"].to(dtype).clone().requires_grad_(True)
    F.relu(ref).backward(inp["dy"].to(dtype))
    return {"dx": ref.grad + inp["add"].to(dtype) if inp["add"] is not None else ref.grad}


def build_seg_act(sigmoid):
    B, K, S = 2, 3, 18
    g = _gen("seg_act", sigmoid)
    logits = 2.0 * torch.randn(B, K, S, S, generator=g)
    return {"logits": logits, "seg": torch.sigmoid(logits.double()).float(), "dseg": torch.randn(B, K, S, S, generator=g), "sigmoid": sigmoid, "shape": (B, K, S)}


def ref_seg_act(inp, dtype=torch.float64):
    o = inp["seg"].to(dtype)
    d = inp["dseg"].to(dtype) * o * (1.0 - o) * (1.0 if inp["sigmoid"] else 2.0)
    return {"dup": d.permute(0, 2, 3, 1).contiguous()}


def torch_seg_act(inp, dtype=torch.float64):
    """autograd through sigmoid(t) (ScaledTanh: (tanh(t / 2 * 2 / 2) + 1) / 2 = sigmoid(2 u) with t = 2 u) at the logits whose activation `seg` is."""
    o = inp["seg"].to(dtype)
    t = torch.logit(o).requires_grad_(True)                        # exact inverse in float64 up to rounding: the saved output defines the point
    u = (t / 2.0).detach().requires_grad_(True)
    if inp["sigmoid"]:
        torch.sigmoid(t).backward(inp["dseg"].to(dtype))
        return {"dup": t.grad.permute(0, 2, 3, 1).contiguous()}
    ((torch.tanh(u) + 1.0) / 2.0).backward(inp["dseg"].to(dtype))  # (tanh(u) + 1) / 2 = sigmoid(2 u): derivative 2 o (1 - o)
    return {"dup": u.grad.permute(0, 2, 3, 1).contiguous()}


def build_merge_scatter():
    B, R, C = 2, 6, 20
    g = _gen("merge")
    return {"dg": torch.randn(B, R // 2, R // 2, 4 * C, generator=g), "shape": (B, R, C)}


def ref_merge_scatter(inp):
    B, R, C = inp["shape"]
    dg = inp["dg"].reshape(B, R // 2, R // 2, 4, C)
    dx = torch.empty(B, R, R, C, dtype=dg.dtype)
    for x in range(2):
        for y in range(2):
            dx[:, y::2, x::2] = dg[:, :, :, y + 2 * x]
    return {"dx": dx}


def torch_merge_scatter(inp):
    B, R, C = inp["shape"]
    x = torch.zeros(B, R, R, C, dtype=torch.float64, requires_grad=True)
    cat = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)     # timm PatchMerging
    cat.backward(inp["dg"].double())
    return {"dx": x.grad}


def build_scale_rows():
    M, C, rps = 24, 12, 6
    g = _gen("scale_rows")
    return {"in": torch.randn(M, C, generator=g), "scale": torch.tensor([0.0, 1.0 / (1.0 - 0.1), 1.7, -0.3]), "shape": (M, C, rps)}


def ref_scale_rows(inp):
    M, C, rps = inp["shape"]
    return {"out": inp["in"] * inp["scale"].repeat_interleave(rps)[:, None]}        # one f32 product per element: bitwise


# ---------------- slices ----------------
REDUCTIONS = ("ln_bwd", "colsum", "colsum2", "bn_fwd", "bn_bwd", "gn_bwd", "smallk")


def row_slices(t, partial=0):
    """first / last row of a [rows][...] tensor; partial: also the rows behind the last full block of `partial` rows."""
    M = t.shape[0]
    yield "row.first", t[:1]
    yield "row.last", t[-1:]
    if partial and M % partial:
        yield f"rows.last_partial_{partial}", t[M // partial * partial:]


def column_block_slices(t, block=64):
    """the 64-column blocks one workgroup column of the reduction kernels owns (last axis)."""
    N = t.shape[-1]
    for c0 in range(0, N, block):
        yield f"cols.{c0}", t[..., c0:c0 + block]


def image_slices(t):
    """per image of an NHWC tensor: the one-pixel border ring and the interior."""
    B, H, W, _ = t.shape
    ring = torch.ones(H, W, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    for b in range(B):
        yield f"img{b}.ring", t[b][ring]
        if H > 2 and W > 2:
            yield f"img{b}.interior", t[b][~ring]


def sample_slices(t, parts=None):
    """every sample of a [B][...] tensor; parts: a [rows][C] tensor cut into that many row blocks (BatchNorm's rows are B * H * W pixels)."""
    if parts is None:
        for b in range(t.shape[0]):
            yield f"sample{b}", t[b]
    else:
        for i, blk in enumerate(torch.tensor_split(t, min(parts, t.shape[0]))):
            yield f"rows.part{i}", blk


def slices(kind: str, name: str, t: torch.Tensor):
    """Every (label, values) output `name` of a `kind` call is measured on; the whole tensor first."""
    yield "whole", t
    if t.dim() == 1 and name not in ("inv",):
        if t.numel() > 64 and kind in REDUCTIONS:        # a column sum: every 64-column block is one workgroup column
            yield from column_block_slices(t)
        return
    if kind == "ln_bwd":
        yield from row_slices(t, partial=4)
    elif kind in ("bn_fwd", "bn_bwd"):
        if name in ("y", "dx"):
            yield from row_slices(t)
            yield from sample_slices(t, parts=4)
    elif kind == "gn_bwd":
        yield from sample_slices(t)
        yield from row_slices(t.reshape(-1, t.shape[-1]))
    elif kind in ("bilinear_bwd", "maxpool_bwd"):
        yield from image_slices(t)
    elif kind in ("depth_tail", "smallk"):
        if name == "dw":
            yield from column_block_slices(t)
        else:
            yield from row_slices(t)
    elif kind == "ws_bwd":
        yield from sample_slices(t)          # each output channel: one workgroup
