"""Float64 reference of the fused MLP half-block (csrc/mlp_fused.hip, mlp_ln_kernel: x += LayerNorm(fc2(GELU(fc1(x_op)))) in one launch) as soccdpt_op_mlp_ln
runs it, with an a-priori per-element bound, plus what tests/test_mlp_fused_gpu.py and tests/test_mlp_fused_refs.py share: the case table, the two input
builders, the special rows and the check of a call's outputs.

Conventions are tests/fused_refs.py's and tests/fwd_aux_refs.py's (imported, not restated: U, gamma, gemm_gamma, round16, ln_bound, check_bound, check_copy16,
merge_layout, merge_layout_swapped, interior): the reference starts from the exact 16-bit and f32 values the kernel reads, |kernel - ref| <= bound must hold for
EVERY element, and no bound is fitted to a measured error.

The chain (u = 2^-24; fmt's gemm_gamma with the 16x16x32 MFMA: 6 roundings per k-step of 32 products):

* pre = x w1^T + b1:  e_pre = gemm_gamma(fmt, C) |x| |w1|^T + u (|x w1^T| + |b1|)  (C / 32 k-steps into a zero accumulator, one f32 addition of the bias).
* h = gelu_erf(pre):  e_h = (L + 1e-5) e_pre + gelu_fast_bound(pre).  L = 1.13 is the Lipschitz constant of GELU (its derivative Phi(x) + x phi(x) peaks at
  x = sqrt 2 with 1.1290); the 1e-5 pays for evaluating gelu_fast_bound at pre where the kernel evaluates at its own f32 pre (the bound's slope is below 1e-5).
  gelu_fast_bound follows csrc/gelu.h line by line (derivation at the function).
* The hidden tile is MODELLED, not allowed for: the kernel rounds it to the operand format on its way into LDS (as the unfused chain stores it), so
  h_mid = RN16(h), h_lo = RN16(h - e_h), h_hi = RN16(h + e_h), e_16 = max(h_hi - h_mid, h_mid - h_lo) -- zero wherever the rounding is decided ("undecided"
  elements are those with e_16 > 0; their share is reported per case, the bound pays for every one of them).  fp16 saturates at +-65504 (half16.h f2h), here too.
  This is fwd_aux_refs.check_interval16's idea applied to a value that never leaves LDS.
* v = h_mid w2^T + b2:  e_v = e_16 |w2|^T + gemm_gamma(fmt, 4C) |h_mid| |w2|^T + u (|h_mid w2^T| + |b2|).  The kernel adds the 4C / 64 chunks into one accumulator, two
  k-steps per chunk: the step count of one K = 4C product.
* t, e_t = ln_bound(v, g, beta, 1e-5, e_v) (biased variance; the cancellation term of a row whose mean is far from its spread is part of it), then
  o = xres + t with bound e_t + gamma(2) (|t| + |xres|).
* The operand copy, the merged copy and the interior of the zero-halo image are exactly RN16 of the kernel's OWN f32 output (check_copy16), in the plain layout
  or in timm PatchMerging's (merge_layout; `merged` below extends it to H != W by the same torch.cat and is checked against it on square grids).  The ring of the
  halo image keeps the bytes it had.

Two input families.  random: operands as tests/test_kernels_gpu.py::test_mlp_ln_fused draws them, pre-rounded to fmt.  dyadic: x in multiples of 1/8 with
|x| <= 2, w1 in multiples of 1/16 with |w1| <= 1/4, b1 in multiples of 1/128, so every fc1 sum is exact in f32 in any order (multiples of 2^-7 below 2^9) and
e_pre = 0 (asserted by the builder): almost every hidden rounding is then decided and the bound drops to f32 level, where a tanh-GELU, eps = 1e-6 or an unbiased
variance cannot hide.  In both families every fourth row of x (the first included) is small -- random: scaled by 0.01; dyadic: two non-zero entries -- and
b2 = 0.1 - RN16(gelu(b1)) w2^T + 0.003 noise, so that such a row's fc2 output is nearly constant over the channels and its variance sits near eps (b2 is a
free parameter of the layer; for the other rows the choice changes nothing).  The dyadic family also has one all-zero row of x (pre = b1, which holds 0 and
+-1/128); b1 ramps over [-3.5, 2.5), and rows 2, 6, 10, ... use the whole range |x| <= 2, so that pre covers [-6, 6] (dyadic_coverage; asserted on the CPU), while
the other rows keep |x| <= 1/2 and pre below about 4.5.  The reason: beyond 4.5 gelu(pre) is pre itself to within the bound on gelu_fast, pre is a multiple of
1/128, and in bf16 (one ulp = 1/32 there) every fourth such value is a rounding midpoint -- an undecided element worth a whole ulp.  They belong in the test
(the wide rows have them and the bound pays), but a few per row would lift every row's bound from f32 level (about 1e-3 here: gemm_gamma(fmt, 4C) of sum |h w2|,
amplified by |g| / sigma and ln_bound's row maximum) to several 1e-3.  Most other undecided elements sit in the negative tail pre < -3, where h is 1e-4 and
smaller and A&S's absolute 1.5e-7 is a visible fraction of it; their e_16 is of the order of e_h and costs next to nothing.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from tests.fused_refs import U, check_bound, check_copy16, gamma, gemm_gamma, round16
from tests.fwd_aux_refs import interior, ln_bound, merge_layout, merge_layout_swapped

F16_MAX = 65504.0
LN_EPS = 1e-5
GELU_LIPSCHITZ = 1.13
DT = {"bf16": torch.bfloat16, "f16": torch.float16}

# Abramowitz & Stegun 7.1.26: erf(z) = 1 - (a1 t + a2 t^2 + a3 t^3 + a4 t^4 + a5 t^5) exp(-z^2) + eps(z), t = 1 / (1 + p z), |eps| <= 1.5e-7
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
AS_ERR = 1.5e-7


def f32(x: torch.Tensor) -> torch.Tensor:
    return x.float().double()


def rnd(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def gelu64(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_fast_bound(x: torch.Tensor) -> torch.Tensor:
    """|gelu_fast(x) in f32 - gelu_erf(x)| for an f32 x, term by term from csrc/gelu.h (x float64; u = 2^-24):

    z = |x| * 0.70710678f            the constant is 1/sqrt2 rounded (u) and the product rounds (u): relative gamma(2)
    d = fmaf(0.3275911f, z, 1)       constant (u), z (2u), both on the part p z < d, and one rounding of d: relative 4u
    t = __frcp_rn(d)                 correctly rounded: relative gamma(6) with d's error; 0 < t <= 1
    P = 4 fmaf (Horner, a5 .. a1)    step k leaves u |p_k| behind, which reaches P multiplied by t^(k-1); the five rounded constants add u sum |a_i| t^(i-1); the error
                                     of t moves P by |P'(t)| t gamma(6) (P'' < 30 on [0, 1]: the 1e-5 on |P'| covers the second order)
    E = __expf(-z * z)               v_exp_f32 of arg * log2e.  The argument -z^2 carries 2 * 2u from z and u from its own product, the product with log2e (and that
                                     constant) 2u more -- a RELATIVE error of the argument, so an absolute error of the result's logarithm that grows like 7 u z^2: it is
                                     allowed as (8 z^2) u; v_exp_f32 itself is allowed 2 ulps (4u; the ISA documents 1 ulp -- taken from the documentation, not measured,
                                     and the CPU check computes this one function in float64).  All of it is multiplied by exp(-z^2): z^2 exp(-z^2) <= 1/e, so the tail costs nothing.
    Q = P * t * E                    two products (gamma(2)), in [0, 1]: |dQ| <= e_P t E + Q (gamma(6) + (8 z^2 + 4) u + gamma(2)); a flushed denormal E is below 2^-120
    e = 1 - Q                        one rounding of a value in [0, 1] (or one fma): u.  With A&S's 1.5e-7: |e - erf(z)| <= 1.5e-7 + dQ + u
    s = 1 + copysign(e, x)           for x < 0 this is 1 - e with e near 1: the ABSOLUTE error of e goes through unreduced (the cancellation of the negative tail), plus u s
    0.5f * x * s                     0.5 x is exact, the product rounds: u |gelu(x)|
    The sum is enlarged by 2^-10 for the products of two of these errors."""
    a1, a2, a3, a4, a5 = AS_A
    ax = x.abs()
    z = ax / math.sqrt(2.0)
    t = 1.0 / (1.0 + AS_P * z)
    p4 = a5 * t + a4
    p3 = p4 * t + a3
    p2 = p3 * t + a2
    p1 = p2 * t + a1
    horner = U * (p4.abs() * t ** 3 + p3.abs() * t ** 2 + p2.abs() * t + p1.abs())
    coef = U * (abs(a1) + abs(a2) * t + abs(a3) * t ** 2 + abs(a4) * t ** 3 + abs(a5) * t ** 4)
    dP = (a2 + 2 * a3 * t + 3 * a4 * t ** 2 + 4 * a5 * t ** 3).abs() + 1e-5
    e_P = horner + coef + dP * t * gamma(6)
    E = torch.exp(-z * z)
    Q = p1 * t * E
    e_Q = e_P * t * E + Q.abs() * (gamma(6) + (8 * z * z + 4) * U + gamma(2)) + 2.0 ** -120
    e_erf = AS_ERR + e_Q + U
    s = 1.0 + torch.sign(x) * torch.erf(z)
    return (0.5 * ax * (e_erf + U * s) + U * gelu64(x).abs()) * (1 + 2.0 ** -10)


def round_hidden(h: torch.Tensor, fmt: str) -> torch.Tensor:
    """half16.h f2h: round to nearest even; fp16 saturates at +-65504 instead of producing inf."""
    return round16(h.clamp(-F16_MAX, F16_MAX) if fmt == "f16" else h, fmt)


def merged(x: torch.Tensor, B: int, H: int, W: int, swapped: bool = False) -> torch.Tensor:
    """[B H W][C] -> the PatchMerging operand layout [B (H/2) (W/2)][4C].  Square grids: fwd_aux_refs.merge_layout (swapped: its planted fault); H != W: the same
    torch.cat of timm's PatchMerging, x0 = x[:, 0::2, 0::2], x1 = x[:, 1::2, 0::2], x2 = x[:, 0::2, 1::2], x3 = x[:, 1::2, 1::2] (test_mlp_fused_refs holds the two
    together on a square grid)."""
    if H == W:
        return (merge_layout_swapped if swapped else merge_layout)(x, B, H)
    return _merged_rect(x, B, H, W, swapped)


def _merged_rect(x, B, H, W, swapped=False):
    C = x.shape[-1]
    x = x.reshape(B, H, W, C)
    x0, x1, x2, x3 = x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]
    return torch.cat([x0, x2, x1, x3] if swapped else [x0, x1, x2, x3], dim=-1).reshape(-1, 4 * C)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
OUTS = ("f32", "copy", "inplace", "halo", "merge", "merge_halo")      # f32 only; + separate operand copy; x_op_out == x_op; + halo; + merged copy; + merged copy + halo
GRIDS = {"g1": (1, 2, 2), "g2": (3, 6, 4), "g3": (2, 8, 8)}           # g2: images of 24 tokens straddle the 64-token tile, H != W, a ragged last tile (72 tokens)
FLAT_M = (1, 63, 64, 65, 130)
SPECIALS = ("var0", "saturate", "shifted", "zero_row")


@dataclass(frozen=True)
class Case:
    C: int
    fmt: str
    out: str
    M: int = 0                  # without a token grid
    grid: str = ""              # a key of GRIDS
    special: str = ""

    @property
    def bhw(self):
        return GRIDS[self.grid] if self.grid else (0, 0, 0)

    @property
    def rows(self):
        B, H, W = self.bhw
        return B * H * W if self.grid else self.M

    @property
    def halo(self):
        return self.out in ("halo", "merge_halo")

    @property
    def merge(self):
        return self.out in ("merge", "merge_halo")

    @property
    def name(self):
        return f"c{self.C}_{self.fmt}_{self.grid or 'm%d' % self.M}_{self.out}" + (f"_{self.special}" if self.special else "")


def _table():
    t = []
    add = lambda C, fmt, out, where: t.append(Case(C, fmt, out, grid=where) if isinstance(where, str) else Case(C, fmt, out, M=where))
    # C = 96: every output variant, the merge variants on all three grids
    add(96, "bf16", "f32", 1), add(96, "f16", "copy", 63), add(96, "bf16", "inplace", 65), add(96, "f16", "halo", "g2")
    add(96, "bf16", "merge", "g1"), add(96, "f16", "merge", "g2"), add(96, "bf16", "merge_halo", "g3"), add(96, "f16", "merge_halo", "g1")
    # C = 128
    add(128, "f16", "f32", 64), add(128, "bf16", "copy", 130), add(128, "bf16", "inplace", 63), add(128, "bf16", "halo", "g3")
    add(128, "f16", "merge", "g3"), add(128, "bf16", "merge_halo", "g2"), add(128, "f16", "inplace", "g1")
    # C = 192
    add(192, "bf16", "f32", 65), add(192, "f16", "copy", 1), add(192, "f16", "inplace", 130), add(192, "f16", "halo", "g1")
    add(192, "bf16", "merge", "g2"), add(192, "f16", "merge_halo", "g3"), add(192, "bf16", "halo", "g1")
    # C = 256 (the SWZ = 15 row layout, like 128; 16 hidden chunks)
    add(256, "f16", "f32", 130), add(256, "bf16", "copy", 64), add(256, "f16", "inplace", 65), add(256, "bf16", "merge_halo", "g1"), add(256, "f16", "halo", "g2")
    add(256, "bf16", "f32", 1), add(256, "f16", "copy", 64), add(256, "bf16", "merge", "g3")
    return {c.name: c for c in t}


CASES = _table()
# special rows as cases of their own, each built on the random family (build)
SPECIAL_CASES = {c.name: c for c in (
    Case(96, "bf16", "copy", M=65, special="var0"), Case(128, "f16", "copy", M=65, special="var0"),           # w2 = 0, b2 constant: o = xres + beta bitwise
    Case(128, "f16", "copy", M=65, special="saturate"), Case(192, "f16", "halo", grid="g2", special="saturate"),  # hidden beyond 65504: saturates, output finite
    Case(96, "f16", "copy", M=65, special="shifted"), Case(192, "bf16", "copy", M=63, special="shifted"),      # fc2 output with mean 50 and spread 0.5
    Case(96, "bf16", "copy", M=65, special="zero_row"), Case(128, "f16", "copy", M=130, special="zero_row"))}   # a row of x all zero: pre = b1
FAMILIES = ("random", "dyadic")


def find(name):
    return CASES.get(name) or SPECIAL_CASES[name]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (float64 tensors holding exact operand values)
# ---------------------------------------------------------------------------------------------------------------------------------
def _tail(inp, C, fmt, seed, b2="near_eps"):
    """w2, b2, the LayerNorm's g / beta and the residual, common to both families."""
    w2 = round16(rnd((C, 4 * C), seed + 10, 1 / math.sqrt(4 * C)), fmt)
    if b2 == "near_eps":
        h0 = round_hidden(gelu64(inp["b1"]), fmt)
        b2v = 0.1 - h0 @ w2.t() + rnd((C,), seed + 11, 0.003)
    else:
        b2v = rnd((C,), seed + 11, 0.2)
    M = inp["x"].shape[0]
    inp.update(w2=w2, b2=f32(b2v), g=f32(1.0 + 0.3 * rnd((C,), seed + 12)), beta=f32(0.2 * rnd((C,), seed + 13)), xres=f32(rnd((M, C), seed + 14)))
    return inp


def build_random(case: Case, seed=0):
    M, C, fmt = case.rows, case.C, case.fmt
    seed = seed + 1000 * C + M
    scale = torch.tensor([0.01, 1.0, 1.5, 0.5], dtype=torch.float64)[torch.arange(M) % 4][:, None]
    inp = {"x": round16(rnd((M, C), seed) * scale, fmt), "w1": round16(rnd((4 * C, C), seed + 1, 1 / math.sqrt(C)), fmt), "b1": f32(rnd((4 * C,), seed + 2, 0.2))}
    return _tail(inp, C, fmt, seed)


def build_dyadic(case: Case, seed=0):
    M, C, fmt = case.rows, case.C, case.fmt
    seed = seed + 1000 * C + M + 500
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-16, 17, (M, C), generator=g).double() / 8
    narrow = (torch.arange(M) % 4 != 2)[:, None]                         # rows 2, 6, 10, ... keep |x| <= 2 and reach |pre| = 6; the others keep |x| <= 1/2 and pre below ~ 4.5
    x = torch.where(narrow, torch.randint(-4, 5, (M, C), generator=g).double() / 8, x)
    small =(torch.arange(M) % 4 == 0)[:, None] & (torch.arange(C)[None, :] % (C // 2) != (torch.arange(M)[:, None] * 7) % (C // 2))
    x = torch.where(small, torch.zeros_like(x), x)                       # every fourth row: two entries survive
    if M >= 3:
        x[M // 3] = 0.0                                                  # pre = b1
    w1 = torch.randint(-4, 5, (4 * C, C), generator=g).double() / 16
    j = torch.arange(4 * C)
    b1 = (torch.round((j * 37 % (4 * C)).double() / (4 * C) * 768) - 448) / 128       # a ramp over [-3.5, 2.5), scattered over the chunks
    b1[:3] = torch.tensor([0.0, 1 / 128, -1 / 128], dtype=torch.float64)
    inp = {"x": x, "w1": w1, "b1": b1}
    for k, unit in (("x", 8), ("w1", 16), ("b1", 128)):
        assert torch.equal(inp[k] * unit, (inp[k] * unit).round()) and torch.equal(round16(inp[k], fmt) if k != "b1" else f32(inp[k]), inp[k]), k
    mag = x.abs() @ w1.abs().t() + b1.abs()
    assert float(x.abs().max()) <= 2 and float(w1.abs().max()) <= 1 and float(mag.max()) < 512, "every partial fc1 sum is a multiple of 2^-7 below 2^9: exact in f32"
    return _tail(inp, C, fmt, seed)


def build(case: Case, family: str):
    """The operands of one case.  A special case builds on the random family (var0, saturate, shifted, zero_row)."""
    if not case.special:
        return build_dyadic(case) if family == "dyadic" else build_random(case)
    inp = build_random(case, seed=77)
    C, M = case.C, case.rows
    if case.special == "var0":
        inp["w2"] = torch.zeros_like(inp["w2"])
        inp["b2"] = torch.full_like(inp["b2"], 0.75)
    elif case.special == "saturate":      # eight hidden units of chunk 0 and of the last chunk far beyond fp16's range, on both sides (gelu(-1e5) = -0)
        inp["b1"][0:8] = 1.0e5
        inp["b1"][8:16] = -1.0e5
        inp["b1"][-8:] = 7.0e4
        inp["w1"][21] = round16(inp["w1"][21] * 256, case.fmt)                                  # and one through x w1^T: unit 21 of row M / 2 + 1 gets
        inp["x"][M // 2 + 1] = 64.0 * torch.sign(inp["w1"][21]) + (inp["w1"][21] == 0).double()   # 64 sum |w1[21]| ~ 64 C 0.08 256 > 65504 (asserted on the CPU)
    elif case.special == "shifted":
        inp["b2"] = f32(50.0 + rnd((C,), 91, 0.2))
    elif case.special == "zero_row":
        inp["x"][M // 2 + 1] = 0.0                                                              # a row of ordinary scale (row 33 of 65, 66 of 130)
    return inp


def dyadic_coverage(inp):
    """What the dyadic family promises about pre = x w1^T + b1 (exact): the occupied half-unit bins of [-6, 6], and the counts of pre == 0, 0 < pre <= 1/16,
    -1/16 <= pre < 0 and pre <= -4 (the tail where 1 - p t exp(-z^2) cancels)."""
    pre = inp["x"] @ inp["w1"].t() + inp["b1"]
    bins = torch.histc(pre.clamp(-6, 6 - 1e-9), bins=24, min=-6, max=6)
    return {"empty_bins": int((bins == 0).sum()), "zero": int((pre == 0).sum()), "small_pos": int(((pre > 0) & (pre <= 1 / 16)).sum()),
            "small_neg": int(((pre < 0) & (pre >= -1 / 16)).sum()), "tail": int((pre <= -4).sum())}


# ---------------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------------
def reference(inp, fmt):
    """-> dict: o, e_o [M][C] (the f32 output and its bound), undecided (share of hidden elements whose 16-bit rounding e_h leaves open), and the intermediates."""
    x, w1, b1, w2, b2 = inp["x"], inp["w1"], inp["b1"], inp["w2"], inp["b2"]
    C = x.shape[1]
    acc1 = x @ w1.t()
    pre = acc1 + b1
    e_pre = gemm_gamma(fmt, C) * (x.abs() @ w1.abs().t()) + U * (acc1.abs() + b1.abs())
    if inp.get("exact_fc1"):
        e_pre = torch.zeros_like(e_pre)
    h = gelu64(pre)
    e_h = (GELU_LIPSCHITZ + 1e-5) * e_pre + gelu_fast_bound(pre)
    h_mid, h_lo, h_hi = round_hidden(h, fmt), round_hidden(h - e_h, fmt), round_hidden(h + e_h, fmt)
    e_16 = torch.maximum(h_hi - h_mid, h_mid - h_lo)
    acc2 = h_mid @ w2.t()
    v = acc2 + b2
    e_v = e_16 @ w2.abs().t() + gemm_gamma(fmt, 4 * C) * (h_mid.abs() @ w2.abs().t()) + U * (acc2.abs() + b2.abs())
    t, e_t = ln_bound(v, inp["g"], inp["beta"], LN_EPS, e_v)
    o = inp["xres"] + t
    return {"o": o, "e_o": e_t + gamma(2) * (t.abs() + inp["xres"].abs()), "undecided": float((e_16 > 0).double().mean()), "pre": pre, "e_pre": e_pre, "h": h, "e_h": e_h,
            "h_mid": h_mid, "e_16": e_16, "v": v, "e_v": e_v, "t": t}


def case_reference(case: Case, family: str, inp):
    """reference() with the dyadic family's claim applied: e_pre = 0 (build_dyadic asserted that every fc1 sum is exact)."""
    return reference(dict(inp, exact_fc1=(family == "dyadic" and not case.special)), case.fmt)


# ---------------------------------------------------------------------------------------------------------------------------------
# the check of one call's outputs, shared by the GPU tests and the CPU emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def check_outputs(case: Case, inp, ref, got, what):
    """got: {"xf": f32 [M][C], "xop": the 16-bit tensor x_op_out pointed at ([M][C], merged [M/4][4C]) or None, "halo": 16-bit [B][H+2][W+2][C] or None}, every
    buffer 0xFF bytes before the call (xf: the residual).  Returns worst error / bound of the f32 output."""
    M, C = case.rows, case.C
    B, H, W = case.bhw
    xf = got["xf"].cpu()
    assert xf.dtype == torch.float32 and tuple(xf.shape) == (M, C)
    if case.special == "var0":         # variance exactly 0: (v - mean) = 0, so t = beta and o = xres + beta in one f32 addition
        want = inp["xres"].float() + inp["beta"].float()
        assert torch.equal(xf.view(torch.int32), want.view(torch.int32)), f"{what}: a row of variance 0 is not xres + beta bit for bit"
    ratio = check_bound(xf, ref["o"], ref["e_o"], f"{what} x_f32")
    assert bool(torch.isfinite(xf).all())
    if case.out == "f32":
        assert got["xop"] is None
    else:
        twin = merged(xf, B, H, W) if case.merge else xf
        if case.out != "halo":
            check_copy16(got["xop"].cpu().reshape(twin.shape), twin, case.fmt, f"{what} operand copy" + (" (PatchMerging layout)" if case.merge else ""))
    if case.halo:
        halo = got["halo"].cpu()
        assert tuple(halo.shape) == (B, H + 2, W + 2, C)
        ring = torch.ones(B, H + 2, W + 2, dtype=torch.bool)
        ring[:, 1:-1, 1:-1] = False
        assert bool((halo.view(torch.int16)[ring] == -1).all()), f"{what}: the ring of the zero-halo image was written"
        check_copy16(interior(halo).contiguous(), xf.reshape(B, H, W, C), case.fmt, f"{what} halo interior")
    else:
        assert got["halo"] is None
    return ratio
