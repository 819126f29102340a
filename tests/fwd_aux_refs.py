"""Float64 references of the forward path's non-GEMM launchers (csrc/elementwise.hip, csrc/hybrid.hip) as soccdpt_op_fwd_aux runs them, each with an
a-priori per-element bound, plus what tests/test_fwd_aux_gpu.py and tests/test_fwd_aux_refs.py share: case tables, input builders and the description of
every call (`Call`).

Conventions are tests/fused_refs.py's (imported, not restated: gamma, round16, bilinear_sample and its f32 position allowance, LERP_SLACK, the
monotone-activation interval of seg_up_act_ref, check_bound / check_copy16 / check_x3): every reference starts from the exact f32 / 16-bit operand values
the kernel reads, |kernel - ref| <= bound must hold for EVERY element, and no bound is fitted to a measured error.  How an output is held to it:

* an f32 output: |kernel - ref| <= bound;
* a 16-bit copy written beside an f32 output of the same launch: exactly RN16 of that f32 output (check_copy16); an x3 copy: check_x3;
* a 16-bit output with no f32 twin: inside [RN16(ref - bound), RN16(ref + bound)] (check_interval16); an x3 one: hi inside that fp16 interval and
  hi + lo / 2048 within bound + 2^-23 |ref| + 2^-36 of ref (check_x3_interval);
* permutations, selections and single roundings (merge_gather, stem_im2col, qkv_bias, cvt, conv_w without scale, the token sum of vit_tokens_ln, the
  identity position-embedding resize): bitwise.

Bound models (u = 2^-24, gamma(n) as in fused_refs):

* LayerNorm of a row v of N values (ln_bound; the model of fused_refs.ln_epilogue_ref with the input error as a parameter): an input error e_v moves the
  output by |g| / sigma (e_v + max e_v (1 + |yhat|)); the f32 statistics add |g| ((|yhat| + 1) gamma(2N + 8) + gamma(N + 2) max|v| / sigma) -- the last
  term is the cancellation of a row whose mean is far from zero compared with its spread ("shifted" rows: it is part of the bound, such rows are compared
  like any other); the affine tail gamma(4) (|yhat g| + |b|).
* patch_embed: v = 48 products + bias in two fma chains: e_v = gamma(52) (sum |x w| + |bias|), then ln_bound.
* ln_residual: o = t * row_scale + xres with t = LN(y) g + beta: bound(t) |row_scale| + gamma(3) (|t row_scale| + |xres|).
* bilinear: fused_refs.bilinear_sample.
* seg tail classifier: a lane's 16 channels (<= 32 roundings), four shuffle adds, the bias: gamma(48) (sum |x w| + |bias|); the up-sampling and activation from
  the kernel's OWN logits (the values its second kernel reads): fused_refs.seg_up_act_ref.
* conv_w with scale: one product, u |w s|.  bn_fold: s = g / sqrt(var + eps): an add, a square root, a division, each allowed 2 ulps: gamma(8) |s|;
  shift = b - mean s: |mean| e_s + gamma(3) (|b| + |mean s|).  logit_scale: expf within 4 ulps.
* cpb_table: coordinates sign(c) log2(|c| + 1) / 3 with c = d / denom * 8: a division, log2f, a division, allowed gamma(8) |coord|; hidden unit
  relu(w0a cy + w0b cx + b0): |w0a| e_cy + |w0b| e_cx + gamma(3) (|w0a cy| + |w0b cx| + |b0|); the 512-term serial sum: sum e_h |w2| + gamma(512 + 2) sum (h + e_h) |w2|;
  16 sigmoid is 4-Lipschitz: 4 e_s + 8 u |table| for expf and the division.
* ws_conv_w: the kernel's statistics are f64 sums; v = (w - f32(mean)) * f32(rstd): rstd u (|mean| + |w - mean|) + |v| (2 u + r) where r is the relative error
  of rstd from the f64 cancellation in E[w^2] - mean^2: 2^-50 E[w^2] / (2 (var + eps)).  An all-equal filter has var = 0 and v = 0: its bound is rstd u |mean|
  with rstd = 1 / sqrt(eps).
* gn_relu_maxpool: per tap gamma(4) (|x - mean| rstd |g| + |b|) (a subtraction, two products, an addition); relu and max are 1-Lipschitz in the sup norm, so the
  window's bound is the largest tap bound.  The builder still keeps every window's best and second-best positive values 1e-3 apart (pool_gaps; checked on
  the CPU), so a kernel that picks the wrong tap cannot hide inside the bound.
* vit_tokens_ln: xf = y + pos is one rounding (bitwise f32 sum); the LayerNorm from the kernel's own xf: ln_bound with e_v = 0, eps = f[0].
* pos_embed_resize: bilinear_sample with align_corners=False (half-pixel positions, fused_refs._f32_halfpixel_error).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from tests import fused_refs as FR
from tests.fused_refs import U, gamma, round16

FMT16 = {0: "bf16", 1: "f16"}
KINDS = ("patch_embed", "ln_residual", "merge_gather", "bilinear", "seg_tail", "cvt", "conv_w", "bn_fold", "qkv_bias", "logit_scale", "cpb_table", "ws_conv_w",
         "stem_im2col", "gn_relu_maxpool", "vit_tokens_ln", "ln_rows", "pos_embed_resize")
PATH_LN_SCALAR, PATH_LN_V4 = 0x100, 0x200
POOL_GAP = 1e-3


def f32(x: torch.Tensor) -> torch.Tensor:
    """float64 -> the nearest f32 value, as float64."""
    return x.float().double()


def rnd(shape, seed, scale=1.0):
    return f32(torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


def flags_of(bits=0, fmt=0, halo_fmt=None):
    return bits | (fmt << 4) | ((0 if halo_fmt is None else halo_fmt + 1) << 8)


def op_dtype(fmt):
    """torch dtype and elements per value of an operand tensor in format fmt (hf / out_mode; x3 = two fp16 words per element)."""
    return {0: (torch.bfloat16, 1), 1: (torch.float16, 1), 2: (torch.float32, 1), 3: (torch.float16, 2), 5: (torch.float16, 1)}[fmt]


@dataclass
class Call:
    """One soccdpt_op_fwd_aux call.  ins: host tensors (already in the dtype the kernel reads) or None; outs: None or (name, shape, fmt) with fmt an operand
    format (2 = f32) -- an x3 output is a flat fp16 tensor of 2 * numel words; preset: name -> host tensor the output holds beforehand (read-modify-write);
    halo: names of zero-halo outputs [B][H+2][W+2][C] whose ring must stay untouched."""
    kind: str
    dim: list
    flags: int = 0
    f: tuple = (0.0, 0.0, 0.0)
    ins: list = field(default_factory=list)
    outs: list = field(default_factory=list)
    preset: dict = field(default_factory=dict)
    halo: tuple = ()
    finite: bool = True


# ---------------------------------------------------------------------------------------------------------------------------------
# checks beyond fused_refs'
# ---------------------------------------------------------------------------------------------------------------------------------
def check_interval16(got, ref, bound, fmt, what):
    """A 16-bit output with no f32 twin lies in [RN16(ref - bound), RN16(ref + bound)]."""
    g = got.double().cpu()
    lo, hi = round16(ref - bound, fmt), round16(ref + bound, fmt)
    bad = ~((g >= lo) & (g <= hi))
    if bad.any():
        t = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} 16-bit values outside [RN16(ref - bound), RN16(ref + bound)]; first at {t}: got {float(g[t])!r}, "
                             f"ref {float(ref[t])!r}, bound {float(bound[t]):.3e}")
    err = (g - ref).abs()
    return float((err / torch.maximum(ref - lo, hi - ref).clamp(min=1e-300)).max()) if err.numel() else 0.0


def check_x3_interval(raw, shape, ref, bound, what):
    """An x3 output with no f32 twin: hi in the fp16 interval, and the decoded pair within bound + 2^-23 |ref| + 2^-36 of ref."""
    return check_x3_interval_parts(*FR.x3_parts(raw, shape), ref, bound, what)


def check_x3_interval_parts(hi, lo, ref, bound, what):
    """The same on decoded (hi, lo) values -- for a part of an x3 tensor, such as the interior of a zero-halo image."""
    check_interval16(hi, ref, bound, "f16", what + " (x3 hi)")
    return FR.check_bound(hi + lo / 2048.0, ref, bound + 2.0 ** -23 * ref.abs() + 2.0 ** -36, what + " (x3 decode)")


def x3_words(raw, shape):
    """Flat x3 storage -> the (hi, lo) 16-bit words as int16 tensors of `shape` (the layout of fused_refs.x3_parts)."""
    r = raw.cpu().view(torch.int16).reshape(-1, 2, 8)
    odd = (torch.arange(r.shape[0]) & 1).bool()[:, None]
    return torch.where(odd, r[:, 1], r[:, 0]).reshape(shape), torch.where(odd, r[:, 0], r[:, 1]).reshape(shape)


def check_op(got, fmt, shape, ref, bound, what, twin=None):
    """An operand output `got` in format fmt against (ref, bound), or -- when the launch also wrote the f32 values `twin` -- against the copy rule."""
    if fmt == 2:
        if twin is not None:
            assert torch.equal(got.view(torch.int32), twin.view(torch.int32)), f"{what}: the two f32 outputs of one launch differ"
            return 0.0
        return FR.check_bound(got, ref, bound, what)
    if fmt == 3:
        if twin is not None:
            return FR.check_x3(got, shape, twin, what)
        return check_x3_interval(got, shape, ref, bound, what)
    if twin is not None:
        FR.check_copy16(got, twin, FMT16[fmt], what)
        return 0.0
    return check_interval16(got, ref, bound, FMT16[fmt], what)


def interior(t):
    return t[:, 1:-1, 1:-1]


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm model
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_bound(v, g, b, eps, e_v=None, unbiased=False):
    """t = LN(v) g + b over the last axis (biased variance) in float64 and its bound; e_v: bound on the error of v itself (same shape) or None."""
    N = v.shape[-1]
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).sum(-1, keepdim=True) / (N - 1 if unbiased else N)
    sigma = (var + eps).sqrt()
    yh = (v - mean) / sigma
    t = yh * g + b
    bound = g.abs() * ((yh.abs() + 1) * gamma(2 * N + 8) + gamma(N + 2) * v.abs().max(-1, keepdim=True).values / sigma) + gamma(4) * ((yh * g).abs() + b.abs())
    if e_v is not None:
        bound = bound + g.abs() / sigma * (e_v + e_v.max(-1, keepdim=True).values * (1 + yh.abs()))
    return t, bound


def ln_inputs(M, C, seed, shifted=False):
    """Rows with a distinct offset and scale each -- every fourth one, the first included, with a spread of 0.01, where eps matters; shifted: row M // 2 has mean 50
    and spread 0.5."""
    scale = torch.tensor([0.01, 1.5, 2.5, 0.5], dtype=torch.float64)[torch.arange(M) % 4][:, None]
    y = rnd((M, C), seed) * scale + 0.3 * (torch.arange(M, dtype=torch.float64)[:, None] % 5 - 2)
    if shifted:
        y[M // 2] = 50.0 + 0.5 * rnd((C,), seed + 1)
    g = 1.0 + 0.3 * rnd((C,), seed + 2)
    b = 0.2 * rnd((C,), seed + 3)
    return f32(y), f32(g), f32(b)


# ---------------------------------------------------------------------------------------------------------------------------------
# PATCH_EMBED
# ---------------------------------------------------------------------------------------------------------------------------------
#                     B, S, C0, shifted
PATCH_CASES = {"1x32x96": (1, 32, 96, False), "3x64x128": (3, 64, 128, False), "1x32x40": (1, 32, 40, False), "8x384x40": (8, 384, 40, False),
               "1x32x96_shifted": (1, 32, 96, True)}
PATCH_RUNS = [("1x32x96", None), ("1x32x96", 0), ("1x32x96", 1), ("1x32x96", 3), ("3x64x128", 1), ("3x64x128", 3), ("1x32x40", 0), ("1x32x40", None), ("8x384x40", None),
              ("1x32x96_shifted", 1)]


def build_patch(case):
    B, S, C0, shifted = PATCH_CASES[case]
    x = rnd((B, 3, S, S), 11) + 0.2 * torch.arange(B, dtype=torch.float64)[:, None, None, None]
    w = rnd((C0, 48), 12, 1 / math.sqrt(48))
    bias = rnd((C0,), 13, 0.3) + (30.0 if shifted else 0.0)
    g, beta = 1.0 + 0.3 * rnd((C0,), 14), 0.2 * rnd((C0,), 15)
    return {"x": f32(x), "w": w, "bias": f32(bias), "g": f32(g), "beta": f32(beta)}


def ref_patch(inp, eps=1e-5, unbiased=False):
    C0 = inp["w"].shape[0]
    wk = inp["w"].view(C0, 3, 4, 4)
    v = F.conv2d(inp["x"], wk, inp["bias"], stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
    mag = F.conv2d(inp["x"].abs(), wk.abs(), inp["bias"].abs(), stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
    wT = torch.zeros(48, 128, dtype=torch.float64)
    wT[:, :C0] = inp["w"].t()
    t, bound = ln_bound(v, inp["g"], inp["beta"], eps, gamma(52) * mag, unbiased)
    return {"xf": (t, bound), "wT": wT}


def call_patch(case, fmt, inp):
    B, S, C0, _ = PATCH_CASES[case]
    M = B * (S // 4) ** 2
    return Call("patch_embed", [B, S, C0], flags_of(0, fmt or 0), ins=[inp[k].float() for k in ("x", "w", "bias", "g", "beta")],
                outs=[("xf", (M, C0), 2), None if fmt is None else ("xb", (M, C0), fmt), ("wT", (48, 128), 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# LN_RESIDUAL
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class LnCase:
    M: int
    C: int
    residual: int = 1
    fmt: int = 0                 # hf of xb
    xb: bool = True
    merge: int = 0
    res: int = 0
    halo: object = None          # None, "op" or "f32"
    halo_fmt: object = None      # hf_halo when it differs
    rps: int = 0                 # rows_per_scale (0: no row_scale)
    shifted: bool = False
    path: int = 0


def _ln(M, C, path, **kw):
    return LnCase(M, C, path=path, **kw)


LN_CASES = {
    "c96_m1": _ln(1, 96, PATH_LN_SCALAR | 2), "c100_m5": _ln(5, 100, PATH_LN_SCALAR | 2, residual=0, fmt=1), "c192_m23": _ln(23, 192, PATH_LN_SCALAR | 4, fmt=3),
    "c384_m7": _ln(7, 384, PATH_LN_SCALAR | 8, xb=False), "c576_m5": _ln(5, 576, PATH_LN_SCALAR | 12), "c1000_m7": _ln(7, 1000, PATH_LN_SCALAR | 16, residual=0, fmt=1),
    "c256_m1": _ln(1, 256, PATH_LN_V4 | 1, fmt=1), "c512_m5": _ln(5, 512, PATH_LN_V4 | 2, residual=0), "c768_m23": _ln(23, 768, PATH_LN_V4 | 3, fmt=3),
    "c1024_m7": _ln(7, 1024, PATH_LN_V4 | 4, fmt=1),
    "merge_r2_c96": _ln(8, 96, PATH_LN_SCALAR | 2, merge=1, res=2), "merge_r6_c256": _ln(72, 256, PATH_LN_V4 | 1, merge=1, res=6, fmt=1, residual=0),
    "merge_r6_c192_x3": _ln(72, 192, PATH_LN_SCALAR | 4, merge=1, res=6, fmt=3),
    "halo16_c192": _ln(18, 192, PATH_LN_SCALAR | 4, res=3, fmt=1, halo="op"), "halo16_c256": _ln(18, 256, PATH_LN_V4 | 1, res=3, fmt=0, halo="op", xb=False),
    "halof32_c256": _ln(18, 256, PATH_LN_V4 | 1, res=3, xb=False, halo="f32"), "halof32_c100": _ln(18, 100, PATH_LN_SCALAR | 2, res=3, fmt=1, halo="f32"),
    "rowscale_c96": _ln(11, 96, PATH_LN_SCALAR | 2, res=2, rps=4, fmt=1), "rowscale_c512": _ln(11, 512, PATH_LN_V4 | 2, res=2, rps=4, xb=False),
    "x3halo_f16_c256": _ln(8, 256, PATH_LN_V4 | 1, res=2, fmt=1, halo="op", halo_fmt=3), "x3halo_f16_c96": _ln(8, 96, PATH_LN_SCALAR | 2, res=2, fmt=1, halo="op", halo_fmt=3),
    "c768_shifted": _ln(5, 768, PATH_LN_V4 | 3, shifted=True, fmt=1), "c100_shifted": _ln(7, 100, PATH_LN_SCALAR | 2, shifted=True, residual=0, fmt=1),
}


def build_ln(case):
    c = LN_CASES[case]
    y, g, b = ln_inputs(c.M, c.C, 21, c.shifted)
    inp = {"y": y, "g": g, "beta": b, "xf0": rnd((c.M, c.C), 25)}
    if c.rps:
        n = -(-c.M // c.rps)
        inp["row_scale"] = f32(torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.8, 1.25, 0.5][:n], dtype=torch.float64))
    return inp


def ref_ln(case, inp, eps=1e-5, unbiased=False):
    c = LN_CASES[case]
    t, bt = ln_bound(inp["y"], inp["g"], inp["beta"], eps, None, unbiased)
    rs = inp["row_scale"][torch.arange(c.M) // c.rps][:, None] if c.rps else torch.ones(c.M, 1, dtype=torch.float64)
    xres = inp["xf0"] if c.residual else torch.zeros_like(t)
    return t * rs + xres, bt * rs.abs() + gamma(3) * ((t * rs).abs() + xres.abs())


def merge_layout(x, B, res):
    """[B res^2][C] -> PatchMerging operand layout [B (res/2)^2][4C], channel blocks (0,0), (1,0), (0,1), (1,1) = (dy, dx) (timm PatchMerging)."""
    C = x.shape[-1]
    x = x.reshape(B, res, res, C)
    return torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], dim=-1).reshape(-1, 4 * C)


def merge_layout_swapped(x, B, res):
    """The planted fault: blocks (1,0) and (0,1) exchanged."""
    C = x.shape[-1]
    x = x.reshape(B, res, res, C)
    return torch.cat([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], dim=-1).reshape(-1, 4 * C)


def call_ln(case, inp):
    c = LN_CASES[case]
    B = c.M // (c.res * c.res) if c.res and c.M % (c.res * c.res) == 0 else 0
    hshape = (B, c.res + 2, c.res + 2, c.C)
    hfmt = c.fmt if c.halo_fmt is None else c.halo_fmt
    outs = [("xf", (c.M, c.C), 2), ("xb", (c.M // 4, 4 * c.C) if c.merge else (c.M, c.C), c.fmt) if c.xb else None,
            ("halo", hshape, hfmt) if c.halo == "op" else None, ("halo_f32", hshape, 2) if c.halo == "f32" else None]
    return Call("ln_residual", [c.M, c.C, c.res, c.rps], flags_of(c.residual | (c.merge << 1), c.fmt, c.halo_fmt),
                ins=[inp["y"].float(), inp["g"].float(), inp["beta"].float(), inp["row_scale"].float() if c.rps else None], outs=outs,
                preset={"xf": inp["xf0"].float()} if c.residual else {}, halo=("halo", "halo_f32"))


# ---------------------------------------------------------------------------------------------------------------------------------
# MERGE_GATHER (bitwise)
# ---------------------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(2, 2, 8, 2), (1, 6, 4, 4), (2, 6, 24, 2), (2, 32, 1056, 4)]       # B, R, C, elem_bytes; the last: 540,672 chunks > 2048 * 256


def build_merge(shape):
    B, R, C, eb = shape
    n = B * R * R * C
    v = torch.arange(n, dtype=torch.int64)
    x = (v * 2654435761 % (1 << (8 * eb - 1))).to(torch.int16 if eb == 2 else torch.int32)       # distinct-looking words, no symmetry between positions
    return {"in": x.reshape(B * R * R, C)}


def call_merge(shape, inp):
    B, R, C, eb = shape
    return Call("merge_gather", [B, R, C, eb], ins=[inp["in"]], outs=[("out", (B * (R // 2) ** 2, 4 * C), inp["in"].dtype)])


# ---------------------------------------------------------------------------------------------------------------------------------
# BILINEAR
# ---------------------------------------------------------------------------------------------------------------------------------
BILINEAR_SHAPES = {"identity": (2, 3, 4, 3, 4), "x2": (1, 4, 5, 8, 10), "nonint": (2, 5, 7, 7, 10), "h1": (1, 1, 6, 4, 9), "w1": (2, 6, 1, 9, 3), "one": (1, 3, 3, 1, 1)}
BILINEAR_BIG = (1, 725, 725, 1450, 1450, 4)         # 2,102,500 threads > 8192 * 256: the grid-stride loop of the generic kernel


def build_bilinear(shape, C, in_fmt=None, seed=31):
    """A map with a ramp (so that a wrong weight shows), noise, a distinct offset per batch row; in_fmt: round to that 16-bit format."""
    B, h, w = shape[:3]
    x = rnd((B, h, w, C), seed) + torch.arange(h, dtype=torch.float64)[None, :, None, None] * 0.7 - torch.arange(w, dtype=torch.float64)[None, None, :, None] * 0.4
    x = x + torch.arange(B, dtype=torch.float64)[:, None, None, None]
    return {"in": f32(x) if in_fmt is None else round16(x, FMT16[in_fmt])}


def ref_bilinear(inp, shape, align_corners=True, rows=None):
    """(ref, bound) [B][H][W][C]; rows: a slice of output rows (the big case is evaluated in bands)."""
    B, H, W = shape[0], shape[3], shape[4]
    ys = torch.arange(H)[rows] if rows is not None else torch.arange(H)
    b = torch.arange(B)[:, None, None].expand(B, len(ys), W)
    Y = ys[None, :, None].expand(B, len(ys), W)
    X = torch.arange(W)[None, None, :].expand(B, len(ys), W)
    return FR.bilinear_sample(inp["in"], b, Y, X, H, W, align_corners)


def call_bilinear(shape, C, inp, in_fmt=None, fmt=0, f32_plain=False, op=None, f32_halo=False):
    """op: None, "plain" or "halo" (the operand output, format fmt)."""
    B, h, w, H, W = shape[:5]
    x = inp["in"].float() if in_fmt is None else inp["in"].to(op_dtype(in_fmt)[0])
    hs = (B, H + 2, W + 2, C)
    outs = [("out_f32", (B, H, W, C), 2) if f32_plain else None, None if op is None else ("out_op", hs if op == "halo" else (B, H, W, C), fmt),
            ("out_f32_halo", hs, 2) if f32_halo else None]
    return Call("bilinear", [B, h, w, H, W, C], flags_of((1 if in_fmt is not None else 0) | (2 if op == "halo" else 0), fmt), ins=[x], outs=outs,
                halo=(("out_op",) if op == "halo" else ()) + ("out_f32_halo",))


# ---------------------------------------------------------------------------------------------------------------------------------
# SEG_TAIL
# ---------------------------------------------------------------------------------------------------------------------------------
SEG_SHAPES = [(1, 1, 1), (1, 1, 3), (1, 3, 6), (1, 192, 192)]      # M = 1, 3, 18 and 36,864 > 2048 * 16 pixels


def build_seg(shape, fmt, seed=41):
    """fmt: 0 / 1 = 16-bit features, 2 = f32.  Three different classifier rows and biases."""
    B, h, w = shape
    M = B * h * w
    x = rnd((M, 256), seed) + 0.1
    wt = rnd((3, 256), seed + 1, 1 / 16.0)
    wt[1] += 0.02
    wt[2] -= 0.02
    return {"feat": f32(x) if fmt == 2 else round16(x, FMT16[fmt]), "w": f32(wt), "bias": f32(torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64))}


def ref_seg_logits(inp):
    v = inp["feat"] @ inp["w"].t() + inp["bias"]
    return v, gamma(48) * (inp["feat"].abs() @ inp["w"].abs().t() + inp["bias"].abs())


def call_seg(shape, fmt, sigmoid, inp):
    B, h, w = shape
    feat = inp["feat"].float() if fmt == 2 else inp["feat"].to(op_dtype(fmt)[0])
    return Call("seg_tail", [B, h, w], flags_of(sigmoid | (2 if fmt == 2 else 0), 0 if fmt == 2 else fmt), ins=[feat, inp["w"].float(), inp["bias"].float()],
                outs=[("tmp", (B * h * w, 3), 2), ("seg", (B, 3, 2 * h, 2 * w), 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# one-time weight preparation: CVT, CONV_W, BN_FOLD, QKV_BIAS, LOGIT_SCALE, CPB_TABLE
# ---------------------------------------------------------------------------------------------------------------------------------
CVT_SIZES = {0: [1, 1000, 600000], 1: [1, 1000, 600000], 3: [16, 1008, 600000], 5: [1, 1000, 600000]}     # 600,000 > 2048 * 256: the strided loop
F16_MAX = 65504.0


def build_cvt(n, fmt, seed=51):
    """Values over many binades, exact zeros, ties of the 16-bit formats and -- except for x3, whose valid range ends there -- values beyond fp16's range."""
    x = rnd((n,), seed) * torch.pow(2.0, torch.randint(-20, 14, (n,), generator=torch.Generator().manual_seed(seed + 1)).double())
    special = [0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, -65504.0, 65519.0, 2.0 ** -25, 6.0e-8]
    if fmt != 3:
        special += [65520.0, -65520.0, 7.0e4, -1.0e6, 3.0e38, float("inf"), float("-inf")]
    k = min(n, len(special))
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed + 2))[:k]
    x[idx] = torch.tensor(special[-k:] if n < len(special) else special, dtype=torch.float64)
    return {"in": f32(x)}


def expect_cvt(x, fmt):
    """The expected 16-bit words.  fmt 1 is csrc/half16.h's f2h<true>: "round to nearest even; fp16 saturates at +-65504 instead of producing inf" -- so everything
    beyond +-65504, the infinities included, gives +-65504; fmt 5 (f2h_ieee) is "WITHOUT the clamp: overflow gives +-inf"."""
    x = x.float()
    if fmt == 0:
        return x.to(torch.bfloat16)
    if fmt == 1:
        return x.clamp(-F16_MAX, F16_MAX).to(torch.float16)
    return x.to(torch.float16)


def call_cvt(n, fmt, inp):
    return Call("cvt", [n], flags_of(0, fmt), ins=[inp["in"].float()], outs=[("out", (n,), fmt)], finite=False)


CONV_W_SHAPES = {"1x1": (1, 1), "3x5": (3, 5), "2x16": (2, 16), "64x912": (64, 912)}       # 64 * 912 * 9 = 525,312 > 2048 * 256
CONV_W_RUNS = [(s, m, sc) for s in ("1x1", "3x5", "64x912") for m in ("bf16", "f16", "f32") for sc in (False, True)] + \
              [(s, "x3", sc) for s in ("2x16", "64x912") for sc in (False, True)]
CONV_W_MODE = {"bf16": (0, 0), "f16": (0, 1), "f32": (1, 0), "x3": (0, 3)}                  # out_is_f32, hf


def build_conv_w(shape, seed=55):
    Cout, Cin = CONV_W_SHAPES[shape]
    return {"w": rnd((Cout, Cin, 3, 3), seed), "scale": f32(0.5 + rnd((Cout,), seed + 1).abs())}


def ref_conv_w(inp, scaled):
    """[Cout][3][3][Cin] (ref, bound): bound 0 without scale (a selection), u |w s| with."""
    v = inp["w"].permute(0, 2, 3, 1)
    if not scaled:
        return v.contiguous(), torch.zeros_like(v)
    v = v * inp["scale"][:, None, None, None]
    return v, U * v.abs()


def call_conv_w(shape, mode, scaled, inp):
    Cout, Cin = CONV_W_SHAPES[shape]
    is_f32, hf = CONV_W_MODE[mode]
    return Call("conv_w", [Cout, Cin], flags_of(is_f32, hf), ins=[inp["w"].float(), inp["scale"].float() if scaled else None],
                outs=[("out", (Cout, 3, 3, Cin), 2 if is_f32 else hf)])


SMALL_SIZES = [1, 100, 300]


def build_bn_fold(C, seed=61):
    var = rnd((C,), seed).abs() + 1e-4
    var[0] = 1e-4
    return {"g": f32(1.0 + 0.3 * rnd((C,), seed + 1)), "b": f32(0.2 * rnd((C,), seed + 2)), "mean": rnd((C,), seed + 3), "var": f32(var)}


def ref_bn_fold(inp, eps_outside=False):
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    s = inp["g"] / ((inp["var"].sqrt() + eps) if eps_outside else (inp["var"] + eps).sqrt())
    e_s = gamma(8) * s.abs()
    return {"scale": (s, e_s), "shift": (inp["b"] - inp["mean"] * s, inp["mean"].abs() * e_s + gamma(3) * (inp["b"].abs() + (inp["mean"] * s).abs()))}


def call_bn_fold(C, inp):
    return Call("bn_fold", [C], ins=[inp[k].float() for k in ("g", "b", "mean", "var")], outs=[("scale", (C,), 2), ("shift", (C,), 2)])


def build_qkv_bias(C, seed=65):
    return {"q": rnd((C,), seed), "v": rnd((C,), seed + 1)}


def call_qkv_bias(C, inp):
    return Call("qkv_bias", [C], ins=[inp["q"].float(), inp["v"].float()], outs=[("out", (3 * C,), 2)])


LOGIT_HEADS = [1, 3, 24, 64, 100]        # 100 > the 64 threads launch_logit_scale used to launch
LN100_F32 = float(torch.tensor(4.605170185988092, dtype=torch.float32))


def build_logit_scale(H, seed=67):
    """On both sides of ln 100, the neighbours of the clamp included."""
    ls = rnd((H,), seed) * 2 + 3.5
    for i, v in enumerate([4.6051, 4.6052, 4.605170185988092, 10.0, 0.0, -3.0][:H]):
        ls[(i * 7) % H] = v
    return {"ls": f32(ls)}


def ref_logit_scale(inp):
    v = inp["ls"].clamp(max=LN100_F32).exp()
    return v, 4 * U * v


def call_logit_scale(H, inp):
    return Call("logit_scale", [H], ins=[inp["ls"].float()], outs=[("out", (H,), 2)])


CPB_CASES = [(8, 0, 3), (12, 0, 6), (16, 8, 24), (24, 12, 32), (8, 8, 6), (12, 16, 3)]      # ws, pws, H; H = 32: 70 KB of LDS
CPB_TOO_MANY_HEADS = 78                                                                    # (1536 + 512 H) floats > 160 KB


def build_cpb(case, seed=71):
    ws, pws, H = case
    return {"w0": rnd((512, 2), seed, 0.7), "b0": rnd((512,), seed + 1, 0.5), "w2": rnd((H, 512), seed + 2, 1 / 16.0)}


def ref_cpb(case, inp, denom_ws=False):
    """table [(2 ws - 1)^2][H] (ref, bound).  denom_ws: the planted fault -- ws - 1 where the pretrained window's pws - 1 is due."""
    ws, pws, H = case
    T = 2 * ws - 1
    denom = float((ws if (pws <= 0 or denom_ws) else pws) - 1)
    d = torch.arange(T, dtype=torch.float64) - (ws - 1)
    c = d / denom * 8
    coord = c.sign() * torch.log2(c.abs() + 1) / 3
    e_c = gamma(8) * coord.abs()
    cy, cx = coord[:, None].expand(T, T).reshape(-1, 1), coord[None, :].expand(T, T).reshape(-1, 1)
    ey, ex = e_c[:, None].expand(T, T).reshape(-1, 1), e_c[None, :].expand(T, T).reshape(-1, 1)
    wa, wb, b0 = inp["w0"][:, 0][None], inp["w0"][:, 1][None], inp["b0"][None]
    pre = wa * cy + wb * cx + b0
    e_h = wa.abs() * ey + wb.abs() * ex + gamma(3) * ((wa * cy).abs() + (wb * cx).abs() + b0.abs())
    h = pre.clamp(min=0)
    w2 = inp["w2"].t()
    s = h @ w2
    e_s = e_h @ w2.abs() + gamma(512 + 2) * ((h + e_h) @ w2.abs())
    tab = 16 * torch.sigmoid(s)
    return tab, 4 * e_s + 8 * U * tab


def call_cpb(case, inp):
    ws, pws, H = case
    return Call("cpb_table", [ws, pws, H], ins=[inp["w0"].float(), inp["b0"].float(), inp["w2"].float()], outs=[("table", ((2 * ws - 1) ** 2, H), 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# hybrid.hip: WS_CONV_W, STEM_IM2COL, GN_RELU_MAXPOOL, VIT_TOKENS_LN, LN_ROWS, POS_EMBED_RESIZE
# ---------------------------------------------------------------------------------------------------------------------------------
WS_CASES = {"stem": (8, 3, 7, 160), "1x1": (5, 64, 1, 64), "3x3_288": (4, 32, 3, 288), "3x3_144": (3, 16, 3, 160)}     # Cout, Cin, k, Kpad; fan-in 147, 64, 288, 144
WS_EPS = float(torch.tensor(1e-8, dtype=torch.float32))


def build_ws(case, seed=81):
    Cout, Cin, k, _ = WS_CASES[case]
    w = rnd((Cout, Cin, k, k), seed, 0.1) + 0.05 * torch.arange(Cout, dtype=torch.float64)[:, None, None, None]
    w[-1] = 0.5                                 # an all-equal filter: variance 0, the result is governed by eps
    return {"w": f32(w)}


def ref_ws(case, inp, eps=WS_EPS, unbiased=False):
    """[Cout][Kpad] tap-major (ref, bound); columns beyond the fan-in: 0 with bound 0."""
    Cout, Cin, k, Kpad = WS_CASES[case]
    fan = Cin * k * k
    w = inp["w"].reshape(Cout, fan)
    mean = w.mean(1, keepdim=True)
    var = ((w - mean) ** 2).sum(1, keepdim=True) / (fan - 1 if unbiased else fan)
    rstd = 1 / (var + eps).sqrt()
    r = 2.0 ** -50 * (w ** 2).mean(1, keepdim=True) / (2 * (var + eps))
    v = (w - mean) * rstd
    e = rstd * U * (mean.abs() + (w - mean).abs()) + v.abs() * (2 * U + r)
    tap = lambda t: t.reshape(Cout, Cin, k * k).permute(0, 2, 1).reshape(Cout, fan)
    return F.pad(tap(v), (0, Kpad - fan)), F.pad(tap(e), (0, Kpad - fan))


def call_ws(case, mode, inp):
    Cout, Cin, k, Kpad = WS_CASES[case]
    return Call("ws_conv_w", [Cout, Cin, k, Kpad], flags_of(0, mode), f=(WS_EPS, 0.0, 0.0), ins=[inp["w"].float()], outs=[("out", (Cout, Kpad), mode)])


IM2COL_SIZES = [16, 34]


def build_im2col(S, seed=85):
    return {"x": f32(rnd((2, 3, S, S), seed) + 3.0)}          # no zeros inside the image: a padding zero is told from a pixel


def ref_im2col(inp, pad_left=False):
    """A [B (S/2)^2][160], k = (ky 7 + kx) 3 + c, TF 'SAME' (2 in front, 3 behind); pad_left: the planted fault (3 in front)."""
    x = inp["x"]
    B, _, S, _ = x.shape
    xp = F.pad(x, (3, 2, 3, 2) if pad_left else (2, 3, 2, 3))
    cols = xp.unfold(2, 7, 2).unfold(3, 7, 2)                      # [B][3][Ho][Ho][ky][kx]
    A = cols.permute(0, 2, 3, 4, 5, 1).reshape(B * (S // 2) ** 2, 147)
    return F.pad(A, (0, 13))


def call_im2col(S, mode, inp):
    return Call("stem_im2col", [2, S], flags_of(0, mode), ins=[inp["x"].float()], outs=[("A", (2 * (S // 2) ** 2, 160), mode)])


POOL_SHAPES = [(2, 2, 16, 2), (2, 6, 32, 8), (2, 16, 16, 4), (1, 6, 64, 2)]       # B, Hi, C, cpg


def build_pool(shape, seed=91):
    """The post-GroupNorm values are chosen first -- per (sample, channel) a permutation of a 4e-3 lattice that misses zero by 2e-3, about 60 % of it negative, and one quadrant of
    channel 1 all negative (a window that is all <= 0) -- and raw is solved from them; pool_gaps checks the promise on what the f32 inputs really give."""
    B, Hi, C, cpg = shape
    G = C // cpg
    gen = torch.Generator().manual_seed(seed)
    n = Hi * Hi
    y = torch.stack([torch.stack([(torch.randperm(n, generator=gen).double() - (6 * n // 10) - 0.5) * 4e-3 * (1 + (c % 3)) for c in range(C)], -1) for _ in range(B)]).reshape(B, Hi, Hi, C)
    if Hi >= 4:
        y[:, : Hi // 2 + 1, : Hi // 2 + 1, 1] = -y[:, : Hi // 2 + 1, : Hi // 2 + 1, 1].abs() - 1e-3
    stats = torch.stack([rnd((B, G), seed + 1, 0.5), 0.5 + rnd((B, G), seed + 2).abs()], -1)
    gamma_, beta = 1.0 + 0.3 * rnd((C,), seed + 3), 0.2 * rnd((C,), seed + 4)
    gamma_ = gamma_.sign() * gamma_.abs().clamp(min=0.3)
    stats, gamma_, beta = f32(stats), f32(gamma_), f32(beta)
    mean, rstd = (stats[..., k].repeat_interleave(cpg, 1)[:, None, None, :] for k in (0, 1))
    raw = f32((y - beta) / (gamma_ * rstd) + mean)
    return {"raw": raw, "stats": stats, "gamma": gamma_, "beta": beta}


def pool_taps(inp, cpg):
    """relu(GN(raw)) per pixel and its per-tap bound."""
    mean, rstd = (inp["stats"][..., k].repeat_interleave(cpg, 1)[:, None, None, :] for k in (0, 1))
    d = (inp["raw"] - mean) * rstd * inp["gamma"]
    y = d + inp["beta"]
    return y.clamp(min=0), gamma(4) * (d.abs() + inp["beta"].abs()) + torch.zeros_like(y)


def pool_windows(t, pad_left=False, fill=0.0):
    """[B][Hi][Hi][C] -> [B][Ho][Ho][C][9]: 3 x 3 / 2 windows, padded behind the image (TF 'SAME' at an even side); pad_left: the planted fault."""
    tp = F.pad(t.permute(0, 3, 1, 2), (1, 0, 1, 0) if pad_left else (0, 1, 0, 1), value=fill)
    win = tp.unfold(2, 3, 2).unfold(3, 3, 2)                          # [B][C][Ho][Ho][3][3]
    return win.permute(0, 2, 3, 1, 4, 5).reshape(*win.shape[:1], win.shape[2], win.shape[3], win.shape[1], 9)


def ref_pool(shape, inp, pad_left=False):
    y, e = pool_taps(inp, shape[3])
    return pool_windows(y, pad_left).max(-1).values, pool_windows(e, pad_left).max(-1).values


def pool_gaps(shape, inp):
    """Smallest distance between the best and the second-best value over the windows whose best is positive, and the number of all-zero windows."""
    y, _ = pool_taps(inp, shape[3])
    top2 = pool_windows(y, fill=-1.0).topk(2, dim=-1).values
    gap = (top2[..., 0] - top2[..., 1])[top2[..., 0] > 0]
    return float(gap.min()) if gap.numel() else float("inf"), int((top2[..., 0] == 0).sum())


def call_pool(shape, mode, inp):
    B, Hi, C, cpg = shape
    return Call("gn_relu_maxpool", [B, Hi, C, cpg], flags_of(0, mode), ins=[inp[k].float() for k in ("raw", "stats", "gamma", "beta")],
                outs=[("out", (B, Hi // 2, Hi // 2, C), mode)])


VIT_EPS = float(torch.tensor(1e-6, dtype=torch.float32))
VIT_CASES = [(2, 2), (3, 3)]                 # B, g: ntok = 1 + g^2 = 5, 10; rows 10, 30 (no multiple of 4)
LN_ROWS_CASES = {"1": (1, False), "7": (7, False), "7_shifted": (7, True)}


def build_vit(case, seed=101):
    B, g = case
    ntok = 1 + g * g
    y = rnd((B * (ntok - 1), 768), seed) + 0.3 * torch.arange(B * (ntok - 1), dtype=torch.float64)[:, None] % 2
    pos = rnd((ntok, 768), seed + 1, 0.5) + 0.01 * torch.arange(ntok, dtype=torch.float64)[:, None]
    pos[2] += 40.0                                        # token 2 of every sample: a shifted row
    pos[1] *= 0.01                                        # token 1 of sample 0: a spread of 0.01, where eps matters
    y[0] *= 0.01
    _, gg, be = ln_inputs(1, 768, seed + 3)
    return {"y": f32(y), "cls": rnd((768,), seed + 2), "pos": f32(pos), "g": gg, "be": be}


def vit_tokens(inp, B, ntok, off_by_one=False):
    """The f32 token sums [B ntok][768] (one rounding each: torch's f32 addition gives the kernel's bits).  off_by_one: the planted fault (pos row t - 1 for t >= 1)."""
    y, cls, pos = inp["y"].float().reshape(B, ntok - 1, 768), inp["cls"].float(), inp["pos"].float()
    p = torch.cat([pos[:1], pos[:-1]]) if off_by_one else pos
    return (torch.cat([cls.expand(B, 1, 768), y], 1) + p[None]).reshape(B * ntok, 768)


def call_vit(case, mode, inp):
    B, g = case
    ntok = 1 + g * g
    return Call("vit_tokens_ln", [B, ntok, 768], flags_of(0, mode), f=(VIT_EPS, 0.0, 0.0), ins=[inp[k].float() for k in ("y", "cls", "pos", "g", "be")],
                outs=[("xf", (B * ntok, 768), 2), ("xb", (B * ntok, 768), mode)])


def build_ln_rows(case, seed=105):
    rows, shifted = LN_ROWS_CASES[case]
    y, g, b = ln_inputs(rows, 768, seed, shifted)
    return {"xf": y, "g": g, "be": b}


def call_ln_rows(case, mode, inp):
    rows = LN_ROWS_CASES[case][0]
    return Call("ln_rows", [rows, 768], flags_of(0, mode), f=(VIT_EPS, 0.0, 0.0), ins=[inp["g"].float(), inp["be"].float()],
                outs=[("xf", (rows, 768), 2), ("xb", (rows, 768), mode)], preset={"xf": inp["xf"].float()})


POS_CASES = [(4, 4, 8), (24, 16, 16), (24, 30, 16), (4, 5, 8)]       # g0, g, C


def build_pos(case, seed=111):
    g0, g, C = case
    return {"pos": f32(rnd((1 + g0 * g0, C), seed) + 0.1 * torch.arange(1 + g0 * g0, dtype=torch.float64)[:, None])}


def ref_pos(case, inp, align_corners=False):
    g0, g, C = case
    src = inp["pos"][1:].reshape(1, g0, g0, C)
    z = torch.zeros(g, g, dtype=torch.long)
    Y, X = torch.arange(g)[:, None].expand(g, g), torch.arange(g)[None, :].expand(g, g)
    v, e = FR.bilinear_sample(src, z, Y, X, g, g, align_corners)
    return torch.cat([inp["pos"][:1], v.reshape(g * g, C)]), torch.cat([torch.zeros(1, C, dtype=torch.float64), e.reshape(g * g, C)])


def call_pos(case, inp):
    g0, g, C = case
    return Call("pos_embed_resize", [g0, g, C], ins=[inp["pos"].float()], outs=[("out", (1 + g * g, C), 2)])
