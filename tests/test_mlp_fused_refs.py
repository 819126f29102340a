"""CPU: tests/mlp_fused_refs.py checked against an f32 emulation of mlp_ln_kernel's arithmetic (csrc/mlp_fused.hip), and the emulation with one planted defect
at a time against the same reference -- the bound must hold the honest emulation on every case of the table in both families, and must refuse every defect on
the case named for it in DEFECTS.

The emulation: fc1 and fc2 as MFMA k-steps (the 32 products of a step summed exactly, rounded once, added to the f32 accumulator), the bias added in f32,
gelu.h's gelu_fast restated operation by operation in f32 (fmaf as a float64 product-sum rounded to f32; __expf as the float64 exp of the f32 argument rounded to
f32 -- the one function whose allowance in gelu_fast_bound is taken from its documented precision, not measured here), the hidden tile rounded with round16
(fp16 saturating), the epilogue in the kernel's order: v = acc + b2, mean = sum / C, the two-pass variance, rsqrt(sq / C + 1e-5f), xres + ((v - mean) rstd g + beta),
and the copies as RN16 of that f32 value in the plain, merged and zero-halo layouts into buffers of 0xFF bytes.
"""
import math

import pytest
import torch

from tests import mlp_fused_refs as R
from tests.fused_refs import round16
from tests.fwd_aux_refs import merge_layout, merge_layout_swapped

F = torch.float32


def fma(a, b, c):
    return (a.double() * b.double() + c.double()).to(F)


def gelu_fast_f32(x):
    """csrc/gelu.h gelu_fast on an f32 tensor."""
    c = lambda v: torch.tensor(v, dtype=F)
    z = x.abs() * c(0.70710678118654752440)
    t = c(1.0) / fma(c(0.3275911), z, c(1.0))
    p = fma(c(1.061405429), t, c(-1.453152027))
    p = fma(p, t, c(1.421413741))
    p = fma(p, t, c(-0.284496736))
    p = fma(p, t, c(0.254829592))
    E = torch.exp((-z * z).double()).to(F)
    e = c(1.0) - p * t * E
    return c(0.5) * x * (c(1.0) + torch.copysign(e, x))


def gelu_tanh_f32(x):
    return (0.5 * x.double() * (1 + torch.tanh(math.sqrt(2 / math.pi) * (x.double() + 0.044715 * x.double() ** 3)))).to(F)


def mfma_gemm(a, w):
    """[M][K] x [N][K]^T in k-steps of 32: exact products, one rounding of the step's sum, one of the accumulation (within the model's 6 roundings per step)."""
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=F)
    for k in range(0, a.shape[1], 32):
        acc = acc + (a[:, k:k + 32].double() @ w[:, k:k + 32].double().t()).to(F)
    return acc


def to16(v, fmt, saturate=True):
    v = v.float()
    if fmt == "f16" and saturate:
        v = v.clamp(-R.F16_MAX, R.F16_MAX)
    return v.to(R.DT[fmt])


def emulate(case, inp, defect=None):
    fmt, M, C = case.fmt, case.rows, case.C
    B, H, W = case.bhw
    x, w1, w2 = inp["x"].to(F), inp["w1"].to(F), inp["w2"].to(F)
    b1, b2, g, beta, xres = (inp[k].to(F) for k in ("b1", "b2", "g", "beta", "xres"))
    if defect == "b1_chunk0":
        b1 = b1[:64].repeat(4 * C // 64)
    pre = mfma_gemm(x, w1) + b1
    h = gelu_tanh_f32(pre) if defect == "tanh_gelu" else gelu_fast_f32(pre)
    h16 = h if defect == "hidden_f32" else to16(h, fmt, saturate=defect != "f16_no_saturate").to(F)
    if defect == "drop_last_chunk":
        h16 = h16.clone()
        h16[:, -64:] = 0
    v = mfma_gemm(h16, w2)
    if defect != "no_b2":
        v = v + b2
    mean = v.sum(-1, keepdim=True) / torch.tensor(float(C), dtype=F)
    d = v - mean
    sq = (d * d).sum(-1, keepdim=True)
    n = float(C - 1) if defect == "unbiased_var" else float(C)
    rstd = torch.rsqrt(sq / torch.tensor(n, dtype=F) + torch.tensor(1e-6 if defect == "eps_1e-6" else 1e-5, dtype=F))
    t = d * rstd * g + beta
    res = xres
    if defect == "no_residual":
        res = torch.zeros_like(xres)
    if defect == "ragged_residual" and M % 64:
        res = xres.clone()
        res[M - M % 64:] = xres[M - 1]
    o = res + t
    o16 = to16(o, fmt)
    got = {"xf": o, "xop": None, "halo": None}
    if case.merge:
        got["xop"] = R.merged(o16, B, H, W, swapped=defect == "merge_swapped")
    elif case.out in ("copy", "inplace"):
        got["xop"] = o16
    if case.halo:
        halo = torch.full((B, H + 2, W + 2, C), -1, dtype=torch.int16).view(R.DT[fmt])
        k = 0 if defect == "halo_no_ring_offset" else 1
        halo[:, k:k + H, k:k + W] = o16.reshape(B, H, W, C)
        got["halo"] = halo
    return got


_cache = {}


def prepared(name, family):
    """(case, inputs, reference) of a case, computed once and left unchanged."""
    if (name, family) not in _cache:
        case = R.find(name)
        inp = R.build(case, family)
        _cache[name, family] = (case, inp, R.case_reference(case, family, inp))
    return _cache[name, family]


# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_table_covers_every_axis_with_both_formats():
    cases = list(R.CASES.values())
    both = lambda sel: {c.fmt for c in cases if sel(c)} == {"bf16", "f16"}
    for C in (96, 128, 192, 256):
        assert both(lambda c: c.C == C), C
    for M in R.FLAT_M:
        assert both(lambda c: not c.grid and c.M == M), M
    for gname in R.GRIDS:
        assert both(lambda c: c.grid == gname), gname
        assert {"merge", "merge_halo"} <= {c.out for c in cases if c.grid == gname}, gname
    for out in R.OUTS:
        assert both(lambda c: c.out == out), out
        for C in (96, 128, 192):
            assert any(c.C == C and c.out == out for c in cases), (C, out)
    assert all(c.rows <= 130 for c in cases + list(R.SPECIAL_CASES.values()))
    assert all((c.halo or c.merge) <= bool(c.grid) for c in cases)
    assert {c.special for c in R.SPECIAL_CASES.values()} == set(R.SPECIALS)
    B, H, W = R.GRIDS["g2"]
    assert H != W and (H * W) % 64 and 64 % (H * W) and (B * H * W) % 64, "g2: images straddle the 64-token tile, the last tile is ragged"


def test_merged_is_merge_layout_and_the_kernel_comment_agrees():
    x = torch.arange(2 * 6 * 6 * 3, dtype=torch.float64).reshape(72, 3)
    assert torch.equal(R._merged_rect(x, 2, 6, 6), merge_layout(x, 2, 6)) and torch.equal(R._merged_rect(x, 2, 6, 6, True), merge_layout_swapped(x, 2, 6))
    # include/soccdpt_hip.h: token (b, y, x) in row (b, y / 2, x / 2) at channel block (y & 1) + 2 (x & 1)
    B, H, W, C = 3, 6, 4, 2
    t = torch.arange(B * H * W * C, dtype=torch.float64).reshape(B * H * W, C)
    out = R.merged(t, B, H, W).reshape(B, H // 2, W // 2, 4, C)
    for b, y, xx in ((0, 0, 0), (1, 3, 2), (2, 5, 3), (2, 4, 1)):
        assert torch.equal(out[b, y // 2, xx // 2, (y & 1) + 2 * (xx & 1)], t[(b * H + y) * W + xx])


def test_gelu_fast_bound_and_lipschitz_on_a_dense_grid():
    """|gelu_fast (f32 emulation, exp in float64) - gelu_erf (float64)| <= gelu_fast_bound on 4,000,001 points of [-10, 10], and L bounds the slope of GELU."""
    x = torch.linspace(-10, 10, 4_000_001, dtype=torch.float64).to(F)
    x = torch.cat([x, torch.tensor([0.0, -0.0, 1e-30, -1e-30, 2.0 ** -126, 1e5, -1e5, 7e4], dtype=F)])
    x64 = x.double()
    err = (gelu_fast_f32(x).double() - R.gelu64(x64)).abs()
    bound = R.gelu_fast_bound(x64)
    assert bool((err <= bound).all()), float((err / bound.clamp(min=1e-300)).max())
    inside = x64.abs() <= 10
    print(f"gelu_fast: worst error / bound {float((err / bound.clamp(min=1e-300))[inside].max()):.3f}; largest bound on [-10, 10] {float(bound[inside].max()):.2e}, at 0.5 {float(R.gelu_fast_bound(torch.tensor(0.5, dtype=torch.float64))):.2e}")
    assert float((bound / x64.abs().clamp(min=1e-30))[inside & (x64 != 0)].max()) < 2e-6      # f32 level relative to |x|, not a loose allowance
    slope = (R.gelu64(x64[1:4_000_001]) - R.gelu64(x64[:4_000_000])) / (x64[1:4_000_001] - x64[:4_000_000])
    assert 1.128 < float(slope.max()) < R.GELU_LIPSCHITZ and float(slope.min()) > -0.13


@pytest.mark.parametrize("name", [n for n, c in R.CASES.items() if c.rows >= 63])
def test_dyadic_fc1_is_exact_and_covers_the_range(name):
    case, inp, ref = prepared(name, "dyadic")
    pre = inp["x"] @ inp["w1"].t() + inp["b1"]
    assert torch.equal(pre * 128, (pre * 128).round()) and float(pre.abs().max()) < 512
    assert torch.equal((mfma_gemm(inp["x"].to(F), inp["w1"].to(F)) + inp["b1"].to(F)).double(), pre), "the f32 fc1 of the emulation is not exact"
    rev = torch.arange(case.C - 1, -1, -1)
    assert torch.equal((inp["x"].to(F)[:, rev] @ inp["w1"].to(F)[:, rev].t() + inp["b1"].to(F)).double(), pre), "nor in another order"
    assert float(ref["e_pre"].abs().max()) == 0
    cov = R.dyadic_coverage(inp)
    print(name, cov, f"undecided {ref['undecided']:.4f}")
    assert cov["empty_bins"] == 0 and min(cov["zero"], cov["small_pos"], cov["small_neg"], cov["tail"]) >= 1, cov


def test_the_saturating_case_saturates():
    for name, c in R.SPECIAL_CASES.items():
        if c.special != "saturate":
            continue
        _, inp, ref = prepared(name, "random")
        row = c.rows // 2 + 1
        assert float(ref["pre"][row, 21]) > 65504 and float(ref["pre"][:, :8].min()) > 65504 and float(ref["pre"][:, 8:16].max()) < -65504
        assert float(ref["h_mid"].max()) == 65504.0 and float(ref["h"].max()) > 1e5 and bool(torch.isfinite(ref["o"]).all()) and bool(torch.isfinite(ref["e_o"]).all())


ALL = [(n, f) for n in R.CASES for f in R.FAMILIES] + [(n, "random") for n in R.SPECIAL_CASES]


@pytest.mark.parametrize("name,family", ALL, ids=[f"{n}-{f}" for n, f in ALL])
def test_emulation_is_inside_the_bound(name, family):
    case, inp, ref = prepared(name, family)
    ratio = R.check_outputs(case, inp, ref, emulate(case, inp), f"{name} {family}")
    print(f"{name} {family}: worst error / bound {ratio:.3f}, undecided {ref['undecided']:.4f}, median bound {float(ref['e_o'].median()):.2e}")
    assert ratio <= 1


# defect -> the (bf16, f16) cases that refuse it, in the dyadic family unless the name says otherwise
DEFECTS = {
    "b1_chunk0": ("c96_bf16_m65_inplace", "c96_f16_m63_copy"),                   # chunk 0's b1 used for every chunk
    "drop_last_chunk": ("c128_bf16_m130_copy", "c128_f16_m64_f32"),              # last hidden chunk dropped
    "no_b2": ("c192_bf16_m65_f32", "c192_f16_m130_inplace"),                     # b2 omitted
    "tanh_gelu": ("c96_bf16_m65_inplace", "c96_f16_m63_copy"),                   # tanh-GELU
    "hidden_f32": ("c128_bf16_m130_copy", "c128_f16_m64_f32"),                   # hidden tile kept in f32 (the fused launch rounds it as the unfused chain stores it)
    "eps_1e-6": ("c96_bf16_m65_inplace", "c256_f16_m130_f32"),                   # eps = 1e-6
    "unbiased_var": ("c192_bf16_m65_f32", "c256_f16_m130_f32"),                  # variance / (C - 1)
    "no_residual": ("c256_bf16_m64_copy", "c96_f16_m63_copy"),                   # residual omitted
    "ragged_residual": ("c128_bf16_m130_copy", "c96_f16_g2_halo"),               # residual of row M - 1 for the whole ragged tile (rows 128-129; 64-71)
    "merge_swapped": ("c192_bf16_g2_merge", "c128_f16_g3_merge"),                # PatchMerging blocks (1,0) and (0,1) exchanged
    "halo_no_ring_offset": ("c128_bf16_g3_halo", "c96_f16_g2_halo"),             # halo written without the + 1 ring offset
    "f16_no_saturate": (None, "c128_f16_m65_copy_saturate"),                     # bf16 has fp32's range: nothing saturates there, the defect exists in f16 only
}
DEFECT_RUNS = [(d, n) for d, pair in DEFECTS.items() for n in pair if n]


@pytest.mark.parametrize("defect,name", DEFECT_RUNS, ids=[f"{d}-{n}" for d, n in DEFECT_RUNS])
def test_planted_defect_is_refused(defect, name):
    family = "random" if R.find(name).special else "dyadic"
    case, inp, ref = prepared(name, family)
    R.check_outputs(case, inp, ref, emulate(case, inp), name)          # the honest emulation passes this very case
    with pytest.raises(AssertionError) as e:
        R.check_outputs(case, inp, ref, emulate(case, inp, defect), f"{name} with {defect}")
    print(str(e.value)[:300])


def test_every_listed_defect_has_a_case():
    assert set(DEFECTS) == {"b1_chunk0", "drop_last_chunk", "no_b2", "tanh_gelu", "hidden_f32", "eps_1e-6", "unbiased_var", "no_residual", "ragged_residual",
                            "merge_swapped", "halo_no_ring_offset", "f16_no_saturate"}
    assert all(any(pair) for pair in DEFECTS.values())
    for d, (b, f) in DEFECTS.items():
        assert (b is None or R.find(b).fmt == "bf16") and (f is None or R.find(f).fmt == "f16"), d
