"""GPU: the reader side of the hybrid's GroupNorm (csrc/hybrid.hip gn_apply_kernel / gn_finish_kernel, round 5) at kernel level.

timm's ResNetV2 puts GroupNormAct(32 groups) after every StdConv2dSame of the stem and the stages (the backbone of dpt_hybrid_384,
/root/reference/SOccDPT/model/backbones/vit.py:147-201; oracle/soccdpt_ref.py rn_bottleneck).  Since round 5 the producing convolution only leaves per-tile
partial sums; the GroupNorm-apply kernel adds them up itself -- per thread for short tile lists, per workgroup for mid ones, by a separate launch for long ones.
These tests feed the kernel partials computed here in float64 from a random raw tensor (tiles of 64 rows, as a 64-row convolution tile would leave them) and
compare every output with torch.nn.functional.group_norm on the same raw tensor: all three finish modes, both shortcut kinds, the two-group float4 case
(C = 64), every output format, and the statistics the kernel writes back.

Below those three tests, every launch of the case table of tests/gn_refs.py runs alone against the float64 reference computed from the f32 partials as handed
and the a-priori element-wise bound derived there (tests/test_gn_refs.py tests that module against itself on the CPU).  Per test id: the bound on every output
element and every stored statistic; 0xFF still in the halo ring, in the 4 KB behind every buffer and in statistics the launch only reads or has no shortcut
for; the inputs unchanged; a second launch bitwise equal; mode 0 reading the statistics the first launch wrote gives the same bits in every output.  Data sets:
(a) neighbouring groups and samples >= 10x apart in mean and >= 4x in spread, (b) mean over spread 30 and 700, (c) a constant group and hand-made partials with
q / n one f32 ulp below mean^2, (d) gamma with zeros and negative entries, raw values at the f32 mean and one ulp either side where beta = -0.  Every refusal raises
the launcher's message and writes nothing.  `pytest -s` prints each id's worst error / bound.

Measured on MI355X (worst error / bound over the table; every bound is the derived one, no constant fitted):

    statistics mode              out_f32   stored {mean, rstd}
    1  per-thread sums            0.781        0.886
    2  workgroup sums             0.561        0.831
    0  after a finish launch      0.484        0.785
    0  finished statistics read   0.566          -
    gn_finish alone (32 ids)        -          0.996

    operand output (out_op / out_halo)     beside an f32 output       alone
    bf16, fp16                             RN16 of it, exactly        inside [RN16(ref - bound), RN16(ref + bound)] (1.0: on its end)
    f32                                    the same bits              0.667
    x3                                     hi = RN16, decode 0.9997*   0.741 (hi inside the fp16 interval)
    (* of 2^-23 |v| + 2^-36 around the kernel's own f32 value)

The stored statistics come close to their bound by construction: its leading term is the f32 store, U |mean|, and half an ulp of a significand near 1 is
just that.  U = 4 and U = 2 of every format: 0.59 / 0.58 (out_f32), 0.74 (x3 alone), 0.57 (f32 alone)."""
import math
import re

import pytest
import torch
import torch.nn.functional as F

from tests import gn_refs as T

pytestmark = pytest.mark.gpu


def _partials(raw, B, hw, C, rows):
    """[B * hw / rows][32][2] = {sum, sum of squares} of each tile of `rows` pixel rows and each group, float32 as the convolution's epilogue leaves them."""
    cpg = C // 32
    t = raw.double().reshape(B, hw // rows, rows, 32, cpg)
    return torch.stack((t.sum((2, 4)), (t * t).sum((2, 4))), -1).reshape(B * (hw // rows), 32, 2).float()


def _gn(raw, B, side, C, gamma, beta):
    x = raw.reshape(B, side, side, C).permute(0, 3, 1, 2)
    return F.group_norm(x.double(), 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 3, 1).reshape(B * side * side, C)


# side, C, tile rows -> tiles per sample: 9 (per-thread walk), 36 (workgroup walk through LDS), 144 (separate finish launch; C = 64: a float4 spans two groups)
CASES = [(24, 256, 64), (24, 1024, 64), (48, 128, 64), (48, 512, 128), (96, 64, 64), (96, 256, 128)]


@pytest.mark.parametrize("shortcut", ["none", "identity", "projection"])
@pytest.mark.parametrize("side,C,rows", CASES)
def test_gn_apply_from_partials_matches_group_norm(gpu_device, side, C, rows, shortcut):
    from soccdpt_amd.lib import PREC_F16, PREC_F16X3, PREC_F32, op_gn_apply, x3_decode
    B, hw, cpg = 2, side * side, C // 32
    g = torch.Generator().manual_seed(side * 1000 + C)
    raw = torch.randn((B * hw, C), generator=g) * 2.0 + 0.7
    raw[:, : C // 2] += 3.0                                   # groups with a large mean: the variance is a difference of large numbers
    gamma, beta = torch.rand((C,), generator=g) + 0.5, torch.randn((C,), generator=g) * 0.3
    ref = _gn(raw, B, side, C, gamma, beta)
    dev = lambda t: t.to(gpu_device)
    kw = {}
    if shortcut == "identity":
        res = torch.randn((B * hw, C), generator=g)
        ref = ref + res.double()
        kw["res"] = dev(res)
    elif shortcut == "projection":
        raw2 = torch.randn((B * hw, C), generator=g) * 0.5 - 1.0
        gamma2, beta2 = torch.rand((C,), generator=g) + 0.5, torch.randn((C,), generator=g) * 0.3
        ref = ref + _gn(raw2, B, side, C, gamma2, beta2)
        kw.update(raw2=dev(raw2), stats2=torch.full((B, 32, 2), -7.0, device=gpu_device), part2=dev(_partials(raw2, B, hw, C, rows)), tps2=hw // rows,
                  gamma2=dev(gamma2), beta2=dev(beta2))
    ref = ref.clamp_min(0.0)
    stats = torch.full((B, 32, 2), -7.0, device=gpu_device)
    out_f32 = torch.empty((B * hw, C), device=gpu_device)
    out_op = torch.empty((B * hw, C), dtype=torch.float16, device=gpu_device)
    op_gn_apply(dev(raw), stats, dev(gamma), dev(beta), hw, side, cpg, part=dev(_partials(raw, B, hw, C, rows)), tps=hw // rows, out_f32=out_f32, out_op=out_op,
                out_format=PREC_F16, **kw)
    torch.cuda.synchronize()
    # the statistics the kernel (or its finish launch) leaves behind
    x = raw.double().reshape(B, hw, 32, cpg)
    mean, var = x.mean((1, 3)), x.var((1, 3), unbiased=False)
    torch.testing.assert_close(stats[..., 0].cpu().double(), mean, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(stats[..., 1].cpu().double(), 1.0 / torch.sqrt(var + 1e-5), rtol=1e-5, atol=1e-6)
    if shortcut == "projection":
        x2 = raw2.double().reshape(B, hw, 32, cpg)
        torch.testing.assert_close(kw["stats2"][..., 0].cpu().double(), x2.mean((1, 3)), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out_f32.cpu().double(), ref, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(out_op.cpu().double(), ref, rtol=2e-3, atol=2e-3)
    # the same launch reading FINISHED statistics (the training step's form) gives the same bits as the one that added the partials up
    out_b = torch.empty_like(out_f32)
    kw_b = {k: v for k, v in kw.items() if k not in ("part2", "tps2")}
    op_gn_apply(dev(raw), stats, dev(gamma), dev(beta), hw, side, cpg, out_f32=out_b, **kw_b)
    torch.cuda.synchronize()
    assert torch.equal(out_b, out_f32)
    # zero-halo image in the x3 format, f32 plain operand copy
    halo = torch.zeros((B * (side + 2) * (side + 2) * C * 2,), dtype=torch.float16, device=gpu_device)
    op32 = torch.empty((B * hw, C), device=gpu_device)
    op_gn_apply(dev(raw), stats, dev(gamma), dev(beta), hw, side, cpg, out_op=op32, out_format=PREC_F32, **kw_b)
    op_gn_apply(dev(raw), stats, dev(gamma), dev(beta), hw, side, cpg, out_halo=halo, out_format=PREC_F16X3, **kw_b)
    torch.cuda.synchronize()
    assert torch.equal(op32, out_f32)
    h = x3_decode(halo, (B, side + 2, side + 2, C)).cpu()
    torch.testing.assert_close(h[:, 1:-1, 1:-1].reshape(B * hw, C), out_f32.cpu().double(), rtol=3e-7, atol=1e-6)
    assert float(h[:, 0].abs().max()) == 0.0 and float(h[:, :, -1].abs().max()) == 0.0


def test_gn_finish_matches_float64(gpu_device):
    from soccdpt_amd.lib import op_gn_finish
    B, hw, C, rows = 3, 192 * 192, 64, 64                      # the stem: 576 tiles per sample
    g = torch.Generator().manual_seed(3)
    raw = torch.randn((B * hw, C), generator=g) * 1.5 + 40.0   # un-normalised pixel levels: mean >> spread
    part = _partials(raw, B, hw, C, rows).to(gpu_device)
    stats = torch.empty((B, 32, 2), device=gpu_device)
    op_gn_finish(part, stats, B, hw // rows, 32, hw, C // 32)
    torch.cuda.synchronize()
    x = raw.double().reshape(B, hw, 32, C // 32)
    torch.testing.assert_close(stats[..., 0].cpu().double(), x.mean((1, 3)), rtol=1e-6, atol=1e-6)
    # the partials are float32: what the sum of squares can resolve of a variance 700 times smaller than mean^2 is ~1e-4 relative
    torch.testing.assert_close(stats[..., 1].cpu().double(), 1.0 / torch.sqrt(x.var((1, 3), unbiased=False) + 1e-5), rtol=5e-4, atol=0)


def test_gn_apply_refuses_what_it_cannot_do(gpu_device):
    from soccdpt_amd.lib import op_gn_apply
    raw = torch.zeros((2 * 16, 96), device=gpu_device)        # C / 4 = 24 does not divide 256
    with pytest.raises(RuntimeError, match="gn_apply"):
        op_gn_apply(raw, torch.zeros((2, 32, 2), device=gpu_device), torch.ones((96,), device=gpu_device), torch.zeros((96,), device=gpu_device), 16, 4, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# every launch of the case table of tests/gn_refs.py against its float64 reference and a-priori bound
# ---------------------------------------------------------------------------------------------------------------------------------
SEEN, RAN = set(), set()


def _guarded(dev, dtype, shape, fill=None):
    """(whole buffer as bytes, view of `shape`): 0xFF everywhere -- the values, a halo ring, and GUARD bytes behind the tensor -- unless `fill` gives the values."""
    n = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((n + T.GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    view = whole[:n].view(dtype).reshape(shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def _guards_intact(bufs, c, what):
    for k, (whole, view) in bufs.items():
        assert bool((whole[-T.GUARD:] == 0xFF).all()), f"{c.name}: {what}: bytes behind {k} were written"


def _launch(c, dinp, dev, stats_from=None):
    """One launch of case c into fresh sentinel-filled buffers; stats_from: the buffers of an earlier launch whose written statistics this one reads (mode 0)."""
    from soccdpt_amd.lib import op_gn_apply
    bufs = {k: _guarded(dev, *T.buf_spec(c, k)[:2]) for k in c.outs}
    proj = c.shortcut == "projection"
    reads = stats_from is not None or not c.tps
    for k in ("stats", "stats2"):
        given = stats_from[k][1] if stats_from is not None else (dinp.get(k) if not c.tps else None)
        bufs[k] = _guarded(dev, torch.float32, (c.B, T.G, 2), fill=given if (k == "stats" or proj) and reads else None)
    before = {k: bufs[k][0].clone() for k in ("stats", "stats2")}
    kw = {}
    if proj:
        kw.update(raw2=dinp["raw2"], gamma2=dinp["gamma2"], beta2=dinp["beta2"])
    if c.shortcut == "identity":
        kw["res"] = dinp["res"]
    if not reads:
        kw.update(part=dinp["part"], tps=c.tps)
        if proj:
            kw.update(part2=dinp["part2"], tps2=c.tps2)
    if c.halo_fmt is not None:
        kw["halo_format"] = T.prec_code(c.halo_fmt)
    op_gn_apply(dinp["raw"], bufs["stats"][1], dinp["gamma"], dinp["beta"], c.HW, c.W, c.cpg, stats2=bufs["stats2"][1],
                out_f32=bufs["f32"][1] if "f32" in c.outs else None, out_op=bufs["op"][1] if "op" in c.outs else None,
                out_halo=bufs["halo"][1] if "halo" in c.outs else None, out_format=T.prec_code(c.fmt), relu=bool(c.relu), eps=T.EPS, **kw)
    torch.cuda.synchronize()
    for k in ("stats", "stats2"):        # statistics that are only read, and the ones of a shortcut that is not there, stay as they were
        if reads or (k == "stats2" and not proj):
            assert torch.equal(bufs[k][0], before[k]), f"{c.name}: {k} was written by a launch that only reads it"
    return bufs


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_gn_apply_case_within_float64_bound(gpu_device, c):
    inp = T.build(c.name)
    ref = T.reference(c, inp)
    flat = lambda k, t: t.reshape(c.B * c.HW, c.C) if k in ("raw", "raw2", "res") else t
    dinp = {k: flat(k, v).to(gpu_device) for k, v in inp.items() if v is not None and not k.startswith("sizes")}
    inputs_before = {k: v.clone() for k, v in dinp.items()}
    first = _launch(c, dinp, gpu_device)
    _guards_intact(first, c, "first launch")
    ratios = T.check_outputs(c, ref, {k: v[1] for k, v in first.items()})
    print(f"\n{c.name}: (OUT, U, mode) {c.triple}: worst error / bound {({k: round(v, 4) for k, v in ratios.items()})}")
    assert ratios and max(ratios.values()) <= 1.0
    again = _launch(c, dinp, gpu_device)
    for k in first:
        assert torch.equal(first[k][0], again[k][0]), f"{c.name}: {k} differs between two launches"
    if c.tps:                            # mode 0 reading the statistics the first launch wrote: the same bits in every output
        third = _launch(c, dinp, gpu_device, stats_from=first)
        for k in c.outs:
            assert torch.equal(first[k][0], third[k][0]), f"{c.name}: {k} differs when the written statistics are read back"
    for k, v in dinp.items():
        assert torch.equal(v, inputs_before[k]), f"{c.name}: input {k} was written"
    SEEN.add(c.triple)
    RAN.add(c.name)


@pytest.mark.parametrize("groups", T.FINISH_G)
@pytest.mark.parametrize("tps", T.FINISH_TPS)
def test_gn_finish_case_within_float64_bound(gpu_device, tps, groups):
    from soccdpt_amd.lib import op_gn_finish
    B = 2
    part, hw, cpg = T.build_finish(tps, groups, B)
    assert T.finish_gw(groups, tps)[1] is None
    ref = T.stats_ref(part, B, tps, hw * cpg)
    dpart = part.to(gpu_device)
    outs = []
    for _ in range(2):
        whole, stats = _guarded(gpu_device, torch.float32, (B, groups, 2))
        op_gn_finish(dpart, stats, B, tps, groups, hw, cpg, eps=T.EPS)
        torch.cuda.synchronize()
        outs.append((whole, stats))
    assert bool((outs[0][0][-T.GUARD:] == 0xFF).all()), "bytes behind stats were written"
    ratio = T.check_stats(outs[0][1], ref, f"gn_finish tps {tps} groups {groups}")
    print(f"\ngn_finish tps {tps} groups {groups} (gw {T.finish_gw(groups, tps)[0]}): worst error / bound {ratio:.3f}")
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(dpart.cpu(), part)


@pytest.mark.parametrize("groups,tps", [(g, 64) for g in T.FINISH_REFUSED] + [(32, 0)])
def test_gn_finish_refusals_launch_nothing(gpu_device, groups, tps):
    from soccdpt_amd.lib import op_gn_finish
    msg = T.finish_gw(groups, tps)[1]
    assert msg is not None and (tps == 0 or msg == T.FINISH_REFUSED[groups])
    part = torch.ones((2 * max(tps, 1), groups, 2), device=gpu_device)
    whole, stats = _guarded(gpu_device, torch.float32, (2, groups, 2))
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        op_gn_finish(part, stats, 2, tps, groups, 4 * 64, 2)
    torch.cuda.synchronize()
    assert bool((whole == 0xFF).all())


# name -> (B, H, W, C, cpg, what is wrong, the launcher's message)
REFUSALS = {
    "cpg_3": (2, 4, 4, 96, 3, {}, "gn_apply: bad geometry"),
    "both_shortcuts": (2, 4, 4, 64, 2, {"both": True}, "gn_apply: one shortcut kind at a time"),
    "c_2048": (2, 1, 2, 2048, 64, {}, "gn_apply: C / 4 must divide 256 and a sample must be whole workgroups"),
    "quarter_workgroup": (2, 2, 2, 64, 2, {}, "gn_apply: C / 4 must divide 256 and a sample must be whole workgroups"),
    "part_without_tps": (2, 4, 4, 64, 2, {"part_only": True}, "gn_apply: bad deferred-statistics arguments"),
    "part2_missing": (2, 4, 4, 64, 2, {"tps": 4, "tps2": 4, "no_part2": True}, "gn_apply: bad deferred-statistics arguments"),
    "projection_without_gamma2": (2, 4, 4, 64, 2, {"no_affine2": True}, "soccdpt_op_gn_apply: the projection shortcut needs stats2, gamma2 and beta2"),
    "hw_is_no_rows_of_w": (2, 4, 4, 64, 2, {"w": 5}, "soccdpt_op_gn_apply: bad arguments"),
    "out_format_mixed": (2, 4, 4, 64, 2, {"out_format": 4}, "soccdpt_op_gn_apply: out_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3"),
    "halo_format_x2w": (2, 4, 4, 64, 2, {"halo_format": 5}, "soccdpt_op_gn_apply_halo: halo_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3"),
}


@pytest.mark.parametrize("name", REFUSALS)
def test_gn_apply_refusals_launch_nothing(gpu_device, name):
    from soccdpt_amd.lib import PREC_F32, op_gn_apply
    B, H, W, C, cpg, wrong, msg = REFUSALS[name]
    HW, groups = H * W, C // cpg
    tps, tps2, both = wrong.get("tps", 0), wrong.get("tps2", 0), wrong.get("both", False)
    proj = both or tps2 > 0 or wrong.get("no_affine2", False)
    if "out_format" not in wrong and "halo_format" not in wrong:   # the launcher's own refusals follow from the restated rules
        restated = T.apply_refusal(B, HW, wrong.get("w", W), C, cpg, tps, tps2, proj, both, part=bool(tps) or wrong.get("part_only", False),
                                   part2=not wrong.get("no_part2", False), affine2=not wrong.get("no_affine2", False))
        assert restated == msg, (restated, msg)
    dev = gpu_device
    z = lambda *s: torch.zeros(s, device=dev)
    bufs = {"f32": _guarded(dev, torch.float32, (B * HW, C)), "op": _guarded(dev, torch.float32, (B * HW, C)), "halo": _guarded(dev, torch.float32, (B, H + 2, W + 2, C)),
            "stats": _guarded(dev, torch.float32, (B, groups, 2)), "stats2": _guarded(dev, torch.float32, (B, groups, 2))}
    kw = {}
    if proj:
        kw.update(raw2=z(B * HW, C), **({} if wrong.get("no_affine2") else {"gamma2": z(C), "beta2": z(C)}))
    if both:
        kw["res"] = z(B * HW, C)
    if tps or wrong.get("part_only"):
        kw.update(part=z(B * max(tps, 1), groups, 2), tps=tps)
    if tps2 and not wrong.get("no_part2"):
        kw.update(part2=z(B * tps2, groups, 2))
    if tps2:
        kw["tps2"] = tps2
    if "halo_format" in wrong:
        kw["halo_format"] = wrong["halo_format"]
    with pytest.raises(RuntimeError, match=re.escape(msg)):
        op_gn_apply(z(B * HW, C), bufs["stats"][1], torch.ones((C,), device=dev), z(C), HW, wrong.get("w", W), cpg, stats2=bufs["stats2"][1], out_f32=bufs["f32"][1],
                    out_op=bufs["op"][1], out_halo=bufs["halo"][1], out_format=wrong.get("out_format", PREC_F32), **kw)
    torch.cuda.synchronize()
    for k, (whole, _) in bufs.items():
        assert bool((whole == 0xFF).all()), f"{name}: {k} was written by a refused launch"


def test_gn_apply_cases_covered_every_instantiation_and_mode():
    """Closing test: the (OUT, U, statistics mode) triples of the launches that ran are the table's -- every OUT x U of gn_apply_kernel, every mode."""
    if RAN != set(T.CASE):
        pytest.skip("only part of the case table ran in this session")
    assert SEEN == {c.triple for c in T.CASES}
    assert {t[:2] for t in SEEN} == {(o, u) for o in range(4) for u in (1, 2, 4)} and {t[2] for t in SEEN} == {"0s", "0f", 1, 2}
