"""GPU: the statistics (ST) and generalised-addressing (GEN) instantiations of csrc/igemm.hip -- every row of tests/igemm_gen_refs.py's table, per operand
family, one launch at a time -- at the smallest non-square shapes where the strided / gathered / grouped / two-segment addressing and the per-tile
statistics layout can go wrong, against float64 products of the operands the launch was given and float64 sums of the launch's own output.

Per launch: out_f32 (and, for the 3x3 GEN cases, bias + res1 + ReLU + a haloed operand copy in the output geometry) into 0xFF-filled buffers between 0xFF
guards; the exact data set must match float64 bitwise, the real one element-wise within igemm_refs' a-priori bound, no element excluded; gn_part is read
as [M tile][N / cpg][2] with the row's BM and held to gamma(BM cpg) sum |v| (sum v^2), bitwise under the exact set, the floats behind the last entry
still 0xFF; gn_stats is untouched without gn_count and {mean, rstd} within the propagated bound -- and within two f32 roundings of the float64 formula on
the device's own partials -- with it; s1_gen equals the row's plain instantiation bitwise; split-K leaves its counters at zero and two launches agree
bitwise.  test_refusals_launch_nothing holds the refusals, test_hybrid_forward_picks_are_rows closes the table over dpt_hybrid_384's forward.

Measured on MI355X: the worst error / bound of the real data set over every row and case of a family, with (row: case) (each test prints its row's
figures with -s).  The exact data set matched bitwise everywhere, partials included; no kernel was found to be wrong.  The asserts are the a-priori
bounds; these ratios are only recorded.  The statistics bounds count every one of the BM x cpg f32 additions as a worst-case rounding, hence the small
ratios; what they still reject is what tests/test_igemm_gen_refs.py plants.

    family  rows  cases  out_f32                      partial sums                     partial squares                   mean / rstd
    bf16       7     77  0.301 (2: gather_s2, 1 kt)   0.041 (20: linear, cpg 2)        0.045 (20: linear, cpg 2)         0.018 / 0.015 (20: linear dc, cpg 4)
    f16        7     77  0.264 (21: gather_s2, 1 kt)  0.024 (20: same_s2 4x8, cpg 2)   0.035 (20: same_s2 4x8, cpg 2)    0.020 / 0.015 (20: linear dc, cpg 4)
    f32        4     20  0.169 (1: gather_s2, 1 kt)   0.005 (1: linear, cpg 2)         0.018 (1: same_s2 4x16, cpg 2)    0.005 / 0.005 (1: linear dc, cpg 8)
    x3         8     53  0.227 (1, 4: gather_s2, 1 kt) 0.008 (4, 12: linear dc, cpg 4) 0.018 (1, 4: same_s2 4x16, cpg 2) 0.008 / 0.007 (4, 12: linear dc, cpg 4)
    x2w        2     34  0.259 (0: gather_s2, 1 kt)   0.007 (0: linear dc, cpg 4)      0.019 (0: linear, cpg 2)          0.007 / 0.006 (0: linear dc, cpg 4)

out_f32's largest figure is in every family that of the one-k-tile strided gather (K = 32 .. 128: the bound is a handful of roundings), the partials' that
of gn_cpg 2 on the ragged N = BN + BN / 2 or of the dc case, where all terms have one sign.  The two grid-selected 128 x 128 tiles (f32 0 and x3 0 with
generalised addressing, 32768 x 128 x 32) gave 0.149 and 0.107 for out_f32 and at most 0.001 for the partials.
"""
import functools

import pytest
import torch

from tests import igemm_gen_refs as T
from tests import igemm_refs as G

pytestmark = pytest.mark.gpu


def _buffers(dev, family, key, c):
    r = T.row(family, key)
    b = {"out": G.guarded(c.M * c.N * 4, dev)}
    if c.copy:
        es = torch.empty((), dtype=G.copy_dtype(family)).element_size()
        b["copy"] = G.guarded(c.B * (c.H + 2) * (c.W + 2) * c.N * es, dev)
    grid = -(-c.M // r.BM) * -(-c.N // r.BN)
    if c.splitk > 1:
        b["part"] = G.guarded(c.splitk * c.M * c.N * 4, dev)            # 0xFF = NaN: a partial read before it was written poisons the result
        b["count"] = G.guarded(grid * 4, dev)
        b["count"][1].zero_()
    if c.st:
        b["gn_part"] = G.guarded((T.part_floats(c, r) + T.PART_SLACK) * 4, dev)
        b["gn_stats"] = G.guarded((c.M // c.hw) * (c.N // c.cpg) * 2 * 4, dev)
        if c.count:
            b["gn_count"] = G.guarded((c.M // c.hw) * 4, dev)
            b["gn_count"][1].zero_()
    if c.stamps:
        b["stamps"] = G.guarded(grid * c.splitk * 4 * 8, dev)
    return b


def _kwargs(family, c, ops, bufs, twin=False):
    kw = dict(taps=c.taps, out_f32=bufs["out"][1].view(torch.float32), precision=G.PREC[family], tune=c.tune)
    if c.epi:
        kw.update(bias=ops["bias"], res1=ops["res1"])
    if c.kind == "linear":
        kw.update(ldx=c.ldx, grp_rows=c.grp_rows, grp_off=c.grp_off, grp_stride=c.grp_stride, seg2_k=c.seg2_k, seg2_off=c.seg2_off)
    else:
        kw.update(H=c.H, W=c.W)
        if c.gen_conv and not twin:
            kw.update(conv=dict(stride=c.stride, pad=c.pad, in_halo=c.in_halo, Hi=c.Hi, Wi=c.Wi), gather1=int(c.kind == "gather"))
    if c.copy:
        kw.update(act=1, out_bf16=bufs["copy"][1].view(G.copy_dtype(family)), out_halo=1)
        if family == "x3":
            kw.update(out_fmt=1)
    if c.splitk > 1:
        kw.update(splitk=c.splitk, sk_part=bufs["part"][1].view(torch.float32), sk_count=bufs["count"][1].view(torch.int32))
    if c.st:
        kw.update(gn_stats=bufs["gn_stats"][1].view(torch.float32), gn_part=bufs["gn_part"][1].view(torch.float32), gn_cpg=c.cpg, gn_hw=c.hw,
                  gn_count=bufs["gn_count"][1].view(torch.int32) if c.count else None)
    if c.stamps and not twin:
        kw.update(stamps=bufs["stamps"][1].view(torch.int64))
    return kw


def _operands(dev, family, d):
    return dict(X=G.device_operand(d["X_src"], G.x_fmt(family), dev), Wt=G.device_operand(d["Wt_src"], G.w_fmt(family), dev),
                bias=d["bias"].float().to(dev), res1=d["res1"].float().to(dev))


def run_case(dev, family, key, c, dataset):
    """The launches of case c (two under split-K; the plain twin of s1_gen) with every check; returns the worst error / bound of out_f32, the partial sums,
    the partial sums of squares, mean and rstd."""
    from soccdpt_amd.lib import op_igemm
    r = T.row(family, key)
    d = T.make_data(c, family, dataset)
    ref = T.reference(c, family, key, d, dev)
    ops = _operands(dev, family, d)
    what = f"{family}-{key} {c.name} ({c.M} x {c.N} x {c.K}) [{dataset}]"
    ratios = [0.0] * 5
    outs = []
    for rep in range(2 if (c.splitk > 1 or c.twin) else 1):
        twin = c.twin and rep == 1
        bufs = _buffers(dev, family, key, c)
        op_igemm(ops["X"], ops["Wt"], c.M, c.N, c.Cin, **_kwargs(family, c, ops, bufs, twin))
        torch.cuda.synchronize()
        out = bufs["out"][1].view(torch.float32).reshape(c.M, c.N)
        ratios[0] = max(ratios[0], G.check_out(c.plain(), dataset, ref, out, what))
        if c.copy:
            G.check_copy(c.plain(), family, out, bufs["copy"][1].view(G.copy_dtype(family)), what)
        for name, (whole, _) in bufs.items():
            G.check_guards(whole, f"{what}: {name}")
        if c.splitk > 1:
            assert int(bufs["count"][1].view(torch.int32).abs().sum()) == 0, f"{what}: split-K counters not back at zero"
        if c.st:
            part = bufs["gn_part"][1].view(torch.float32)
            ratios[1:3] = T.check_part(c, r, dataset, out, part, what)
            if c.dc:
                T.check_dc(c, out)
            if c.count:
                ratios[3:5] = T.check_stats(c, r, out, part, bufs["gn_stats"][1].view(torch.float32).reshape(c.M // c.hw, c.N // c.cpg, 2), what)
                assert int(bufs["gn_count"][1].view(torch.int32).abs().sum()) == 0, f"{what}: gn_count was written"
            else:
                assert bool((bufs["gn_stats"][1] == 0xFF).all()), f"{what}: gn_stats was written without gn_count"
        outs.append(out.cpu())
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), \
            f"{what}: " + ("the GEN and the plain instantiation differ" if c.twin else "two split-K launches differ")
    return ratios


NAMES = ("out_f32", "partial sums", "partial squares", "mean", "rstd")


@pytest.mark.parametrize("fk", T.configs(), ids=G.config_id)
def test_igemm_gen_st_row(gpu_device, fk):
    family, key = fk
    worst, at = [0.0] * 5, [""] * 5
    cs = T.cases(family, key)
    for c in cs:
        for dataset in c.datasets:
            for i, v in enumerate(run_case(gpu_device, family, key, c, dataset)):
                if v > worst[i]:
                    worst[i], at[i] = v, c.name
    print(f"igemm-gen {family}-{key}: {len(cs)} cases, {sum(len(c.datasets) for c in cs)} data sets; worst error / bound: " +
          "; ".join(f"{n} {w:.3f} [{a}]" for n, w, a in zip(NAMES, worst, at) if a))


def _refusal_cases(family):
    """(what, row key, case, changes to the launch's keyword arguments, short part by one float, message)."""
    from dataclasses import replace
    gkey = {"bf16": 2, "f16": 2, "x3": 1, "f32": 1, "x2w": 0}[family]
    skey = {"bf16": 23, "f16": 23, "x3": 4, "f32": 1, "x2w": 0}[family]
    r = T.row(family, skey)
    gen = {c.name.split(",")[0]: c for c in T.cases(family, gkey)}
    st = next(c for c in T.cases(family, skey) if c.st and c.kind == "linear" and not c.count)
    out = [("gn_part one float too short", skey, st, {}, True, "GroupNorm-statistics"),
           ("gn_hw no multiple of BM", skey, replace(st, hw=r.BM // 2), {}, False, "GroupNorm-statistics"),
           ("gn_cpg does not divide BN", skey, replace(st, N=3 * r.BN, cpg=12), {}, False, "GroupNorm-statistics"),
           ("a tap leaves the input image", gkey, replace(gen["same_s2"], Hi=gen["same_s2"].Hi - 2), {}, False, "leave the input image"),
           ("seg2_k no multiple of 128", gkey, replace(gen["readout"], seg2_k=64), {}, False, "second-segment"),
           ("seg2_k >= Cin", gkey, replace(gen["readout"], seg2_k=gen["readout"].Cin), {}, False, "second-segment"),
           ("row groups with taps 9", gkey, gen["same_s2"], {"grp_rows": 5, "grp_stride": 64, "conv": None}, False, "row groups")]
    if family in ("bf16", "f16"):
        out += [("a row without statistics", skey, replace(st, tune=0), {}, False, "no GroupNorm-statistics instantiation"),
                ("a row without generalised addressing", gkey, replace(gen["gather_s2"], tune=0), {}, False, "no generalised-addressing instantiation"),
                ("row 4 with generalised addressing and no statistics", gkey, replace(gen["gather_s2"], tune=4), {}, False, "no generalised-addressing instantiation")]
    if family == "x3":
        out += [("x3 12 with generalised addressing", gkey, replace(gen["gather_s2"], tune=12), {}, False, "configuration 12 has no generalised addressing"),
                ("x3 12 with statistics and generalised addressing", skey, replace(next(c for c in T.cases("x3", 4) if c.st and c.kind == "gather"), tune=12), {}, False,
                 "configuration 12 has no generalised addressing")]
    return out


@pytest.mark.parametrize("family", G.FAMILIES)
def test_refusals_launch_nothing(gpu_device, family):
    """What launch_igemm must refuse: nothing is launched, every buffer is still 0xFF."""
    from soccdpt_amd.lib import op_igemm
    for what, key, c, changes, short, msg in _refusal_cases(family):
        d = T.make_data(_storage_case(c), family, "exact")
        ops = _operands(gpu_device, family, d)
        bufs = _buffers(gpu_device, family, key, _storage_case(c))
        kw = _kwargs(family, c, ops, bufs)
        kw.update(changes)
        if short:
            kw["gn_part"] = kw["gn_part"][:T.part_floats(c, T.row(family, key)) - 1]
        with pytest.raises(RuntimeError, match=msg):
            op_igemm(ops["X"], ops["Wt"], c.M, c.N, c.Cin, **kw)
        torch.cuda.synchronize()
        for name, (whole, payload) in bufs.items():
            if name not in ("count", "gn_count"):
                assert bool((whole == 0xFF).all()), f"{family} {what}: {name} was written by a refused launch"


def _storage_case(c):
    """A refused descriptor need not be consistent; its operands and buffers are sized by a consistent one that is at least as large."""
    from dataclasses import replace
    if c.kind != "linear" and (c.Hi or c.H) < 2 * c.H - 1 and c.gen_conv and c.stride == 2:
        c = replace(c, Hi=2 * c.H)
    if c.seg2_k and (c.seg2_k % 128 or c.seg2_k >= c.Cin):
        c = replace(c, seg2_k=128)
    return c


# per sample of dpt_hybrid_384 at 384 x 384: (pixels, N, K, taps) of the launches that need a statistics or generalised-addressing instantiation
_P = {192: 192 * 192, 96: 96 * 96, 48: 48 * 48, 24: 24 * 24}
HYBRID_SITES = {
    "stem (GroupNorm)": (_P[192], 64, 160, 1),
    "stage 1 conv1 (GroupNorm)": (_P[96], 64, 64, 1), "stage 1 conv2 (GroupNorm)": (_P[96], 64, 576, 9), "stage 1 conv3 / shortcut (GroupNorm)": (_P[96], 256, 64, 1),
    "stage 1 conv1 of later blocks (GroupNorm)": (_P[96], 64, 256, 1),
    "stage 2 conv1 of the first block (GroupNorm)": (_P[96], 128, 256, 1), "stage 2 conv2, the first at stride 2 (GroupNorm)": (_P[48], 128, 1152, 9),
    "stage 2 conv3 (GroupNorm)": (_P[48], 512, 128, 1), "stage 2 shortcut: strided 1x1 (GroupNorm)": (_P[48], 512, 256, 1), "stage 2 conv1 (GroupNorm)": (_P[48], 128, 512, 1),
    "stage 3 conv1 of the first block (GroupNorm)": (_P[48], 256, 512, 1), "stage 3 conv2, the first at stride 2 (GroupNorm)": (_P[24], 256, 2304, 9),
    "stage 3 conv3 (GroupNorm)": (_P[24], 1024, 256, 1), "stage 3 shortcut: strided 1x1 (GroupNorm)": (_P[24], 1024, 512, 1), "stage 3 conv1 (GroupNorm)": (_P[24], 256, 1024, 1),
    "read-out projection (K = 2 x 768)": (576, 768, 1536, 1),
    "act_postprocess4: Conv2d(3, 2, 1)": (144, 768, 6912, 9),
}


@functools.lru_cache(maxsize=1)
def _state_dict():
    from soccdpt_amd.utils.synth import synth_state_dict
    return synth_state_dict("vitb_rn50_384", alias_pretrained=True)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3", "mixed"])
def test_hybrid_forward_picks_are_rows(gpu_device, mode, tmp_path):
    """dpt_hybrid_384 at B = 1 and B = 4 with site profiling on: every site with taps 9 at stride 2, a strided 1x1, K = 2 x 768 or a GroupNorm consumer
    reports a configuration id that is a row of GTABLE, and every such launch of the architecture (HYBRID_SITES) is among the sites.
    What the site record (M, N, K, taps, id) cannot show: neither the stride nor the consumer, so the sites are recognised by their shapes, which the
    architecture fixes -- and a decoder convolution of the same shape as a ResNetV2 one (3x3, 256 -> 256 at 24 x 24) shares its record, whose id is that of
    the first launch, the ResNetV2 one (across batch sizes it would be the other way round: 4 x 12 x 12 = 24 x 24, hence one record list per B); no operand family, so it is the run mode's (the stem's K = 160 GEMM runs x3 tiles in every mode), and in the mixed mode, where a
    launch is fp16, x3 or x2w by the precision map and a shape has one record per format, one record of the shape has to hold a row of one of the three
    tables (for an x2w launch the record holds the 16-bit rule's id, not the x2w tile that ran); and the id names the tile rule, not the instantiation: that the row carries the instantiation is the table's statement,
    which test_igemm_gen_st_row holds against a launch."""
    from soccdpt_amd.lib import PREC_BF16, PREC_F16, PREC_F16X3, PREC_MIXED
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_input, write_synth_calib
    calib = write_synth_calib(str(tmp_path / "calib.yaml"))
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, model_type="dpt_hybrid_384",
                   precision={"bf16": PREC_BF16, "f16": PREC_F16, "f16x3": PREC_F16X3, "mixed": PREC_MIXED}[mode])
    m.load_state_dict(_state_dict(), strict=False)
    m = m.eval().to(gpu_device)
    eng = m._engine(gpu_device)
    picked = {}
    for B in (4, 1):
        eng.profile_sites(True)          # a record list per batch size: M = B x pixels of one map is M of another map at the other B
        eng.profile_enable(True)
        m.network(synth_input(B, size=384, seed0=3).to(gpu_device))
        torch.cuda.synchronize()
        eng.profile_collect()
        eng.profile_enable(False)
        sites = eng.sites()
        for name, (px, N, K, taps) in HYBRID_SITES.items():
            hits = [s for s in sites if (s["M"], s["N"], s["K"], s["taps"]) == (B * px, N, K, taps)]
            assert hits, f"hybrid_384 {mode} B {B}: no site of the shape of {name}: {(B * px, N, K, taps)}"
            fams = ("f16", "x3", "x2w") if mode == "mixed" else (("x3",) if mode == "f16x3" or K == 160 else (mode,))
            rows = [s for s in hits if any(s["cfg"] in T.GTABLE[f] for f in fams)]
            # mixed: the fp16, x3 and x2w launches of a shape are records of their own, and the ResNetV2 launch is one of them
            assert rows and (mode == "mixed" or len(rows) == len(hits)), \
                f"hybrid_384 {mode} B {B}: {name}: sites {hits} select a configuration that is no row of the table of {fams}"
            for s in rows:
                picked.setdefault(s["cfg"], set()).add(name.split(" (")[0])
    print(f"hybrid_384 {mode}: " + "; ".join(f"{k}: {len(v)} kinds of launch" for k, v in sorted(picked.items())))
