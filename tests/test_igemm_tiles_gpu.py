"""GPU: every tile configuration of csrc/igemm.hip -- every row of tests/igemm_refs.py's table, per operand family -- at the shapes where the ring and the
tile addressing can go wrong (fewer k-tiles than ring slots, exactly NS - 1 and NS of them, every slot reused twice; M = 1, N = 4, M = BM +- 1,
N = BN +- 4; Linear rows with ldx > K and NaN behind K; 3 x 3 convolutions whose M-tiles straddle image rows and batch images; split-K with 2, a
non-dividing number and one k-tile per split, eager and deferred), against float64 products of the operands the launch was given.

Per launch: bias and res1 are present (both residual paths), out_f32 and -- for the convolutions -- a haloed operand copy are written into 0xFF-filled
buffers between 0xFF guards.  The exact data set (small integers) must match the float64 result bitwise; the real data set must stay within the a-priori
bound of igemm_refs (no element excluded); the copy must be RN16(relu(out_f32)) bitwise with an untouched ring; guards intact; split-K launches leave
their counters at zero, never read their NaN-filled scratch before writing it, and two launches agree bitwise.  test_forward_picks_are_rows closes the
table over what the three models' forwards select.

Measured on MI355X: the worst error / bound of the real data set over every row and case of a family (each test prints its row's figure with -s).
The exact data set matched bitwise everywhere; no kernel was found to be wrong.

    family  rows  cases  worst error / bound (row)
    bf16      38    327  0.295 (8)     32 x 32 x 16 MFMA rows 40-45: 0.058 .. 0.226
    f16       38    327  0.326 (10)    32 x 32 x 16 MFMA rows 40-45: 0.126 .. 0.249
    f32        5     32  0.354 (3)
    x3        17    133  0.274 (0)
    x2w        4     32  0.156 (2)

Each family's largest figure is that of a one-k-tile case (K = 32 or 64: bf16 257 x 260 x 64, f16 129 x 260 x 64, f32 24575 x 132 x 32, x3 129 x 132 x 32,
x2w 129 x 132 x 64), where the bound is a handful of roundings; 76 of the 102 rows have their largest figure there.
"""
import functools

import pytest
import torch

from tests import igemm_refs as G

pytestmark = pytest.mark.gpu

WORST = {}


def _launch(dev, family, c, d, ops, bufs):
    from soccdpt_amd.lib import op_igemm
    kw = dict(taps=c.taps, out_f32=bufs["out"][1].view(torch.float32), precision=G.PREC[family], tune=c.tune)
    if not c.sk_defer:
        kw.update(bias=ops["bias"], res1=ops["res1"])
    if c.kind == "linear":
        kw.update(ldx=c.ldx)
    else:
        kw.update(H=c.H, W=c.W, act=1, out_bf16=bufs["copy"][1].view(G.copy_dtype(family)), out_halo=1)
        if family == "x3":
            kw.update(out_fmt=1)
    if c.splitk > 1:
        kw.update(splitk=c.splitk, sk_part=bufs["part"][1].view(torch.float32), sk_count=bufs["count"][1].view(torch.int32), sk_defer=c.sk_defer)
    op_igemm(ops["X"], ops["Wt"], c.M, c.N, c.Cin, **kw)
    torch.cuda.synchronize()


def _buffers(dev, family, key, c):
    r = G.TABLE[family][key]
    b = {"out": G.guarded(c.M * c.N * 4, dev)}
    if c.kind == "conv":
        es = torch.empty((), dtype=G.copy_dtype(family)).element_size()
        b["copy"] = G.guarded(c.B * (c.H + 2) * (c.W + 2) * c.N * es, dev)
    if c.splitk > 1:
        b["part"] = G.guarded(c.splitk * c.M * c.N * 4, dev)            # 0xFF = NaN: a partial read before it was written poisons the result
        b["count"] = G.guarded(-(-c.M // r.BM) * -(-c.N // r.BN) * 4, dev)
        b["count"][1].zero_()
    return b


def run_case(dev, family, key, c, dataset):
    """One launch (two under split-K) of case c with every check; returns the worst error / bound."""
    d = G.make_data(c, family, dataset)
    ref = G.reference(c, family, key, d, dev)
    ops = dict(X=G.device_operand(d["X_src"], G.x_fmt(family), dev), Wt=G.device_operand(d["Wt_src"], G.w_fmt(family), dev),
               bias=d["bias"].float().to(dev), res1=d["res1"].float().to(dev))
    what = f"{family}-{key} {c.what} ({c.M} x {c.N} x {c.taps * c.Cin}) [{dataset}]"
    outs = []
    for rep in range(2 if c.splitk > 1 else 1):
        bufs = _buffers(dev, family, key, c)
        _launch(dev, family, c, d, ops, bufs)
        out = bufs["out"][1].view(torch.float32).reshape(c.M, c.N)
        ratio = G.check_out(c, dataset, ref, out, what)
        if c.kind == "conv":
            G.check_copy(c, family, out, bufs["copy"][1].view(G.copy_dtype(family)), what)
        for name, (whole, _) in bufs.items():
            G.check_guards(whole, f"{what}: {name}")
        if c.splitk > 1:
            assert int(bufs["count"][1].view(torch.int32).abs().sum()) == 0, f"{what}: split-K counters not back at zero"
        outs.append(out.cpu())
    if len(outs) == 2:
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what}: two split-K launches differ"
    return ratio


@pytest.mark.parametrize("fk", G.configs(), ids=G.config_id)
def test_igemm_tile_configuration(gpu_device, fk):
    family, key = fk
    worst, at = 0.0, ""
    for c in G.cases(family, key):
        for dataset in ("exact", "real"):
            ratio = run_case(gpu_device, family, key, c, dataset)
            if ratio > worst:
                worst, at = ratio, f"{c.what}, {c.M} x {c.N} x {c.taps * c.Cin}"
    WORST[family] = max(WORST.get(family, 0.0), worst)
    print(f"igemm {family}-{key}: {len(G.cases(family, key))} cases x 2 data sets, worst error / bound {worst:.3f} at [{at}] (family so far {WORST[family]:.3f})")


def test_shapes_that_leave_a_row_are_refused(gpu_device):
    """The shapes the generator had to move because the launcher refuses them: N <= 32 with Cin % 64 != 0 in the 16-bit and x2w families."""
    from soccdpt_amd.lib import op_igemm
    for family in ("bf16", "f16", "x2w"):
        c = G.Case("linear", 1, 4, 32, 1, 48, 0, 0, 0, 4 if family != "x2w" else -1, 1, 0, "")
        d = G.make_data(c, family, "exact")
        out = torch.zeros(1, 4, device=gpu_device)
        with pytest.raises(RuntimeError, match="Cin % 64"):
            op_igemm(G.device_operand(d["X_src"], G.x_fmt(family), gpu_device), G.device_operand(d["Wt_src"], G.w_fmt(family), gpu_device), 1, 4, 32, ldx=48,
                     out_f32=out, precision=G.PREC[family], tune=c.tune)
        torch.cuda.synchronize()
        assert float(out.abs().sum()) == 0.0


@pytest.mark.parametrize("family,ldx,why", [("bf16", 68, "16 bytes"), ("f16", 68, "16 bytes"), ("x2w", 68, "16 bytes"), ("f32", 66, "16 bytes"),
                                            ("bf16", 32, "shorter than a row"), ("f16", 0, "shorter than a row"), ("f32", 32, "shorter than a row"),
                                            ("x3", 32, "shorter than a row"), ("x2w", 0, "shorter than a row")])
def test_plain_mode_ldx_is_refused(gpu_device, family, ldx, why):
    """launch_igemm refuses plain-mode rows that do not start on 16 bytes (bf16 / f16 / f32) and, without row groups or a second segment, ldx < Cin
    (0, op_igemm's default, included): nothing is launched, the output is still 0xFF."""
    from soccdpt_amd.lib import op_igemm
    M, N, K = 5, 36, 64
    x = G.device_operand(torch.ones(M, 96), G.x_fmt(family), gpu_device)      # larger than any row the refused descriptor names
    w = G.device_operand(torch.ones(N, K), G.w_fmt(family), gpu_device)
    whole, payload = G.guarded(M * N * 4, gpu_device)
    with pytest.raises(RuntimeError, match=why):
        op_igemm(x, w, M, N, K, ldx=ldx, out_f32=payload.view(torch.float32), precision=G.PREC[family])
    torch.cuda.synchronize()
    assert bool((whole == 0xFF).all())


MODELS = {"tiny_256": ("dpt_swin2_tiny_256", "swin2t16_256", 256, 8), "base_384": ("dpt_swin2_base_384", "swin2b24_384", 384, 8),
          "hybrid_384": ("dpt_hybrid_384", "vitb_rn50_384", 384, 4)}   # (model type, backbone, image size, the benchmark's batch)


@functools.lru_cache(maxsize=1)
def _state_dict(backbone):
    from soccdpt_amd.utils.synth import synth_state_dict
    return synth_state_dict(backbone, alias_pretrained=True)


@pytest.mark.parametrize("mode", ["bf16", "f16", "f16x3"])
@pytest.mark.parametrize("model", list(MODELS))
def test_forward_picks_are_rows(gpu_device, model, mode, tmp_path):
    """Every configuration id the forward's sites report, at the benchmark's batch size and at B = 1, is a row of the table of the mode's family.
    What this does not show: a site record carries the id of igemm_config_id and no operand family, so the family is taken from the run mode (and the
    hybrid's stem GEMM, K = 160, which runs the x3 tiles in every mode); for launches with a LayerNorm, statistics, generalised-addressing, dot3 or
    split-K instantiation the id names the tile rule, not the instantiation that ran, and ids 0-12 are rows of both the 16-bit and the x3 table."""
    from soccdpt_amd.lib import PREC_BF16, PREC_F16, PREC_F16X3
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_input, write_synth_calib
    model_type, backbone, img, batch = MODELS[model]
    calib = write_synth_calib(str(tmp_path / "calib.yaml"))
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, model_type=model_type,
                   precision={"bf16": PREC_BF16, "f16": PREC_F16, "f16x3": PREC_F16X3}[mode])
    m.load_state_dict(_state_dict(backbone), strict=False)
    m = m.eval().to(gpu_device)
    eng = m._engine(gpu_device)
    eng.profile_sites(True)
    eng.profile_enable(True)
    for B in (batch, 1):
        m.network(synth_input(B, size=img, seed0=3).to(gpu_device))
    torch.cuda.synchronize()
    eng.profile_collect()
    eng.profile_enable(False)
    sites = eng.sites()
    assert len(sites) > 10
    picked = set()
    for s in sites:
        # the hybrid's stem GEMM (K = 160) runs the x3 tiles in every 16-bit mode; everything else runs the mode's family
        fam = "x3" if mode == "f16x3" or (model == "hybrid_384" and s["K"] == 160 and s["taps"] == 1) else mode
        assert s["cfg"] in G.TABLE[fam], f"{model} {mode}: site {s} selects a configuration that is no row of the {fam} table"
        picked.add((fam, s["cfg"]))
    print(f"{model} {mode}: {len(sites)} sites select {sorted(picked)}")
