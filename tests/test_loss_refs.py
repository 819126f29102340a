"""CPU: the float64 reference, the pins and the bound of tests/loss_refs.py, which tests/test_loss_bound_gpu.py holds csrc/loss.hip to.
  * the float64 reference meets tests/golden/loss.npz (the reference's own ssi_loss module + torch autograd): values and d_seg within the
    tolerances tests/test_oracle_loss.py applies to the float32 restatement, every entry of d_inv within the tolerance tests/test_loss_gpu.py
    applies to the golden (the golden is a float32 result); the directly stated criterion is the oracle wherever both apply;
  * every case satisfies the sign pins, the clamp pins and the conditioning with cap 0: no unpinned pair, no unpinned pixel;
  * the bound accepts the yardstick and rejects each planted fault (a variant of the float64 reference, as the kernel would commit it) in
    the case and slice named in REJECTED_BY."""
import os

import numpy as np
import pytest
import torch

from oracle import loss_ref as LR
from tests import loss_refs as R
from tests.golden_inputs import loss_inputs

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "loss.npz"))

# fault -> (case, slice) that must reject it
REJECTED_BY = {
    "1r": ("8x12-37x53", "d_inv.img0.border"),
    "1c": ("8x12-37x53", "d_inv.img0.border"),
    "2": ("8x12-37x53", "d_inv.img0.interior"),
    "3": ("8x12-37x53", "loss_disp"),
    "4": ("8x12-37x53", "d_inv.img1.interior"),
    "5": ("8x12-37x53", "d_inv.img0.clampfoot"),
    "6": ("8x12-37x53", "d_seg.img0.class2.last"),
    "7": ("8x12-37x53", "loss_seg"),
    "8": ("8x12-37x53", "scale.img1"),
    "9": ("w37", "loss"),
    "10": ("8x12-37x53", "scale.img0"),
}


@pytest.mark.parametrize("tag,compute_ss", [("ss", True), ("noss", False)])
def test_float64_reference_meets_the_golden(tag, compute_ss):
    keys = ("inv", "seg", "y_disp", "mask_disp", "y_seg", "mask_seg")
    ins = dict(zip(keys, loss_inputs()))
    cast = [t.double() if t.is_floating_point() else t for t in ins.values()]
    own = R.criterion(ins, R.Case(2, 3, 64, 64, 135, 240, compute_ss=compute_ss))
    for r in (LR.loss_and_grads(*cast, compute_ss=compute_ss), own):
        assert r["d_inv"].dtype == torch.float64
        got = np.array([float(r["loss"]), float(r["loss_disp"]), float(r["loss_seg"])])
        np.testing.assert_allclose(got, G[f"{tag}_loss"], rtol=1e-6)
        np.testing.assert_allclose(r["d_seg"].numpy(), G[f"{tag}_d_seg"], rtol=1e-5, atol=1e-10)
        # d_inv: the tolerance tests/test_loss_gpu.py applies to this golden, with none of its exemptions.  The 1e-4 relative + 1e-9 that
        # tests/test_oracle_loss.py applies to the float32 restatement (which reproduces the golden bit for bit) cannot hold for a float64
        # evaluation: the golden is a float32 result, 4.4e-6 of its largest entry away from float64 (noss: 12 of 8192 entries miss that
        # tolerance, by at most 4.2e-9 on a largest entry of 1.6e-3; ss: none).
        g = G[f"{tag}_d_inv"]
        diff = np.abs(r["d_inv"].numpy() - g)
        print(f"  {tag}: d_inv {diff.max() / np.abs(g).max():.1e} of the largest entry; {int((diff > 1e-9 + 1e-4 * np.abs(g)).sum())} entries outside 1e-4 relative + 1e-9")
        assert bool((diff <= 1e-3 * np.abs(g) + 2e-4 * np.abs(g).max()).all())
        assert int((r["d_inv"].numpy() == 0).sum()) == int((g == 0).sum())                 # the same clamped-away cells


@pytest.mark.parametrize("name", list(R.CASES))
def test_pins_hold_with_cap_zero(name):
    c, ins = R.CASES[name], R.build(name)
    rep = R.pin_report(ins, c)
    print(f"  {name}: {rep['pairs']} pairs, smallest gap {rep['min_gap_over_margin']:.2f} margins, {ins['nudged']} targets nudged, clamp gap {rep['clamp_gap']:.1e}, "
          f"{rep['clamped']} clamped / {rep['unclamped']} unclamped pixels, conditioning {rep['cond']:.1e}, valid {rep['valid']}")
    assert len(rep["unpinned"]) == 0 and rep["min_gap_over_margin"] >= 1.0
    assert rep["unpinned_pixels"] == 0 and rep["clamp_gap"] >= R.CLAMP_PIN
    assert rep["cond"] >= R.COND_MIN
    forced = R.forced_solve_error(name)
    print(f"  {name}: float32 up-sampling alone moves scale / shift by {forced:.2f} of the yardstick's bound")
    assert forced <= 0.5
    assert (rep["clamped"] == 0) == (name in R.UNCLAMPED_CASES)
    assert rep["unclamped"] > 0 or name == "2x2-1x1"
    assert ins["nudged"] <= 0.02 * c.B * c.H * c.W                     # the nudging touches few pixels (most at 33 x up-sampling, where neighbours nearly agree)
    for k in ("inv", "seg", "y_disp", "y_seg"):
        assert ins[k].dtype == torch.float32 and bool(torch.isfinite(ins[k]).all())


def test_cases_reach_their_edges():
    v = lambda n: R.pin_report(R.build(n), R.CASES[n])["valid"]
    assert v("mid_empty")[1] == 0 and min(v("mid_empty")[0], v("mid_empty")[2]) > 1000
    assert v("two_pixels")[1] == 2 and v("one_pixel")[1] == 1 and v("2x2-1x1-positive") == [1]
    m = R.build("m3_zero")["mask_disp"]
    assert int(m[:, ::8, ::8].sum()) == 0 and int(m[:, ::4, ::4].sum()) > 0
    assert int(R.build("seg_empty")["mask_seg"].sum()) == 0 and int(R.build("class_off")["mask_seg"][:, 1].sum()) == 0
    sat = R.build("seg_sat")
    ny = R.nearest_index(37, 8)
    for row, target in R.SAT_ROWS.items():
        assert sat["seg"][0, 0, row, :4].tolist() == [0.0, 1.0, float(np.float32(1 - 2.0 ** -24)), 2.0 ** -30]
        assert bool((sat["y_seg"][:, 0, ny == row, :] == target).all())
    labels = [s[0] for s in R.slices("seg_sat")["d_seg"]]
    assert "img0.class0.saturated" in labels and "img1.class0.saturated" in labels
    assert any(s[0].endswith(".empty") for s in R.slices("24x16-20x13")["d_seg"]) and any(s[0].endswith(".empty") for s in R.slices("300x300-40x56")["d_seg"])
    assert R.CASES["16x16-258x257"].H * R.CASES["16x16-258x257"].W > 65536 and 3 * 300 * 300 > 262144
    ref = R.evaluate("one_pixel")
    y = R.build("one_pixel")
    assert float(ref["scale"][1]) == 0.0 and float(ref["shift"][1]) == 0.0
    # the data term of the one-pixel image is y^2 / (2 M): the least-squares fit does not exist, nothing is fitted away
    zero_fit = R.criterion(y, R.CASES["one_pixel"]._replace(alpha=0.0))
    with_img0_only = dict(y, mask_disp=y["mask_disp"].clone())
    with_img0_only["mask_disp"][1] = False
    img0 = R.criterion(with_img0_only, R.CASES["one_pixel"]._replace(alpha=0.0))
    M = float(y["mask_disp"].sum())
    yv = float(y["y_disp"][1][y["mask_disp"][1]].double())
    assert abs(float(zero_fit["loss_disp"]) - (float(img0["loss_disp"]) * (M - 1) / M + yv * yv / (2 * M))) < 1e-15


@pytest.mark.parametrize("name", list(R.CASES))
def test_direct_statement_is_the_oracle_and_the_bound_accepts_the_yardstick(name):
    ref, yard = R.evaluate(name, torch.float64), R.evaluate(name, torch.float32)
    assert ref["d_inv"].dtype == torch.float64 and yard["d_inv"].dtype == torch.float32
    if R.oracle_applies(name):
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-4)):
            own, orc = R.criterion(R.build(name), R.CASES[name], dtype), R.oracle(name, dtype)
            for k in own:
                scale = float(orc[k].detach().abs().max())
                assert float((own[k] - orc[k]).detach().abs().max()) <= tol * scale, (k, dtype)
    rows = R.compare(name, yard)
    assert all(r.ok for r in rows), [r for r in rows if not r.ok]
    assert all(r.ok and r.err == 0 for r in R.compare(name, ref))
    # every element of both gradients lies in a slice
    for key in ("d_inv", "d_seg"):
        covered = torch.zeros_like(ref[key], dtype=torch.bool)
        for _, mask, _ in R.slices(name)[key]:
            covered |= mask
        assert bool(covered.all())


@pytest.mark.parametrize("fault", list(R.FAULTS))
def test_bound_rejects_planted_fault(fault):
    name, label = REJECTED_BY[fault]
    bad = R.criterion(R.build(name), R.CASES[name], torch.float64, fault=fault)
    rejected = {r.label: r for r in R.compare(name, bad) if not r.ok}
    print(f"  fault {fault} ({R.FAULTS[fault]}): rejected at {name} by {sorted(rejected)}")
    assert label in rejected, f"fault {fault} passes {name} / {label}"
    r = rejected[label]
    print(f"  {name} {label}: error {r.err:.2e}, bound {r.bound:.2e}")
    assert r.err > 10 * r.bound                                             # by an order of magnitude, not by luck
