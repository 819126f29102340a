"""CPU: the bounds of tests/metrics_refs.py admit float32 emulations of the metric kernels' arithmetic (with and without contraction) on every case of the
tables, refuse each named defect on at least one case, the committed inputs keep det away from cancellation and the undecided pixels under their cap, and the
references agree with oracle/metrics_ref.py (the restatement of the reference's functions) where that one is defined the same way."""
import numpy as np
import pytest
import torch

from oracle import metrics_ref as MR
from tests import metrics_refs as R

SMALL = [c for c in R.DEPTH_CASES if c != f"npix {R.DEPTH_NPIX[-1]}"]


@pytest.fixture(scope="module")
def cases():
    return {c: R.depth_case(c) for c in R.DEPTH_CASES}


@pytest.mark.parametrize("contract", [False, True])
@pytest.mark.parametrize("case", R.DEPTH_CASES)
def test_emulation_is_admitted(cases, case, contract):
    p, g, m = cases[case]
    out = R.emulate_depth(p, g, m, contract)
    a, b = R.check_depth(out, p, g, m, case)
    print(f"{case} contract {contract}: scale/shift {a:.3f}, metrics {b:.3f} of the bound")
    pp, pg = R.poison(p, g, m)
    assert torch.equal(R.emulate_depth(pp, pg, m, contract).view(torch.int32), out.view(torch.int32)), "masked-out values entered a sum"


def test_inputs_are_conditioned_and_decided(cases):
    for case, (p, g, m) in cases.items():
        *_, det, Edet = R.ref_scale_shift(p, g, m)
        live = (det != 0) & (det == det)
        assert bool((Edet[live] <= R.MAX_DET_ERROR * det[live].abs()).all()), case
        out = R.emulate_depth(p, g, m)
        T = R.ref_metrics(out[7::2], out[8::2], p, g, m)
        assert max(T.undecided) <= R.MAX_UNDECIDED, (case, T.undecided)


def test_cases_reach_what_they_are_for(cases):
    p, g, m = cases["empty and single"]
    *_, det, _ = R.ref_scale_shift(p, g, m)
    assert float(det[1]) == 0 and float(det[2]) == 0 and float(det[0]) != 0 and int(m[2].sum()) == 1
    x = float(p[2, 123])
    assert float(torch.tensor(x * x, dtype=torch.float64).float()) != x * x, "p^2 is not representable: det is 0 only through the float32 rounding"
    out = R.emulate_depth(p, g, m)
    assert float(out[7 + 4]) == 0 and float(out[8 + 4]) == 0 and float(out[7]) != 0
    p, g, m = cases["exact thresholds"]
    out = R.emulate_depth(p, g, m)
    assert float(out[7]) == 1.0 and float(out[8]) == 0.0
    T = R.ref_metrics(out[7::2], out[8::2], p, g, m)
    assert T.undecided == [0.0, 0.0, 0.0] and T.lo == T.hi
    assert [float(v) for v in out[4:7]] == T.lo and T.lo[0] == 0.0 and 0 < T.lo[1] < T.lo[2] < 1      # a ratio equal to a threshold is a miss
    p, g, m = cases["negative aligned"]
    out = R.emulate_depth(p, g, m)
    q = out[7::2].view(2, 1) * p + out[8::2].view(2, 1)
    assert int(((q < 0) & (m != 0)).sum()) >= 3 and float(out[3]) == 0 and float(out[2]) > 0
    p, g, m = cases["non-positive gt"]
    out = R.emulate_depth(p, g, m)
    assert float(out[0]) == 0 and float(out[1]) == 0 and float(out[3]) == 0 and float(out[2]) > 0
    assert bool(((g <= 0) & (m != 0)).sum() == 3)
    p, g, m = cases["mask bytes"]
    assert {0, 1, 2, 255, 128} == set(m.unique().tolist())
    out = R.emulate_depth(*cases["nan under the mask"])
    assert bool((out[:7] == 0).all()) and bool(torch.isnan(out[7:]).all())
    out = R.emulate_depth(*cases["all empty"])
    assert bool((out == 0).all())
    assert R.DEPTH_NPIX[-1] == 512 * 2048 + 1 and R.DEPTH_B[-1] == 256


def test_against_the_oracle_restatement(cases):
    """oracle/metrics_ref.py sums in float32 and multiplies by the mask; on healthy inputs it agrees with the float64 terms to its own summation error."""
    for case in ("npix 2049", "B 2", "empty and single", "mask bytes"):
        p, g, m = cases[case]
        ref = MR.depth_metrics_batch(p.unsqueeze(1), g.unsqueeze(1), (m != 0).unsqueeze(1))
        out = R.emulate_depth(p, g, m)
        np.testing.assert_allclose(out[:7].numpy(), np.array(ref[:7], dtype=np.float64), rtol=2e-4, atol=1e-6)
        np.testing.assert_allclose(out[7::2].numpy(), ref[7], rtol=2e-4, atol=1e-6)
    out = R.emulate_depth(*cases["nan under the mask"])
    p, g, m = cases["nan under the mask"]
    ref = MR.depth_metrics_batch(p.unsqueeze(1), g.unsqueeze(1), (m != 0).unsqueeze(1))
    assert all(float(v) == 0 for v in ref[:7]) and bool(np.isnan(ref[7]).all())
    # the divergence: a NaN at a masked-out pixel poisons the reference's sums and not ours
    p, g, m = cases["B 2"]
    pp, pg = R.poison(p, g, m)
    ref = MR.depth_metrics_batch(pp.unsqueeze(1), pg.unsqueeze(1), (m != 0).unsqueeze(1))
    assert bool(np.isnan(ref[7]).all())
    for name in R.IOU_CASES:
        pr, t = R.iou_case(name)
        np.testing.assert_allclose(R.ref_iou(pr, t).numpy(), MR.iou_batch(pr.unsqueeze(-1), t.unsqueeze(-1)), rtol=1e-6)


@pytest.mark.parametrize("defect", R.DEPTH_DEFECTS)
def test_depth_defects_are_refused(cases, defect):
    refused = []
    for case in SMALL:
        p, g, m = cases[case]
        try:
            R.check_depth(R.emulate_depth(p, g, m, defect=defect), p, g, m, case)
        except AssertionError:
            refused.append(case)
    assert refused, f"no case refuses: {defect}"
    print(f"{defect}: refused by {refused}")


@pytest.mark.parametrize("defect", R.IOU_DEFECTS)
def test_iou_defects_are_refused(defect):
    refused = [n for n in R.IOU_CASES if not torch.equal(R.ref_iou(*R.iou_case(n), defect=defect).view(torch.int32), R.ref_iou(*R.iou_case(n)).view(torch.int32))]
    assert refused, defect
    print(f"{defect}: refused by {refused}")


def test_iou_cases_reach_their_edges():
    for name, (B, C, npix) in R.IOU_CASES.items():
        p, t = R.iou_case(name)
        assert p.shape == (B, C, npix)
        if npix > 1:
            for v in (0.5, 0.5 + 2.0 ** -24):
                assert bool((p == v).any()) and bool((t == v).any())
            assert bool(torch.isnan(p).any()) and bool((p == float("inf")).any()) and bool((t == float("-inf")).any())
        assert float(R.ref_iou(p, t)[-1]) < 1.0
    p, t = R.iou_case("B 300")
    assert float(R.ref_iou(p, t)[-1]) == 0.0          # C = 1 and an empty union
    assert {b for b, _, _ in R.IOU_CASES.values()} >= {65, 300} and {c for _, c, _ in R.IOU_CASES.values()} >= {1, 4}
