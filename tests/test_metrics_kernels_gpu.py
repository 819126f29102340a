"""GPU: the HIP metric reductions (csrc/metrics.hip through the C ABI).

Two layers.  (1) test_depth_and_iou_metrics_match_oracle / test_metrics_full_resolution_and_edge_cases: the Python wrappers against the CPU oracle and the
reference's golden values at two shapes, to the float32 restatement's own summation error (rtol 2e-4 .. 2e-3).  (2) One call at a time through
soccdpt_metrics_depth / soccdpt_metrics_iou against tests/metrics_refs.py (derivations there; tests/test_metrics_refs.py is the CPU companion): scale and
shift against the float32 solve of the float64 sums under a bound that is the conditioning of det; the seven metrics against float64 terms from the scale
and shift the launch returned, each under its term-by-term rounding bound, a1..a3 between the decided and the decided plus undecided counts; IoU bitwise.
Tables: npix 1, 63, 255, 256, 257, 2049 and 512 * 2048 + 1; B 1, 2, 65, 256 (257 refused); an image with an empty mask and one with a single masked pixel
(det exactly 0) beside healthy ones; an all-empty batch; ratios exactly on 1.25, 1.25^2, 1.25^3; non-positive ground truth and negative aligned predictions
under the mask; mask bytes 2, 128, 255; a NaN under the mask; IoU at npix 1 / 257 / 2049, C 1 / 3 / 4, B 65 / 300 with 0.5, the next float above it, NaN and
+-inf among the values and an empty union.

Per call: outputs and scratch are 0xFF bytes beforehand; the scratch is EXACTLY soccdpt_metrics_scratch_bytes(B, C) bytes; a 4 KB 0xFF guard sits behind
every operand, output and the scratch; afterwards every guard and operand is untouched and a second call gives the same bits (the float64 atomics are
added in a varying order: the float32 results must not depend on it for these inputs).  Every depth case runs a second time with NaN and +-inf at every
masked-out pixel and must give the same bits: masked-out values are never read into a sum (a deliberate divergence from the reference, which multiplies by
the mask).  A refused call launches nothing and leaves every output at its sentinel.  A HIP error ends the session.

Measured on MI355X, worst error / bound (every test prints its figures with -s): scale and shift 0.090 at most (B 256); the metrics 0.141
(negative aligned), 0.126 (exact thresholds), 0.11 and below elsewhere -- the figures of the CPU emulation with contraction; IoU bitwise on every case.  No
kernel was found wrong."""
import numpy as np
import pytest
import torch

from oracle import metrics_ref as MR
from tests import metrics_refs as R
from tests.golden_inputs import metrics_inputs
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu


def test_depth_and_iou_metrics_match_oracle(gpu_device, golden_dir):
    from soccdpt_amd.utils.metrics import DEPTH_KEYS, depth_metrics, iou_metric
    g = np.load(f"{golden_dir}/metrics.npz")
    pred, gt, mask, seg_pred, seg_gt = metrics_inputs(int(g["seed"]))
    m = depth_metrics(pred.to(gpu_device), gt.to(gpu_device), mask.to(gpu_device))
    got = np.array([float(m[k]) for k in DEPTH_KEYS])
    np.testing.assert_allclose(got, g["depth"], rtol=2e-4)          # f32 sums on the CPU vs f64 block sums here
    np.testing.assert_allclose(m["scale"].cpu().numpy(), g["scale"], rtol=2e-4)
    np.testing.assert_allclose(m["shift"].cpu().numpy(), g["shift"], rtol=2e-3, atol=1e-6)
    np.testing.assert_allclose(iou_metric(seg_pred.to(gpu_device), seg_gt.to(gpu_device)).cpu().numpy(), g["iou"], rtol=1e-6)


def test_metrics_full_resolution_and_edge_cases(gpu_device):
    from soccdpt_amd.utils.metrics import DEPTH_KEYS, depth_metrics, iou_metric
    pred, gt, mask, seg_pred, seg_gt = metrics_inputs(seed=5, B=2, H=1080, W=1920)   # camera resolution
    m = depth_metrics(pred.to(gpu_device), gt.to(gpu_device), mask.to(gpu_device))
    ref = MR.depth_metrics_batch(pred, gt, mask)
    np.testing.assert_allclose(np.array([float(m[k]) for k in DEPTH_KEYS]), np.array(ref[:7], dtype=np.float64), rtol=5e-4)
    np.testing.assert_allclose(iou_metric(seg_pred.to(gpu_device), seg_gt.to(gpu_device)).cpu().numpy(), MR.iou_batch(seg_pred, seg_gt), rtol=1e-6)
    # empty mask -> zeros (the reference maps NaN/inf to 0); empty union -> IoU 0
    z = depth_metrics(pred.to(gpu_device), gt.to(gpu_device), torch.zeros_like(mask).to(gpu_device))
    assert all(float(z[k]) == 0.0 for k in DEPTH_KEYS) and float(z["scale"].abs().sum()) == 0.0
    assert float(iou_metric(torch.zeros(1, 3, 8, 8, device=gpu_device), torch.zeros(1, 3, 8, 8, device=gpu_device))[0]) == 0.0


# ---------------- one call at a time against tests/metrics_refs.py ----------------
MEASURED = {}


@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after {what}: {e}", returncode=3)


def _scratch(B, C, dev):
    from soccdpt_amd.lib import load_library
    n = int(load_library().soccdpt_metrics_scratch_bytes(B, C))
    assert n == (B * 5 + 8) * 8 + B * C * 16
    return Buf((n,), torch.uint8, dev)


def _operands(dev, **host):
    bufs = {k: Buf(t.shape, t.dtype, dev, t) for k, t in host.items()}
    return bufs


def _untouched(bufs, host, scratch, out, what):
    for k, b in bufs.items():
        assert b.guard_untouched(), f"{what}: the guard behind {k} was written"
        assert torch.equal(_bits(b.t.cpu()), _bits(host[k])), f"{what}: operand {k} was written"
    assert scratch.guard_untouched(), f"{what}: the guard behind the scratch was written"
    assert out.guard_untouched(), f"{what}: the guard behind the output was written"


def run_depth(pred, gt, mask, dev, scratch=None, expect_launches=3):
    from soccdpt_amd.lib import _call, load_library
    L = load_library()
    B, npix = pred.shape
    host = dict(pred=pred, gt=gt, mask=mask)
    bufs = _operands(dev, **host)
    out = Buf((7 + 2 * B,), torch.float32, dev)
    scratch = scratch or _scratch(B, 1, dev)
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    _call("soccdpt_metrics_depth", bufs["pred"].ptr(), bufs["gt"].ptr(), bufs["mask"].ptr(), B, npix, out.ptr(), scratch.ptr(), device=dev)
    _sync(f"soccdpt_metrics_depth (B {B}, npix {npix})")
    assert int(L.soccdpt_launch_counter()) - before == expect_launches
    _untouched(bufs, host, scratch, out, f"depth B {B} npix {npix}")
    return out.t.cpu()


def run_iou(pred, gt, dev, scratch=None):
    from soccdpt_amd.lib import _call
    B, C, npix = pred.shape
    host = dict(pred=pred, gt=gt)
    bufs = _operands(dev, **host)
    out = Buf((B,), torch.float32, dev)
    scratch = scratch or _scratch(B, C, dev)
    _call("soccdpt_metrics_iou", bufs["pred"].ptr(), bufs["gt"].ptr(), B, C, npix, out.ptr(), scratch.ptr(), device=dev)
    _sync(f"soccdpt_metrics_iou (B {B}, C {C}, npix {npix})")
    _untouched(bufs, host, scratch, out, f"iou B {B} C {C} npix {npix}")
    return out.t.cpu()


@pytest.mark.parametrize("case", R.DEPTH_CASES)
def test_depth_metrics_case(dev, case):
    p, g, m = R.depth_case(case)
    out = run_depth(p, g, m, dev)
    again = run_depth(p, g, m, dev)
    assert torch.equal(_bits(out), _bits(again)), f"{case}: two calls differ"
    a, b = R.check_depth(out, p, g, m, case)
    MEASURED[case] = (a, b)
    print(f"MEASURED {case}: scale/shift {a:.3f}, metrics {b:.3f} of the bound; out {out[:9].tolist()}")
    pp, pg = R.poison(p, g, m)
    assert torch.equal(_bits(run_depth(pp, pg, m, dev)), _bits(out)), f"{case}: NaN / inf at masked-out pixels changed the result"
    if case == "exact thresholds":
        assert float(out[7]) == 1.0 and float(out[8]) == 0.0 and float(out[4]) == 0.0
    if case in ("all empty", "npix 1"):
        assert bool((out[7:] == 0).all())
    if case == "nan under the mask":
        assert bool((out[:7] == 0).all()) and bool(torch.isnan(out[7:]).all())


@pytest.mark.parametrize("case", list(R.IOU_CASES))
def test_iou_case(dev, case):
    p, t = R.iou_case(case)
    out = run_iou(p, t, dev)
    assert torch.equal(_bits(out), _bits(run_iou(p, t, dev))), f"{case}: two calls differ"
    ref = R.ref_iou(p, t)
    same = out.view(torch.int32) == ref.view(torch.int32)
    assert bool(same.all()), f"{case}: {int((~same).sum())} of {len(ref)} images differ; first {int((~same).nonzero()[0])}: {out[~same][0]!r} vs {ref[~same][0]!r}"
    for d in R.IOU_DEFECTS:
        if not torch.equal(R.ref_iou(p, t, defect=d).view(torch.int32), ref.view(torch.int32)):
            assert not torch.equal(out.view(torch.int32), R.ref_iou(p, t, defect=d).view(torch.int32))


def test_depth_and_iou_share_an_exact_scratch(dev):
    """Depth and IoU calls back to back on one scratch buffer of exactly soccdpt_metrics_scratch_bytes(B, C) bytes: the IoU counts live behind the depth sums."""
    B, C, npix = 5, 3, 300
    p, g, m = R.healthy(B, npix, 11)
    gen = torch.Generator().manual_seed(12)
    sp, st = torch.rand(B, C, npix, generator=gen), torch.rand(B, C, npix, generator=gen)
    scratch = _scratch(B, C, dev)
    d1 = run_depth(p, g, m, dev, scratch)
    i1 = run_iou(sp, st, dev, scratch)
    d2 = run_depth(p, g, m, dev, scratch)
    i2 = run_iou(sp, st, dev, scratch)
    assert torch.equal(_bits(d1), _bits(d2)) and torch.equal(_bits(i1), _bits(i2))
    R.check_depth(d1, p, g, m, "shared scratch")
    assert torch.equal(i1.view(torch.int32), R.ref_iou(sp, st).view(torch.int32))
    assert torch.equal(_bits(d1), _bits(run_depth(p, g, m, dev))) and torch.equal(_bits(i1), _bits(run_iou(sp, st, dev)))


def test_metrics_refusals_write_nothing(dev):
    from soccdpt_amd.lib import load_library
    L = load_library()
    arena = Buf((8, 4096), torch.uint8, dev)                  # 0xFF; every pointer of the refused calls points into it
    P = lambda r: arena.ptr() + 4096 * r
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    depth = {
        "B 257": (P(0), P(1), P(2), R.MAX_B + 1, 4, P(3), P(4)),
        "B 0": (P(0), P(1), P(2), 0, 4, P(3), P(4)),
        "B -1": (P(0), P(1), P(2), -1, 4, P(3), P(4)),
        "npix 0": (P(0), P(1), P(2), 1, 0, P(3), P(4)),
        "null pred": (None, P(1), P(2), 1, 4, P(3), P(4)),
        "null gt": (P(0), None, P(2), 1, 4, P(3), P(4)),
        "null mask": (P(0), P(1), None, 1, 4, P(3), P(4)),
        "null out": (P(0), P(1), P(2), 1, 4, None, P(4)),
        "null scratch": (P(0), P(1), P(2), 1, 4, P(3), None),
    }
    iou = {
        "B 0": (P(0), P(1), 0, 1, 4, P(3), P(4)),
        "C 0": (P(0), P(1), 1, 0, 4, P(3), P(4)),
        "C -1": (P(0), P(1), 1, -1, 4, P(3), P(4)),
        "npix 0": (P(0), P(1), 1, 1, 0, P(3), P(4)),
        "null pred": (None, P(1), 1, 1, 4, P(3), P(4)),
        "null gt": (P(0), None, 1, 1, 4, P(3), P(4)),
        "null out": (P(0), P(1), 1, 1, 4, None, P(4)),
        "null scratch": (P(0), P(1), 1, 1, 4, P(3), None),
    }
    for fn, table in ((L.soccdpt_metrics_depth, depth), (L.soccdpt_metrics_iou, iou)):
        for label, args in table.items():
            assert fn(*args, None) == 1, f"accepted: {label}"
            torch.cuda.synchronize()
            assert int(L.soccdpt_launch_counter()) == before, f"{label}: a refused call launched a kernel"
            assert bool((arena.raw == 0xFF).all()), f"{label}: a refused call wrote"


def test_metrics_measured_table():
    print()
    for case, (a, b) in MEASURED.items():
        print(f"TABLE {case:<24} scale/shift {a:.3f}  metrics {b:.3f}")
