"""GPU: dpt_swin_large_384 (Swin-V1-L encoder, 384 x 384) through the C ABI against the CPU statement on the same synthetic weights and frame.

The statement (tests/swin1_large_refs.py: the Swin-V1 encoder in torch on top of oracle/soccdpt_ref.py's decoder and heads, fp32 on the CPU) gives (inv, seg)
for the one frame, computed once per module.  Bars: f32 and f16x3 within the north star's 1e-3 (relative L2), f16x3 also within the 1e-4 dpt_swin2_base_384 and dpt_swin_large_384 hold,
the default arithmetic (SOCCDPT_PREC_MIXED) within its 5e-4 budget -- there is no shipped precision map for this model, so an uncalibrated handle runs every
group in x3.  fp16 and bf16 are regression pins at twice the error measured when the model was added (MEASURED below)."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import swin1_large_refs as L

pytestmark = pytest.mark.gpu

# relative L2 vs the fp32 CPU statement measured on MI355X when the model was added: (inverse depth, sigmoid probabilities), B = 1, synth_input(1, 384, seed0=8)
MEASURED = {"f16": (2.26e-4, 1.19e-3), "bf16": (2.14e-3, 7.10e-3)}
# (same run: f32 3.9e-7 / 1.3e-6, f16x3 2.4e-7 / 8.9e-7, mixed uncalibrated = every group x3 with fp16 attention 7.5e-6 / 3.5e-5.  The probabilities carry the
#  synthetic head's x12 logit gain, as on the Swin-V2 models.)
# B = 2 against two B = 1 runs, fp16 operands: measured (inv, seg); a different tile or split-K changes which fp16 roundings flip.  The bound is twice the measured
# pair, recorded like the pins above (dpt_swin2_base_384's own bounds, 4e-4 / 1.2e-3, would hold here too).
MEASURED_B_INVARIANCE = (1.50e-4, 4.53e-4)      # frame 0; frame 1: 1.51e-4 / 4.20e-4
# net.calibrate_precision on six frames: 3.4 s, 277 forwards, 49 groups x3 + 16 x2w of 114, worst quantity 4.25e-4 (calibration frames) / 4.27e-4 (hold-out); fp16 everywhere 1.24e-3
CALIBRATION_SECONDS = 3.4


REFUSAL = r"no training step is built for dpt_swin_large_384 \(Swin-V1-L\)"


def _rel_l2(a, b):
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope="module")
def ref():
    """State dict, one frame and the oracle's (inv, seg) for it, computed once and left unchanged."""
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict
    sd = synth_state_dict(L.BACKBONE, alias_pretrained=True)
    x = synth_input(1, size=384, seed0=8)
    torch.set_num_threads(16)
    with torch.no_grad():
        o_inv, o_seg, _ = L.network(sd, x, sigmoid=True)
    return sd, x, o_inv, o_seg


def _build(sd, precision, dev):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(sigmoid=True, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, model_type=L.MODEL_TYPE, precision=precision)
    r = m.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys
    return m.eval().to(dev)


@pytest.fixture(scope="module")
def mixed(ref, gpu_device):
    from soccdpt_amd.lib import PREC_MIXED
    return _build(ref[0], PREC_MIXED, gpu_device)


@pytest.mark.parametrize("precision", ["f32", "f16x3", "f16", "bf16"])
def test_network_vs_oracle(ref, gpu_device, precision):
    from soccdpt_amd.lib import PREC_BF16, PREC_F16, PREC_F16X3, PREC_F32
    sd, x, o_inv, o_seg = ref
    m = _build(sd, {"f32": PREC_F32, "f16": PREC_F16, "bf16": PREC_BF16, "f16x3": PREC_F16X3}[precision], gpu_device)
    inv, seg = m.network(x.to(gpu_device))
    torch.cuda.synchronize()
    assert tuple(inv.shape) == (1, 384, 384) and tuple(seg.shape) == (1, 3, 384, 384)
    assert bool(torch.isfinite(inv).all()) and bool(torch.isfinite(seg).all())
    e_inv, e_seg = _rel_l2(inv.cpu(), o_inv), _rel_l2(seg.cpu(), o_seg)
    print(f"swin_large_384 {precision}: rel L2 inv {e_inv:.2e} seg {e_seg:.2e}")
    if precision in ("f32", "f16x3"):
        assert e_inv < 1e-3 and e_seg < 1e-3          # the north star
    if precision == "f16x3":
        assert e_inv < 1e-4 and e_seg < 1e-4          # split-operand fp16 is f32-grade: the bar dpt_swin2_base_384 holds
    if precision in MEASURED:
        m_inv, m_seg = MEASURED[precision]
        assert e_inv <= 2 * m_inv and e_seg <= 2 * m_seg, (e_inv, e_seg, MEASURED[precision])


def test_mixed_uncalibrated_runs_x3_within_its_budget(ref, mixed, gpu_device):
    """No shipped map: the handle says so and every group runs x3 until a calibration has run."""
    sd, x, o_inv, o_seg = ref
    inv, seg = mixed.network(x.to(gpu_device))
    torch.cuda.synchronize()
    assert mixed.precision_map_source() == "uncalibrated-all-x3"
    e_inv, e_seg = _rel_l2(inv.cpu(), o_inv), _rel_l2(seg.cpu(), o_seg)
    print(f"swin_large_384 mixed (uncalibrated): rel L2 inv {e_inv:.2e} seg {e_seg:.2e}")
    assert e_inv < 5e-4 and e_seg < 5e-4


def test_full_forward_grid_and_projection_bit_exact(ref, mixed, gpu_device):
    from oracle import cref
    x = ref[1].to(gpu_device)
    inv_up, seg_up, pts, occ = mixed(x)
    torch.cuda.synchronize()
    assert tuple(occ.shape) == (1, 256, 256, 32, 3) and tuple(inv_up.shape) == (1, 1080, 1920) and tuple(seg_up.shape) == (3, 1080, 1920)
    assert int(occ.sum().item()) > 0
    # the projection stage on the network's own output, against the C oracle
    inv, seg = mixed.network(x)
    out = mixed.get_semantic_occupancy(inv, seg)
    torch.cuda.synchronize()
    want = cref.project(inv.cpu(), seg.cpu())
    assert np.array_equal(mixed.last_occ_bits.cpu().numpy().view(np.uint32), want["occ_bits"])
    assert np.array_equal(np.nan_to_num(out[2].cpu().numpy(), nan=-7), np.nan_to_num(want["points"], nan=-7))


def test_batch_of_two_matches_single_frames(ref, gpu_device):
    """Frames are independent through the network; B = 2 picks other tiles / split-K than B = 1, so only round-off may differ.  fp16 operands, as in
    test_swin2_base_384_B8_vs_oracle, and its margin."""
    from soccdpt_amd.lib import PREC_F16
    from soccdpt_amd.utils.synth import synth_input
    m = _build(ref[0], PREC_F16, gpu_device)
    x = synth_input(2, size=384, seed0=40).to(gpu_device)
    inv2, seg2 = m.network(x)
    inv2, seg2 = inv2.clone(), seg2.clone()
    singles = [m.network(x[i:i + 1]) for i in range(2)]
    torch.cuda.synchronize()
    errs = [(_rel_l2(inv2[i:i + 1], inv1), _rel_l2(seg2[i:i + 1], seg1)) for i, (inv1, seg1) in enumerate(singles)]
    for i, (e_inv, e_seg) in enumerate(errs):
        print(f"swin_large_384 f16 frame {i}: B = 2 vs B = 1 rel L2 inv {e_inv:.2e} seg {e_seg:.2e}")
    for e_inv, e_seg in errs:
        assert e_inv <= 2 * MEASURED_B_INVARIANCE[0] and e_seg <= 2 * MEASURED_B_INVARIANCE[1], errs


def test_training_is_refused(ref, mixed, gpu_device):
    """net.train(); net(x): the refusal that names this model -- from the Python mirror, and from the library itself on a SOCCDPT_PREC_F32 handle (what a
    caller of the C ABI meets; its training workspace has size 0)."""
    from soccdpt_amd.lib import PREC_F32, Engine, make_config
    x = ref[1].to(gpu_device)
    mixed.train()
    try:
        with pytest.raises(RuntimeError, match=REFUSAL):
            mixed(x)
    finally:
        mixed.eval()
    cfg = make_config(L.BACKBONE, 3, 256, True, False, 1920, 1080, 1250.6, 1254.8, 978.4, 562.1, (256, 256, 32), (128.0, 128.0, 48.0), (10000.0, 50000.0, 800.0),
                      (55.0, -20.0, 15.0), (7.0, 0, 0), precision=PREC_F32)
    eng = Engine(cfg, gpu_device)
    inv = torch.empty((1, 384, 384), device=gpu_device)
    seg = torch.empty((1, 3, 384, 384), device=gpu_device)
    assert eng.L.soccdpt_train_workspace_bytes(eng._h, 1) == 0
    with pytest.raises(RuntimeError, match=REFUSAL):
        eng.train_forward(x, inv, seg)


def test_eval_script_runs_the_model(gpu_device, capsys):
    """eval_SOccDPT -t dpt_swin_large_384 -d cuda:0 on synthetic weights and the synthetic validation subset (fp16 operands: -o)."""
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    r = main(build_parser().parse_args(["-v", "3", "-dt", "bdd", "-t", L.MODEL_TYPE, "-d", "cuda:0", "-b", "/nonexistent", "-o"]))
    out = capsys.readouterr().out
    for line in ("Model: SOccDPT_V3_dpt_swin_large_384", "FPS:", "IOU:", "ABS_REL:", "RMSE:", "A3:"):
        assert line in out
    assert r["fps"] > 10 and 0.0 < r["iou"] <= 1.0 and r["rmse"] > 0


def test_calibration_derives_a_map_within_the_budget(ref, mixed, gpu_device):
    """net.calibrate_precision on six synthetic frames (four select, two hold out): the verify error of the derived map is inside the budget and the handle
    says "calibrated".  Last in the module: it changes the `mixed` handle's map.  Measured when the model was added: see CALIBRATION_SECONDS."""
    import time
    from soccdpt_amd.utils.synth import synth_input
    frames = synth_input(6, size=384, seed0=200).to(gpu_device)
    assert mixed.precision_map_source() == "uncalibrated-all-x3"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = mixed.calibrate_precision(frames, budget=5e-4)
    torch.cuda.synchronize()
    print(f"swin_large_384 calibration: {time.perf_counter() - t0:.1f} s, report { {k: v for k, v in rep.items() if not isinstance(v, (bytes, str)) or len(v) < 80} }")
    assert mixed.precision_map_source() == "calibrated"
    assert max(rep["err_calibrated"].values()) <= 5e-4
    assert rep["err_holdout"] is not None and max(rep["err_holdout"].values()) <= 5e-4
    inv, seg = mixed.network(ref[1].to(gpu_device))
    torch.cuda.synchronize()
    assert _rel_l2(inv.cpu(), ref[2]) < 1e-3 and bool(torch.isfinite(seg).all())
