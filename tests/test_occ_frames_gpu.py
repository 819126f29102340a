"""GPU: per-frame semantic occupancy grids (csrc/occ_frames.hip, soccdpt_voxelise_frames / soccdpt_occ_expand_frames / soccdpt_forward_frames,
SOccDPT(occupancy_per_frame=True)) against the C oracle run on ONE FRAME AT A TIME: row b must be, word for word, what the reference computes when
frame b is handed to it as a batch of one."""
import os
import tempfile

import numpy as np
import pytest
import torch

from oracle import cref, soccdpt_ref as R
from tests.golden_inputs import proj_inputs

pytestmark = pytest.mark.gpu

GRID = (256, 256, 32)


def _engine(dev, cam=R.Camera()):
    from soccdpt_amd.lib import Engine, make_config
    cfg = R.ProjConfig()
    c = make_config("swin2t16_256", 3, 256, False, True, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                    cfg.grid_size, cfg.occupancy_shape(), cfg.pc_scale, cfg.pc_shift, cfg.correction_angle)
    return Engine(c, dev)


def _np(bits):
    return bits.cpu().numpy().view(np.uint32)


def _project_and_frames(eng, inv, seg, dev, cam=R.Camera(), fill=-1):
    """eng.project (inv_up + union bits) followed by eng.voxelise_frames into a buffer pre-filled with `fill`."""
    B = inv.shape[0]
    inv_d, seg_d = inv.to(dev), seg.to(dev)
    inv_up = torch.empty((B, cam.height, cam.width), device=dev)
    union = torch.full((eng.occ_words(),), -1, dtype=torch.int32, device=dev)
    eng.project(inv_d, seg_d, inv_up, None, None, union, clear_bits=True)
    rows = torch.full((B, eng.occ_words()), fill, dtype=torch.int32, device=dev)
    eng.voxelise_frames(inv_up, seg_d, rows, clear_bits=True)
    torch.cuda.synchronize()
    return inv_up, seg_d, union, rows


def _oracle_rows(inv, seg, cam=R.Camera()):
    return np.stack([cref.project(inv[b:b + 1], seg[b:b + 1], cam=cam, want=("occ_bits",))["occ_bits"] for b in range(inv.shape[0])])


def _check_rows(eng, inv, seg, dev, cam=R.Camera()):
    _, _, union, rows = _project_and_frames(eng, inv, seg, dev, cam)
    want = _oracle_rows(inv, seg, cam)
    got = _np(rows)
    for b in range(inv.shape[0]):
        assert np.array_equal(got[b], want[b]), f"frame {b}: {int((got[b] != want[b]).sum())} words differ from the single-frame oracle"
    assert np.array_equal(np.bitwise_or.reduce(got, axis=0), _np(union))     # OR of the rows == the fused kernel's union
    return got, want, _np(union)


def _popcount(words):
    return int(np.unpackbits(words.view(np.uint8)).sum())


def test_rows_bit_exact_b8(gpu_device):
    eng = _engine(gpu_device)
    inv, seg = proj_inputs(seed=21, B=8)
    got, want, union = _check_rows(eng, inv, seg, gpu_device)
    # the inputs are not trivial: every frame is non-empty, the rows differ from each other and no row is the union
    counts = [_popcount(got[b]) for b in range(8)]
    assert min(counts) > 1000 and _popcount(union) > max(counts)
    assert all(not np.array_equal(got[b], union) for b in range(8))
    assert all(not np.array_equal(got[a], got[b]) for a in range(8) for b in range(a + 1, 8))


def test_rows_bit_exact_golden_seed(gpu_device, golden_dir):
    eng = _engine(gpu_device)
    g = np.load(f"{golden_dir}/projection_B2.npz")
    inv, seg = proj_inputs(int(g["seed"]))
    got, _, union = _check_rows(eng, inv, seg, gpu_device)
    assert np.array_equal(union, g["occ_bits"])                              # ... which is the reference's own output for this batch


@pytest.mark.parametrize("size", [(1918, 1080), (998, 540), (1280, 722)])
def test_rows_bit_exact_other_cameras(gpu_device, size):
    """width % 4 != 0 takes the kernel's scalar-load form (one and two row segments, partly filled last threads); 1280 x 722 is the vector form with
    a camera height that is not a multiple of the rows per workgroup."""
    cam = R.Camera(fx=1250.6 * size[0] / 1920.0, fy=1254.8 * size[1] / 1080.0, cx=978.4 * size[0] / 1920.0, cy=562.1 * size[1] / 1080.0,
                   width=size[0], height=size[1])
    eng = _engine(gpu_device, cam)
    inv, seg = proj_inputs(seed=33, B=3)
    got, _, _ = _check_rows(eng, inv, seg, gpu_device, cam)
    assert all(_popcount(got[b]) > 100 for b in range(3))


@pytest.mark.parametrize("fill", [float("nan"), 0.0, float("inf"), -1.0])
def test_degenerate_frame_is_isolated(gpu_device, fill):
    eng = _engine(gpu_device)
    inv, seg = proj_inputs(seed=7, B=3)
    inv[1] = fill
    got, want, _ = _check_rows(eng, inv, seg, gpu_device)
    assert not got[1].any() and got[0].any() and got[2].any()


def test_all_zero_seg_frame_is_empty(gpu_device):
    eng = _engine(gpu_device)
    inv, seg = proj_inputs(seed=8, B=3)
    seg[2] = 0.0
    got, _, _ = _check_rows(eng, inv, seg, gpu_device)
    assert not got[2].any() and got[0].any() and got[1].any()


def test_buffer_contract(gpu_device):
    eng = _engine(gpu_device)
    inv, seg = proj_inputs(seed=5, B=2)
    inv_up, seg_d, union, rows = _project_and_frames(eng, inv, seg, gpu_device, fill=-1)   # pre-filled with -1, cleared by clear_bits=1
    want = _oracle_rows(inv, seg)
    assert np.array_equal(_np(rows), want)
    before = _np(rows).copy()
    eng.voxelise_frames(inv_up, seg_d, rows, clear_bits=False)                              # ORs the same bits again: nothing changes
    torch.cuda.synchronize()
    assert np.array_equal(_np(rows), before)
    stale = torch.full_like(rows, 0x00010000)
    eng.voxelise_frames(inv_up, seg_d, stale, clear_bits=False)                             # ... and really does OR into what is there
    torch.cuda.synchronize()
    assert np.array_equal(_np(stale), before | np.uint32(0x00010000))
    # B = 1: the row is the union
    inv1, seg1 = proj_inputs(seed=5, B=1)
    _, _, union1, rows1 = _project_and_frames(eng, inv1, seg1, gpu_device)
    assert np.array_equal(_np(rows1)[0], _np(union1)) and _np(union1).any()


def test_entry_point_errors(gpu_device):
    eng = _engine(gpu_device)
    inv_up = torch.full((1, 1080, 1920), 0.1, device=gpu_device)
    seg = torch.ones((1, 3, 256, 256), device=gpu_device)
    rows = torch.zeros((1, eng.occ_words()), dtype=torch.int32, device=gpu_device)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    L, h = eng.L, eng._h
    assert L.soccdpt_voxelise_frames(h, None, seg.data_ptr(), 1, 256, 256, rows.data_ptr(), 1, st) != 0
    assert b"soccdpt_voxelise_frames" in L.soccdpt_last_error(h)
    assert L.soccdpt_voxelise_frames(h, inv_up.data_ptr(), seg.data_ptr(), 0, 256, 256, rows.data_ptr(), 1, st) != 0
    assert L.soccdpt_occ_expand_frames(h, rows.data_ptr(), 0, inv_up.data_ptr(), st) != 0
    assert L.soccdpt_occ_expand_frames(h, None, 1, inv_up.data_ptr(), st) != 0
    assert b"soccdpt_occ_expand_frames" in L.soccdpt_last_error(h)
    # soccdpt_forward_frames: null inv_up / frame bits, empty batch, workspace too small
    x = torch.zeros((1, 3, 256, 256), device=gpu_device)
    ws = torch.empty(64, dtype=torch.uint8, device=gpu_device)
    assert L.soccdpt_forward_frames(h, x.data_ptr(), 1, None, None, None, None, None, rows.data_ptr(), ws.data_ptr(), ws.numel(), st) != 0
    assert b"dev_inv_up" in L.soccdpt_last_error(h)
    assert L.soccdpt_forward_frames(h, x.data_ptr(), 1, inv_up.data_ptr(), None, None, None, None, None, ws.data_ptr(), ws.numel(), st) != 0
    assert b"dev_frame_bits" in L.soccdpt_last_error(h)
    assert L.soccdpt_forward_frames(h, x.data_ptr(), 0, inv_up.data_ptr(), None, None, None, None, rows.data_ptr(), ws.data_ptr(), ws.numel(), st) != 0
    assert L.soccdpt_forward_frames(h, x.data_ptr(), 1, inv_up.data_ptr(), None, None, None, None, rows.data_ptr(), ws.data_ptr(), ws.numel(), st) != 0
    assert b"workspace too small" in L.soccdpt_last_error(h)
    torch.cuda.synchronize()


def _dense(words):
    return np.unpackbits(words.view(np.uint8), bitorder="little").astype(np.float32).reshape(GRID + (3,))


def test_occ_expand_frames(gpu_device):
    eng = _engine(gpu_device)
    inv, seg = proj_inputs(seed=21, B=8)
    _, _, _, rows = _project_and_frames(eng, inv, seg, gpu_device)
    occ = torch.full((8,) + GRID + (3,), 7.0, device=gpu_device)
    eng.occ_expand_frames(rows, 8, occ)
    torch.cuda.synchronize()
    got = _np(rows)
    for b in range(8):
        o = occ[b].cpu().numpy()
        assert np.array_equal(o, _dense(got[b]))
        assert set(np.unique(o).tolist()) == {0.0, 1.0}
    # random words, every bit position
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, eng.occ_words()), dtype=torch.int32, generator=torch.Generator().manual_seed(3)).to(gpu_device)
    occ2 = torch.empty((2,) + GRID + (3,), device=gpu_device)
    eng.occ_expand_frames(rnd, 2, occ2)
    torch.cuda.synchronize()
    for b in range(2):
        assert np.array_equal(occ2[b].cpu().numpy(), _dense(_np(rnd)[b]))


# ---- whole model ----
@pytest.fixture(scope="module")
def nets(gpu_device):
    """(per-frame, union) models on the same synthetic weights and calibration file, as smoke() builds them."""
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    sd = synth_state_dict(alias_pretrained=True)
    out = []
    for per_frame in (True, False):
        m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=per_frame)
        m.load_state_dict(sd, strict=False)
        out.append(m.eval().to(gpu_device))
    return out


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _check_model_rows(net, occ, inv256, seg256):
    """occ rows, last_occ_frame_bits and last_occ_bits of `net` against the single-frame oracle on the network-resolution outputs."""
    B = inv256.shape[0]
    want = _oracle_rows(inv256.cpu(), seg256.cpu())
    rows = net.last_occ_frame_bits
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (B, want.shape[1])
    assert tuple(occ.shape) == (B,) + GRID + (3,)
    for b in range(B):
        assert np.array_equal(_np(rows)[b], want[b])
        assert np.array_equal(occ[b].cpu().numpy(), _dense(want[b]))
    assert np.array_equal(_np(net.last_occ_bits), np.bitwise_or.reduce(want, axis=0))
    return want


def test_whole_model_b4(gpu_device, nets):
    from soccdpt_amd.utils.synth import synth_input
    per, uni = nets
    x = synth_input(4, seed0=60).to(gpu_device)
    inv_p, seg_p, pts_p, occ_p = per(x)
    inv_u, seg_u, pts_u, occ_u = uni(x)
    inv256, seg256 = per.network(x)
    torch.cuda.synchronize()
    assert _same(inv_p, inv_u) and _same(seg_p, seg_u) and _same(pts_p, pts_u)
    assert torch.equal(per.last_occ_bits, uni.last_occ_bits) and per.last_occ_bits.dtype == torch.int32
    want = _check_model_rows(per, occ_p, inv256, seg256)
    # the frames really differ, and the default model still returns the union in every row
    assert all(not np.array_equal(want[b], _np(uni.last_occ_bits)) for b in range(4))
    union_dense = _dense(_np(uni.last_occ_bits))
    for b in range(4):
        assert np.array_equal(occ_u[b].cpu().numpy(), union_dense)
    assert getattr(uni, "last_occ_frame_bits", None) is None
    # the union also equals the fused kernel's on the same network outputs (what soccdpt_forward writes)
    ref = cref.project(inv256.cpu(), seg256.cpu(), want=("occ_bits",))
    assert np.array_equal(_np(per.last_occ_bits), ref["occ_bits"])


def test_get_semantic_occupancy_per_frame(gpu_device, nets):
    per, uni = nets
    inv, seg = proj_inputs(seed=21, B=4)
    out_p = per.get_semantic_occupancy(inv.to(gpu_device), seg.to(gpu_device))
    rows = per.last_occ_frame_bits.clone()
    out_u = uni.get_semantic_occupancy(inv.to(gpu_device), seg.to(gpu_device))
    torch.cuda.synchronize()
    for a, b in zip(out_p[:3], out_u[:3]):
        assert _same(a, b)
    _check_model_rows(per, out_p[3], inv, seg)
    assert torch.equal(per.last_occ_bits, uni.last_occ_bits)
    union_dense = _dense(_np(uni.last_occ_bits))
    assert all(np.array_equal(out_u[3][b].cpu().numpy(), union_dense) for b in range(4))
    assert not torch.equal(rows[0], rows[1])


def test_train_mode_per_frame(gpu_device):
    """net.train(): occupancy goes through _forward_train -> get_semantic_occupancy (no_grad) or the autograd node; it carries no gradient."""
    from soccdpt_amd.lib import PREC_F32
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    net = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True, precision=PREC_F32)
    net.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    net = net.to(gpu_device).train()
    seen = {}
    orig = net.train_forward

    def spy(x, seed=None):
        seen["out"] = orig(x, seed)
        return seen["out"]
    net.train_forward = spy
    x = synth_input(2, seed0=70).to(gpu_device)
    with torch.no_grad():
        _, _, _, occ = net(x)
    torch.cuda.synchronize()
    _check_model_rows(net, occ, *seen["out"])
    out = net(x)                       # autograd-tracked tuple
    torch.cuda.synchronize()
    assert out[0].requires_grad and not out[3].requires_grad
    _check_model_rows(net, out[3], *seen["out"])


def test_consumers(gpu_device, nets):
    from soccdpt_amd.utils.metrics import evaluate_occupancy
    from soccdpt_amd.utils.occupancy import occupancy_grid_to_points, occupancy_iou
    from soccdpt_amd.utils.synth import synth_input
    per, uni = nets
    x = synth_input(4, seed0=60).to(gpu_device)
    inv, seg, _, occ = per(x)
    rows = per.last_occ_frame_bits
    for b in range(4):
        a = per.occupancy_points(frame=b)
        assert a.dtype == torch.float64 and a.shape[0] > 0 and torch.equal(a, occupancy_grid_to_points(occ[b]))
    assert torch.equal(per.occupancy_points(), occupancy_grid_to_points((occ.sum(dim=0) > 0).float()))   # frame=None: the union, as before
    uni(x)
    with pytest.raises(RuntimeError):
        uni.occupancy_points(frame=0)
    rng = np.random.default_rng(4)
    flip = torch.from_numpy(rng.random((4,) + GRID + (3,)) < 1e-4).to(gpu_device)
    gt = (occ >= 0.5) ^ flip
    res = occupancy_iou(rows, gt, 3)
    assert tuple(res["iou_3D"].shape) == (4,)
    for b in range(4):
        one = occupancy_iou(rows[b], gt[b:b + 1], 3)
        assert float(res["iou_3D"][b]) == float(one["iou_3D"][0]) and 0.0 < float(one["iou_3D"][0]) < 1.0
        assert torch.equal(res["counts"][b], one["counts"][0])
    # utils.metrics.evaluate_occupancy takes the multi-row prediction as it is
    class Rec:
        def log(self, d):
            self.d = d
    x_raw = torch.zeros((4, per.height, per.width, 3), dtype=torch.uint8)
    out = evaluate_occupancy(per, None, gpu_device, False, x_raw, gt, occ, inv, seg, {0: (255, 0, 0), 1: (0, 255, 0), 2: (0, 0, 255)},
                             torch.tensor(0.5), 1e-4, 1, 1, Rec())
    assert out["iou_3D"] == float(res["iou_3D"].mean().item())


def test_eval_script_per_frame_flag(gpu_device, capsys):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    base = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", "/nonexistent"]
    r1 = main(build_parser().parse_args(base + ["--occupancy-per-frame"]))
    out = capsys.readouterr().out
    for line in ("IOU_3D:", "OCC_POINTS:"):
        assert line in out
    r0 = main(build_parser().parse_args(base + ["--occupancy"]))
    # the script's synthetic validation set has batch size 1: a frame's own grid is the union
    assert r1["iou_3D"] == r0["iou_3D"] and r1["occ_points"] == r0["occ_points"] and r1["occ_points"] > 0
