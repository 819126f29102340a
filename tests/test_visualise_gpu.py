"""GPU: the evaluation pictures (csrc/visualise.hip, soccdpt_amd/utils/visualise.py) against the numpy specification of tests/visualise_refs.py and the
reference's own color_segmentation (tests/golden/vis_color_segmentation.npz).  Every operation is integer or IEEE-exact f32, so every comparison is
byte for byte.  The kernel tests run twice: on the null stream and on a side stream with the result consumed on that stream."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import visualise_refs as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COLORS3 = {0: (255, 0, 0), 1: (0, 255, 0), 2: (0, 0, 255)}


@pytest.fixture(params=["null_stream", "side_stream"])
def on_stream(request, gpu_device):
    if request.param == "null_stream":
        yield None
        return
    s = torch.cuda.Stream(device=gpu_device)
    s.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(s):
        yield s
        s.synchronize()


def _same(got: torch.Tensor, want: np.ndarray):
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape, (g.dtype, g.shape, want.dtype, want.shape)
    assert g.tobytes() == np.ascontiguousarray(want).tobytes(), f"{int((g != want).sum())} bytes differ"


# ---- colourise ----
def _check_colorize(d: np.ndarray, dev):
    from soccdpt_amd.utils.visualise import colorize_disparity, disparity_minmax
    t = torch.from_numpy(d).to(dev)
    _same(colorize_disparity(t), R.colorize(d))
    frames = d if d.ndim == 3 else d[None]
    mm = disparity_minmax(t if d.ndim == 3 else t[None]).cpu().numpy()
    assert np.array_equal(mm, np.array([R.minmax(f) for f in frames], dtype=np.float32))


def test_colorize_frames_keep_their_own_range(gpu_device, on_stream):
    rng = np.random.default_rng(1)
    d = np.stack([rng.random((7, 13), dtype=np.float32) * 0.01 + 0.002, rng.random((7, 13), dtype=np.float32) * 300.0 - 150.0])
    _check_colorize(d, gpu_device)
    _check_colorize(d[1], gpu_device)                      # the [H,W] form
    assert R.colorize_index(d[0]).max() == 255 and R.colorize_index(d[1]).min() == 0


def test_colorize_extremes_in_the_last_two_elements(gpu_device, on_stream):
    d = np.random.default_rng(2).random((1, 64, 96), dtype=np.float32)
    d[0, -1, -2], d[0, -1, -1] = -3.5, 7.25
    _check_colorize(d, gpu_device)


def test_colorize_truncation_boundaries(gpu_device, on_stream):
    lo, hi = np.float32(0.125), np.float32(9.875)
    k = np.arange(256 * 3, dtype=np.float32) % 256
    d = (lo + k * ((hi - lo) / np.float32(255.0))).astype(np.float32).reshape(1, 24, 32)
    assert d.min() == lo
    _check_colorize(d, gpu_device)
    assert len(np.unique(R.colorize_index(d[0]))) > 200


def test_colorize_constant_frame_is_index_zero(gpu_device, on_stream):
    from soccdpt_amd.utils.visualise import colorize_disparity
    d = np.full((1, 5, 9), 3.25, dtype=np.float32)
    got = colorize_disparity(torch.from_numpy(d).to(gpu_device))
    _same(got, np.broadcast_to(R.LUT_BGR[0], (1, 5, 9, 3)).copy())
    _check_colorize(d, gpu_device)


def test_colorize_non_finite_pixels(gpu_device, on_stream):
    d = np.random.default_rng(3).random((1, 9, 14), dtype=np.float32) * 5.0 + 1.0
    d[0, 0, 0], d[0, 0, 1] = 0.5, 6.5                      # the extremes are elsewhere than the two pixels that turn non-finite
    clean = R.colorize(d)
    d2 = d.copy()
    d2[0, 2, 3], d2[0, 6, 13] = np.nan, np.inf
    want = clean.copy()
    want[0, 2, 3] = want[0, 6, 13] = R.LUT_BGR[0]
    assert np.array_equal(R.colorize(d2), want)            # the other pixels are not affected
    _check_colorize(d2, gpu_device)
    _check_colorize(np.full((1, 3, 5), np.nan, dtype=np.float32), gpu_device)     # no finite value at all


def test_colorize_camera_frame(gpu_device, on_stream):
    rng = np.random.default_rng(4)
    d = (rng.random((1, 1080, 1920), dtype=np.float32) * 0.08 + 0.001).astype(np.float32)
    _check_colorize(d, gpu_device)


# ---- class colours ----
@pytest.mark.parametrize("C", [3, 5])
def test_color_segmentation_reference_golden(gpu_device, on_stream, C):
    from soccdpt_amd.utils.visualise import color_masks, color_segmentation
    G = np.load(os.path.join(HERE, "golden", "vis_color_segmentation.npz"))
    masks, colors, want = G[f"c{C}_masks"], G[f"c{C}_colors"], G[f"c{C}_image"]
    c2c = {c: tuple(int(v) for v in colors[c]) for c in range(C)}
    assert np.array_equal(R.color_masks_hwc(masks, c2c), want)
    t = torch.from_numpy(masks).to(gpu_device)
    _same(color_segmentation(t, torch.empty((12, 16, 3), dtype=torch.uint8), c2c), want)
    _same(color_masks(t.permute(2, 0, 1).unsqueeze(0).contiguous(), c2c), want[None])


def test_color_masks_batched(gpu_device, on_stream):
    from soccdpt_amd.utils.visualise import color_masks
    rng = np.random.default_rng(5)
    seg = rng.random((2, 5, 9, 11), dtype=np.float32)
    colors = [tuple(int(v) for v in rng.integers(1, 256, 3)) for _ in range(5)]
    _same(color_masks(torch.from_numpy(seg).to(gpu_device), colors), R.color_masks(seg, colors))


def test_color_masks_nan_and_threshold_stay_black(gpu_device, on_stream):
    from soccdpt_amd.utils.visualise import color_masks
    seg = np.full((1, 3, 4, 6), 0.9, dtype=np.float32)
    seg[0, :, 1, 2] = np.nan
    seg[0, :, 3, 5] = 0.5
    got = color_masks(torch.from_numpy(seg).to(gpu_device), COLORS3)
    _same(got, R.color_masks(seg, COLORS3))
    g = got.cpu().numpy()
    assert not g[0, 1, 2].any() and not g[0, 3, 5].any() and tuple(g[0, 0, 0]) == COLORS3[2]


# ---- resize ----
@pytest.mark.parametrize("src,dst", [((6, 9), (12, 18)), ((9, 12), (6, 8)), ((7, 10), (7, 10)), ((1, 1), (3, 5)), ((7, 5), (4, 9))])
def test_resize(gpu_device, on_stream, src, dst):
    """(H, W) -> (H, W): 2x up, 3:2 down, identity, a 1 x 1 source, odd to odd."""
    from soccdpt_amd.utils.visualise import resize_bgr, resize_taps
    img = np.random.default_rng(6).integers(0, 256, size=src + (3,), dtype=np.uint8)
    assert np.array_equal(resize_taps(src[1], dst[1]), R.resize_taps(src[1], dst[1])) and np.array_equal(resize_taps(src[0], dst[0]), R.resize_taps(src[0], dst[0]))
    want = R.resize(img, (dst[1], dst[0]))
    _same(resize_bgr(torch.from_numpy(img).to(gpu_device), (dst[1], dst[0])), want)
    if src == dst:
        assert np.array_equal(want, img)
    both = np.stack([img, img[::-1, ::-1].copy()])
    _same(resize_bgr(torch.from_numpy(both).to(gpu_device), (dst[1], dst[0])), np.stack([R.resize(b, (dst[1], dst[0])) for b in both]))


def test_tiles_leave_the_rest_of_a_pitched_buffer_untouched(gpu_device, on_stream):
    """Resize, colourise and class colours into a sub-rectangle of a larger image whose row pitch is odd."""
    from soccdpt_amd.utils import visualise as V
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, size=(7, 5, 3), dtype=np.uint8)
    d = rng.random((4, 9), dtype=np.float32)
    seg = rng.random((3, 4, 9), dtype=np.float32)
    for fill, tile in (("resize", R.resize(img, (9, 4))), ("depth", R.colorize(d)), ("classes", R.color_masks(seg[None], COLORS3)[0])):
        panel = torch.full((11, 17, 3), 0xA5, dtype=torch.uint8, device=gpu_device)
        rect = V._Rect.tile(panel, 3, 5)
        if fill == "resize":
            V._resize_into(torch.from_numpy(img).to(gpu_device).unsqueeze(0), 4, 9, rect)
        elif fill == "depth":
            V._colorize_into(torch.from_numpy(d).to(gpu_device).unsqueeze(0), rect)
        else:
            V._masks_into(torch.from_numpy(seg).to(gpu_device).unsqueeze(0), False, COLORS3, rect)
        want = np.full((11, 17, 3), 0xA5, dtype=np.uint8)
        want[3:7, 5:14] = tile
        _same(panel, want)


def test_a_rectangle_that_does_not_fit_is_refused(gpu_device):
    from soccdpt_amd.utils import visualise as V
    panel = torch.zeros((6, 8, 3), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(RuntimeError, match="does not fit"):
        V._colorize_into(torch.zeros((1, 4, 5), device=gpu_device), V._Rect.tile(panel, 3, 4))      # rows 3..6 of a 6-row panel
    with pytest.raises(RuntimeError, match="does not fit"):
        V._colorize_into(torch.zeros((1, 2, 9), device=gpu_device), V._Rect.tile(panel, 0, 0))      # wider than the pitch


# ---- shrink ----
@pytest.mark.parametrize("shape,half", [((2, 2), (1, 1)), ((5, 7), (2, 4)), ((12, 22), (6, 11)), ((3, 9), (2, 4))])
@pytest.mark.parametrize("swap", [False, True])
def test_shrink_half(gpu_device, on_stream, shape, half, swap):
    from soccdpt_amd.utils.visualise import shrink_half
    img = np.random.default_rng(8).integers(0, 256, size=shape + (3,), dtype=np.uint8)
    want = R.shrink_half(img, swap_rb=swap)
    assert want.shape == half + (3,)
    _same(shrink_half(torch.from_numpy(img).to(gpu_device), swap_rb=swap), want)
    if shape == (5, 7):     # the last column averages column 6 with itself
        assert np.array_equal(R.shrink_half(img)[:, 3], ((img[0:4:2, 6].astype(int) + img[1:4:2, 6].astype(int)) * 2 + 2) >> 2)


# ---- panel ----
@pytest.mark.parametrize("H,W", [(6, 10), (5, 7)])
@pytest.mark.parametrize("k", [2, 3])
def test_panel(gpu_device, on_stream, H, W, k):
    from soccdpt_amd.utils.visualise import evaluation_panel
    rng = np.random.default_rng(9)
    frame = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    dp, dg = rng.random((H, W), dtype=np.float32), rng.random((H, W), dtype=np.float32) * 40.0
    sp, sg = rng.random((3, H, W), dtype=np.float32), rng.random((3, H, W), dtype=np.float32)
    dev = lambda a: torch.from_numpy(a).to(gpu_device)
    gt = dict(disp_gt=dev(dg), seg_gt=dev(sg)) if k == 3 else {}
    want = R.panel(frame, dp, sp, COLORS3, **(dict(disp_gt=dg, seg_gt=sg) if k == 3 else {}))
    assert want.shape == (H, int(round(k * W / 2)), 3)
    _same(evaluation_panel(dev(frame), dev(dp), dev(sp), COLORS3, **gt), want)


def test_panel_resizes_pictures_of_another_size(gpu_device, on_stream):
    from soccdpt_amd.utils.visualise import evaluation_panel
    rng = np.random.default_rng(10)
    frame = rng.integers(0, 256, size=(6, 10, 3), dtype=np.uint8)
    dp, sp = rng.random((4, 7), dtype=np.float32), rng.random((3, 3, 5), dtype=np.float32)
    dev = lambda a: torch.from_numpy(a).to(gpu_device)
    _same(evaluation_panel(dev(frame), dev(dp), dev(sp), COLORS3), R.panel(frame, dp, sp, COLORS3))


# ---- callers ----
class _Recorder:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)


@pytest.fixture(scope="module")
def net(gpu_device):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True)
    m.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    return m.eval().to(gpu_device)


def test_evaluate_occupancy_always_logs_the_panel(gpu_device, on_stream, net):
    from soccdpt_amd.utils.metrics import evaluate_occupancy
    from soccdpt_amd.utils.occupancy import occupancy_grid_to_points, occupancy_iou, semantic_pc_to_colors_and_pc
    from soccdpt_amd.utils.synth import synth_input
    x = synth_input(2, seed0=20).to(gpu_device)
    inv, seg, _, occ = net(x)
    flip = torch.from_numpy(np.random.default_rng(2).random((2, 256, 256, 32, 3)) < 1e-4).to(gpu_device)
    gt = (occ >= 0.5) ^ flip
    exp = _Recorder()
    x_raw = torch.from_numpy(np.random.default_rng(3).integers(0, 256, size=(2, net.height, net.width, 3), dtype=np.uint8))
    out = evaluate_occupancy(net, None, gpu_device, False, x_raw, gt, occ, inv, seg, COLORS3, torch.tensor(0.25), 1e-4, 7, 1, exp)
    assert exp.logged == [out]
    # without wandb the key set is what the function logged before, plus the picture
    assert {k for k in out if "/" not in k} == {"learning rate", "iou_3D", "plot_points_gt", "plot_points_pred", "loss", "step", "epoch", "plot"}
    plot = out["plot"]
    assert isinstance(plot, np.ndarray) and plot.dtype == np.uint8 and plot.shape == (net.height, net.width, 3)
    assert np.array_equal(plot, R.panel(x_raw[0].numpy(), inv[0].cpu().numpy(), seg[0].cpu().numpy(), COLORS3))
    # the other values as the function computed them before
    assert out["iou_3D"] == float(occupancy_iou(occ, gt, 3)["iou_3D"].mean().item())
    assert out["loss"] == 0.25 and out["step"] == 7 and out["epoch"] == 1 and out["learning rate"] == 1e-4
    for key, grid in (("plot_points_gt", gt[0]), ("plot_points_pred", occ[0])):
        pts, colors = semantic_pc_to_colors_and_pc(occupancy_grid_to_points(grid), COLORS3)
        assert np.array_equal(out[key], torch.cat([pts, colors.to(pts.dtype)], dim=1).cpu().numpy())


def test_evaluate_logs_the_reference_keys(gpu_device, on_stream, net, capsys):
    from soccdpt_amd.model.SOccDPT import DepthNet, SegNet
    from soccdpt_amd.utils.metrics import DEPTH_KEYS, evaluate, evaluate_depth, evaluate_seg
    from soccdpt_amd.utils.synth import synth_input
    H, W = net.height, net.width
    x = synth_input(1, seed0=31)
    inv, seg, points, _ = net(x.to(gpu_device))
    inv, seg = inv.reshape(1, H, W), seg.reshape(1, 3, H, W)
    rng = np.random.default_rng(11)
    y_disp = inv * 0.9 + 0.003
    y_seg = torch.from_numpy(rng.random((1, 3, H, W), dtype=np.float32)).to(gpu_device)
    y_seg[0, 1:, ::2] = 0.0        # rows of the ground-truth picture whose first colour channel stays 0 wherever class 0 does not match
    ones = torch.ones((1, H, W), dtype=torch.bool)
    val_set = [(x, None, ones, y_disp.cpu(), torch.ones((1, 3, H, W), dtype=torch.bool), y_seg.cpu())]
    x_raw = torch.from_numpy(rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8))
    exp = _Recorder()
    out = evaluate(net, SegNet(net), DepthNet(net), val_set, gpu_device, False, x_raw, y_disp, inv, y_seg, seg, points, COLORS3, torch.tensor(0.5),
                   3e-4, 11, 2, exp)
    assert exp.logged == [out]
    assert {k for k in out if "/" not in k} == {"learning rate", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "iou", "plot", "plot_points",
                                               "loss", "step", "epoch"}
    printed = capsys.readouterr().out
    assert "abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3" in printed and "iou " in printed and "loss: " in printed
    # the depth sums are accumulated with floating-point atomics (csrc/metrics.hip), so two runs may differ in the last bits of the f32 results
    assert tuple(out[k] for k in DEPTH_KEYS) == pytest.approx(evaluate_depth(DepthNet(net), val_set, gpu_device), rel=1e-5)
    assert out["iou"] == evaluate_seg(SegNet(net), val_set, gpu_device)
    assert out["loss"] == 0.5 and out["step"] == 11 and out["epoch"] == 2 and out["learning rate"] == 3e-4
    want = R.panel(x_raw[0].numpy(), inv[0].cpu().numpy(), seg[0].cpu().numpy(), COLORS3, disp_gt=y_disp[0].cpu().numpy(), seg_gt=y_seg[0].cpu().numpy())
    assert out["plot"].dtype == np.uint8 and out["plot"].shape == (H, W * 3 // 2, 3) and np.array_equal(out["plot"], want)
    gt_img = R.color_masks(y_seg.cpu().numpy(), COLORS3)[0]
    pp = R.plot_points(points.cpu().numpy()[0], gt_img)
    assert 0 < pp.shape[0] < H * W // 10 and out["plot_points"].shape == pp.shape
    assert np.array_equal(out["plot_points"], pp, equal_nan=True)


class _FixedNet:
    """Stands in for the model in write_visuals: camera size and one fixed forward result per call."""

    def __init__(self, H, W, outputs):
        self.height, self.width, self.outputs, self.calls = H, W, outputs, 0

    def __call__(self, x):
        self.calls += 1
        return self.outputs[self.calls - 1]


def test_write_visuals_files_decode_to_the_primitives(gpu_device, tmp_path):
    from soccdpt_amd.scripts.eval_SOccDPT import CLASS_2_COLOR_BDD, VISUAL_DIRS, write_visuals
    H, W = 6, 10
    rng = np.random.default_rng(12)
    dataset, outputs, want = [], [], []
    for i in range(2):
        frame = rng.integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)
        yd, ys = rng.random((1, H, W), dtype=np.float32), rng.random((1, 3, H, W), dtype=np.float32)
        pd, ps = rng.random((1, H, W), dtype=np.float32) * 3.0, rng.random((3, H, W), dtype=np.float32)      # B == 1: the model drops seg's batch dim
        dataset.append((torch.zeros((1, 3, 4, 4)), torch.from_numpy(frame), None, torch.from_numpy(yd), None, torch.from_numpy(ys)))
        outputs.append((torch.from_numpy(pd).to(gpu_device), torch.from_numpy(ps).to(gpu_device), None, None))
        bgr = {"RGB": frame[0], "GT_Depth": R.colorize(yd[0]), "GT_Seg": R.color_masks(ys, CLASS_2_COLOR_BDD)[0], "Pred_Depth": R.colorize(pd[0]),
               "Pred_Seg": R.color_masks(ps[None], CLASS_2_COLOR_BDD)[0]}
        rgb = {k: v[:, :, ::-1] for k, v in bgr.items()}
        rgb["Panel"] = R.panel(frame[0], pd[0], ps, CLASS_2_COLOR_BDD, disp_gt=yd[0], seg_gt=ys[0])
        want.append(rgb)
    root = write_visuals(_FixedNet(H, W, outputs), dataset, gpu_device, str(tmp_path / "vis"))
    for i, rgb in enumerate(want):
        for d in VISUAL_DIRS:
            got = R.png_decode(open(os.path.join(root, d, f"{i:04d}.png"), "rb").read())
            assert np.array_equal(got, rgb[d]), (i, d)
    assert not np.array_equal(want[0]["GT_Seg"], want[0]["Pred_Seg"])


BASE = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", "/nonexistent"]
PINNED_KEYS = {"fps", "iou", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"}


def test_eval_script_without_the_flag_is_unchanged(gpu_device, capsys, tmp_path, monkeypatch):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    monkeypatch.chdir(tmp_path)
    assert build_parser().parse_args(BASE).visuals is None
    assert build_parser().parse_args(BASE + ["--visuals"]).visuals == os.path.join("media", "visuals")
    plain = main(build_parser().parse_args(BASE))
    assert set(plain) == PINNED_KEYS
    assert "VISUALS" not in capsys.readouterr().out and not os.listdir(tmp_path)


def test_eval_script_visuals_flag(gpu_device, capsys, tmp_path):
    from soccdpt_amd.scripts.eval_SOccDPT import VISUAL_DIRS, build_parser, main
    r = main(build_parser().parse_args(BASE + ["--visuals", str(tmp_path)]))
    assert set(r) == PINNED_KEYS | {"visuals"} and "VISUALS: " in capsys.readouterr().out
    root = r["visuals"]
    assert root == os.path.join(str(tmp_path), "dpt_swin2_tiny_256_bdd_3") and sorted(os.listdir(root)) == sorted(VISUAL_DIRS)
    for d in VISUAL_DIRS:
        assert sorted(os.listdir(os.path.join(root, d))) == [f"{i:04d}.png" for i in range(10)]
    # the pictures of one frame hang together: the panel is the half-size RGB view of [RGB | Pred_Depth | GT_Depth] over [RGB | Pred_Seg | GT_Seg]
    for i in (0, 9):
        pic = {d: R.png_decode(open(os.path.join(root, d, f"{i:04d}.png"), "rb").read()) for d in VISUAL_DIRS}
        assert pic["RGB"].shape == (1080, 1920, 3) and pic["Panel"].shape == (1080, 2880, 3)
        bgr = {d: p[:, :, ::-1] for d, p in pic.items()}
        vis = np.concatenate([np.concatenate([bgr["RGB"], bgr["Pred_Depth"], bgr["GT_Depth"]], 1), np.concatenate([bgr["RGB"], bgr["Pred_Seg"], bgr["GT_Seg"]], 1)], 0)
        assert np.array_equal(pic["Panel"], R.shrink_half(vis, swap_rb=True))
        assert len(np.unique(pic["Pred_Depth"].reshape(-1, 3), axis=0)) > 100
