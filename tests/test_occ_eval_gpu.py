"""GPU: the occupancy-evaluation kernels (csrc/occ_eval.hip) and their Python layer against the numpy specification of tests/occ_eval_refs.py, which
tests/test_occ_eval_cpu.py pins bit for bit to the reference.  Every comparison is exact unless a tolerance is named.  Every test but the
evaluation-script one runs twice: on the null stream and on a side stream with the result consumed on that stream."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import occ_eval_refs as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "occ_points.npz"))
DEFAULT_GRID, DEFAULT_SCALE = (256, 256, 32), (2.0, 2.0, 0.666)


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


def _dev_bits(words, dev):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).to(dev)


def _points(words, grid, scale, C, dev, rows=1, **kw):
    from soccdpt_amd.utils.occupancy import occupancy_bits_to_points
    return occupancy_bits_to_points(_dev_bits(words, dev), grid, scale, num_classes=C, rows=rows, **kw)


def _check_list(words, grid, scale, C, dev):
    res = _points(words, grid, scale, C, dev)
    want = R.points_from_bits(words, grid, scale, C)
    got = res.points.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)
    mask = R.unpack_bits(words, int(np.prod(grid)) * C)
    assert np.array_equal(res.counts.cpu().numpy(), R.class_counts(mask, C)[None])
    assert int(res.total.item()) == want.shape[0]
    return res, want


def test_points_from_forward_golden_bits(gpu_device, on_stream):
    words = np.load(os.path.join(HERE, "golden", "e2e_B1_tanh_oracle.npz"))["occ_bits"]
    res, want = _check_list(words, DEFAULT_GRID, DEFAULT_SCALE, 3, gpu_device)
    assert want.shape[0] == 707
    again = _points(words, DEFAULT_GRID, DEFAULT_SCALE, 3, gpu_device)
    assert again.points.cpu().numpy().tobytes() == res.points.cpu().numpy().tobytes()          # two runs, identical bytes


@pytest.mark.parametrize("case", ["default", "odd", "small", "empty"])
def test_points_from_fixture_bits(gpu_device, on_stream, case):
    """The packed grids of the reference fixture -> the lists the reference itself returned (`small` has its padding bits set)."""
    grid = [int(v) for v in G[case + "_grid"]]
    res = _points(G[case + "_bits"], grid[:3], tuple(G[case + "_scale"]), grid[3], gpu_device)
    got = res.points.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == G[case + "_points"].shape
    assert np.array_equal(got, G[case + "_points"])


@pytest.mark.parametrize("density", [0.0, 1e-4, 1e-2, 0.5, 1.0])
def test_points_random_default_geometry(gpu_device, on_stream, density):
    """density 1.0 is all ones: 6,291,456 rows (201 MB), the scan and the write at full scale."""
    ncell = int(np.prod(DEFAULT_GRID)) * 3
    rng = np.random.default_rng(int(density * 1e6) + 5)
    mask = np.ones(ncell, dtype=bool) if density == 1.0 else rng.random(ncell) < density
    words = R.pack_bits(mask)
    res, want = _check_list(words, DEFAULT_GRID, DEFAULT_SCALE, 3, gpu_device)
    assert want.shape[0] == int(mask.sum())
    if density == 1e-2:
        again = _points(words, DEFAULT_GRID, DEFAULT_SCALE, 3, gpu_device)
        assert torch.equal(again.points, res.points)


@pytest.mark.parametrize("C", [1, 3, 4, 5])
def test_points_class_counts(gpu_device, on_stream, C):
    grid, scale = (33, 21, 7), (2.0, 1.5, 0.666)          # 4851 voxels: ncell is a multiple of 32 for no C here
    rng = np.random.default_rng(40 + C)
    mask = rng.random(int(np.prod(grid)) * C) < 0.2
    _check_list(R.pack_bits(mask), grid, scale, C, gpu_device)


@pytest.mark.parametrize("geom", [(DEFAULT_GRID, DEFAULT_SCALE), ((5, 7, 3), (1.5, 0.7, 0.666)), ((48, 40, 12), (2.0, 2.0, 0.666))])
def test_points_batched_rows(gpu_device, on_stream, geom):
    grid, scale = geom
    C, ncell = 3, int(np.prod(grid)) * 3
    rng = np.random.default_rng(77)
    masks = [rng.random(ncell) < d for d in (0.02, 0.0, 0.3)]
    words = np.stack([R.pack_bits(m) for m in masks])
    res = _points(words, grid, scale, C, gpu_device, rows=3)
    want = [R.points_from_mask(m, grid, scale, C) for m in masks]
    assert np.array_equal(res.points.cpu().numpy(), np.concatenate(want, axis=0))
    assert np.array_equal(res.counts.cpu().numpy(), np.stack([R.class_counts(m, C) for m in masks]))
    assert np.array_equal(res.counts.cpu().numpy(), np.stack([np.bincount(w[:, 3].astype(np.int64), minlength=C) for w in want]))


def test_points_capacity_form_and_colours(gpu_device, on_stream):
    """max_points: no host synchronisation; the first min(N, max_points) rows of the full list, the true N on the device."""
    grid, scale, C = (48, 40, 12), (2.0, 2.0, 0.666), 3
    rng = np.random.default_rng(9)
    mask = rng.random(int(np.prod(grid)) * C) < 0.1
    words = R.pack_bits(mask)
    want = R.points_from_mask(mask, grid, scale, C)
    n = want.shape[0]
    colors = {0: (255, 0, 0), 1: (0, 200, 10), 2: (7, 8, 9)}
    small = _points(words, grid, scale, C, gpu_device, max_points=1000, class_2_color=colors)
    assert tuple(small.points.shape) == (1000, 4) and int(small.total.item()) == n > 1000
    assert np.array_equal(small.points.cpu().numpy(), want[:1000])
    table = np.array([colors[c] for c in range(C)], dtype=np.uint8)
    assert np.array_equal(small.colors.cpu().numpy(), table[want[:1000, 3].astype(np.int64)])
    big = _points(words, grid, scale, C, gpu_device, max_points=n + 50, class_2_color=colors)
    assert int(big.total.item()) == n
    assert np.array_equal(big.points.cpu().numpy()[:n], want) and not big.points[n:].any()
    full = _points(words, grid, scale, C, gpu_device, class_2_color=colors)
    assert np.array_equal(full.colors.cpu().numpy(), table[want[:, 3].astype(np.int64)])
    from soccdpt_amd.utils.occupancy import semantic_pc_to_colors_and_pc
    pts, col = semantic_pc_to_colors_and_pc(full.points, colors)
    assert torch.equal(col, full.colors) and torch.equal(pts, full.points[:, :3])


def _np_pred(a, t, strict):
    with np.errstate(invalid="ignore"):
        return (a.astype(np.float32) > np.float32(t)) if strict else (a.astype(np.float32) >= np.float32(t))


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("geom", [(64, 48, 16, 3), (5, 7, 3, 3)])
@pytest.mark.parametrize("rows", [1, 2])
def test_pack_matches_packbits(gpu_device, on_stream, strict, geom, rows):
    from soccdpt_amd.utils.occupancy import pack_occupancy
    rng = np.random.default_rng(3 + rows)
    ncell = int(np.prod(geom))
    shape = ((rows,) if rows > 1 else ()) + geom
    f = rng.random(shape).astype(np.float32)
    flat = f.reshape(-1)
    flat[::7] = 0.5
    flat[3::41] = np.nan
    flat[5::53] = np.inf
    flat[6::59] = -np.inf
    grids = [(f, 0.5), (rng.random(shape) < 0.3, 0.5), ((rng.random(shape) * 4).astype(np.uint8), 2.0),
             (rng.integers(0, 25, size=shape).astype(np.int32), 10.0), (rng.integers(-3, 3, size=shape).astype(np.int32), 0.0)]
    for a, thr in grids:
        got = pack_occupancy(torch.from_numpy(a).to(gpu_device), threshold=thr, strict=strict)
        assert got.dtype == torch.int32 and tuple(got.shape) == (rows, (ncell + 31) // 32)
        m = _np_pred(a, thr, strict).reshape(rows, ncell)
        want = np.stack([R.pack_bits(r) for r in m])
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want), (a.dtype, thr)
        by = np.stack([np.packbits(r, bitorder="little") for r in m])
        assert np.array_equal(got.cpu().numpy().view(np.uint8)[:, : by.shape[1]], by)
        if ncell & 31:
            assert not (got.cpu().numpy().view(np.uint32)[:, -1] >> (ncell & 31)).any()        # tail bits zero


def test_pack_default_geometry_two_rows(gpu_device, on_stream):
    from soccdpt_amd.utils.occupancy import pack_occupancy
    rng = np.random.default_rng(12)
    a = rng.random((2,) + DEFAULT_GRID + (3,), dtype=np.float32)
    got = pack_occupancy(torch.from_numpy(a).to(gpu_device))
    want = np.stack([R.pack_bits(r.reshape(-1) >= 0.5) for r in a])
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want)


@pytest.fixture(scope="module")
def nets(gpu_device):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    sd = synth_state_dict(alias_pretrained=True)
    out = []
    for share in (False, True):
        m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, share_occupancy_rows=share)
        m.load_state_dict(sd, strict=False)
        out.append(m.eval().to(gpu_device))
    return out


@pytest.mark.parametrize("share", [False, True])
def test_through_the_model(gpu_device, on_stream, nets, share):
    from soccdpt_amd.utils.occupancy import occupancy_grid_to_points, pack_occupancy
    from soccdpt_amd.utils.synth import synth_input
    net = nets[1 if share else 0]
    x = synth_input(2, seed0=20).to(gpu_device)
    _, _, _, occ = net(x)
    assert tuple(occ.shape) == (2, 256, 256, 32, 3)
    a = occupancy_grid_to_points(occ[0])
    b = net.occupancy_points()
    want = R.points_from_mask(occ[0].cpu().numpy() >= 0.5, DEFAULT_GRID, DEFAULT_SCALE, 3)
    assert want.shape[0] > 100
    assert a.dtype == torch.float64 and np.array_equal(a.cpu().numpy(), want) and torch.equal(a, b)
    assert torch.equal(pack_occupancy(occ[0]).reshape(-1), net.last_occ_bits) and net.last_occ_bits.dtype == torch.int32
    pts, col = net.occupancy_points(class_2_color=[(1, 2, 3), (4, 5, 6), (7, 8, 9)])
    assert torch.equal(pts, a) and np.array_equal(col.cpu().numpy(), np.array([(1, 2, 3), (4, 5, 6), (7, 8, 9)], dtype=np.uint8)[want[:, 3].astype(int)])


def test_gt_processor_occupancy_points(gpu_device, on_stream):
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    from tests.golden_inputs import gt_occ_inputs
    disp, seg, K, H, W, C = gt_occ_inputs()
    proc = OccupancyProcessor(intrinsic_matrix=K, height=H, width=W, grid_size=(256, 256, 32), scale=(2.0, 2.0, 0.666), shift=(0.0, 0.0, 0.0),
                              pc_scale=(500.0, 2500.0, 200.0), pc_shift=(100.0, 40.0, 0.0), point_count_threshold=10, num_classes=C)
    d, s = torch.from_numpy(np.stack([disp, disp])).to(gpu_device), torch.from_numpy(np.stack([seg, seg])).to(gpu_device)
    plain = proc.process(d, s)
    assert sorted(plain) == ["counts", "depth", "occupancy_grid", "points"]
    r = proc.process(d, s, want_occupancy_points=True)
    assert sorted(r) == ["counts", "depth", "occupancy_grid", "occupancy_points", "points"]
    assert isinstance(r["occupancy_points"], list) and len(r["occupancy_points"]) == 2
    for p in r["occupancy_points"]:
        assert p.dtype == torch.float64 and np.array_equal(p.cpu().numpy(), G["gt_points"])
    assert torch.equal(r["occupancy_grid"], plain["occupancy_grid"]) and int(r["occupancy_grid"][0].sum().item()) == 1810


def test_occupancy_iou(gpu_device, on_stream):
    from soccdpt_amd.utils.occupancy import occupancy_iou
    grid, C = (48, 40, 12), 3
    ncell = int(np.prod(grid)) * C
    rng = np.random.default_rng(21)
    gts = [rng.random(ncell) < d for d in (0.3, 0.05, 0.0)]
    preds = [np.where(rng.random(ncell) < 0.8, g, rng.random(ncell) < 0.2) for g in gts]
    gt_bits = _dev_bits(np.stack([R.pack_bits(m) for m in gts]), gpu_device)
    pred_bits = _dev_bits(np.stack([R.pack_bits(m) for m in preds]), gpu_device)

    def check(res, want_counts):
        assert res["counts"].dtype == torch.int64 and np.array_equal(res["counts"].cpu().numpy(), want_counts)
        per, mean = R.iou_from_counts(want_counts)
        np.testing.assert_allclose(res["iou_3D"].cpu().numpy(), mean, rtol=1e-12, atol=0)
        np.testing.assert_allclose(res["iou_per_class"].cpu().numpy(), per, rtol=1e-12, atol=0)
        for k in ("iou_3D", "iou_per_class", "precision", "recall"):
            assert res[k].dtype == torch.float64 and bool(torch.isfinite(res[k]).all())

    want = np.stack([R.iou_counts(p, g, C) for p, g in zip(preds, gts)])
    check(occupancy_iou(pred_bits, gt_bits, C), want)                                                   # packed / packed
    dense = torch.from_numpy(np.stack(preds).reshape((3,) + grid + (C,)).astype(np.float32)).to(gpu_device)
    check(occupancy_iou(dense, gt_bits, C), want)                                                       # dense / packed
    check(occupancy_iou(pred_bits, torch.from_numpy(np.stack(gts).reshape((3,) + grid + (C,))).to(gpu_device), C), want)   # packed / dense bool
    check(occupancy_iou(pred_bits[0], gt_bits, C), np.stack([R.iou_counts(preds[0], g, C) for g in gts]))   # one predicted row against three
    same = occupancy_iou(gt_bits[:1], gt_bits[:1], C)
    n = want[0, :, 3].astype(np.float64)
    np.testing.assert_allclose(same["iou_per_class"].cpu().numpy()[0], n / (n + 1e-7), rtol=1e-12, atol=0)
    assert (same["iou_per_class"] < 1.0).all()
    a = rng.random(ncell) < 0.3
    disjoint = occupancy_iou(_dev_bits(R.pack_bits(a), gpu_device), _dev_bits(R.pack_bits(~a), gpu_device), C)
    assert (disjoint["iou_3D"] == 0).all() and (disjoint["counts"][..., 0] == 0).all()
    empty = occupancy_iou(gt_bits[2], gt_bits[2], C)
    assert (empty["iou_3D"] == 0).all() and bool(torch.isfinite(empty["iou_3D"]).all()) and (empty["precision"] == 0).all() and (empty["recall"] == 0).all()
    # a 315-cell grid with garbage in the padding bits: counted only up to ncell
    small = (rng.random(315) < 0.5)
    w = R.pack_bits(small)
    w[-1] |= np.uint32(0xF8000000)
    res = occupancy_iou(_dev_bits(w, gpu_device), _dev_bits(w, gpu_device), 3, grid_size=(5, 7, 3))
    assert np.array_equal(res["counts"].cpu().numpy()[0], R.iou_counts(small, small, 3))


def test_iou_default_geometry_eight_rows(gpu_device, on_stream):
    from soccdpt_amd.utils.occupancy import occupancy_iou
    ncell = int(np.prod(DEFAULT_GRID)) * 3
    rng = np.random.default_rng(5)
    pred = rng.random(ncell) < 0.01
    gts = [np.where(rng.random(ncell) < 0.9, pred, rng.random(ncell) < 0.01) for _ in range(8)]
    res = occupancy_iou(_dev_bits(R.pack_bits(pred), gpu_device), _dev_bits(np.stack([R.pack_bits(g) for g in gts]), gpu_device), 3)
    assert np.array_equal(res["counts"].cpu().numpy(), np.stack([R.iou_counts(pred, g, 3) for g in gts]))


class _Recorder:
    def __init__(self):
        self.logged = []

    def log(self, d):
        self.logged.append(d)


def test_evaluate_occupancy_logs_the_reference_keys(gpu_device, on_stream, nets):
    from soccdpt_amd.utils.metrics import evaluate_occupancy
    from soccdpt_amd.utils.occupancy import occupancy_iou
    from soccdpt_amd.utils.synth import synth_input
    net = nets[0]
    x = synth_input(2, seed0=20).to(gpu_device)
    inv, seg, _, occ = net(x)
    rng = np.random.default_rng(2)
    flip = torch.from_numpy(rng.random((2,) + DEFAULT_GRID + (3,)) < 1e-4).to(gpu_device)
    gt = (occ >= 0.5) ^ flip
    colors = {0: (255, 0, 0), 1: (0, 255, 0), 2: (0, 0, 255)}
    exp = _Recorder()
    x_raw = torch.zeros((2, net.height, net.width, 3), dtype=torch.uint8)
    out = evaluate_occupancy(net, None, gpu_device, False, x_raw, gt, occ, inv, seg, colors, torch.tensor(0.25), 1e-4, 7, 1, exp)
    assert len(exp.logged) == 1 and exp.logged[0] is out
    for k in ("learning rate", "iou_3D", "plot_points_gt", "plot_points_pred", "loss", "step", "epoch"):
        assert k in out
    want = float(occupancy_iou(occ, gt, 3)["iou_3D"].mean().item())
    assert out["iou_3D"] == want and 0.0 < want < 1.0
    assert out["loss"] == 0.25 and out["step"] == 7 and out["epoch"] == 1 and out["learning rate"] == 1e-4
    pred_list = R.points_from_mask(occ[0].cpu().numpy() >= 0.5, DEFAULT_GRID, DEFAULT_SCALE, 3)
    assert isinstance(out["plot_points_pred"], np.ndarray) and out["plot_points_pred"].shape == (pred_list.shape[0], 6)
    assert np.array_equal(out["plot_points_pred"][:, :3], pred_list[:, :3])
    assert np.array_equal(out["plot_points_pred"][:, 3:], np.array([colors[c] for c in range(3)], dtype=np.float64)[pred_list[:, 3].astype(int)])
    gt_list = R.points_from_mask(gt[0].cpu().numpy(), DEFAULT_GRID, DEFAULT_SCALE, 3)
    assert np.array_equal(out["plot_points_gt"][:, :3], gt_list[:, :3])


def test_eval_script_occupancy_flag(gpu_device, capsys):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    base = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", "/nonexistent"]
    assert build_parser().parse_args(base).occupancy is False
    r = main(build_parser().parse_args(base + ["--occupancy"]))
    out = capsys.readouterr().out
    for line in ("FPS:", "IOU:", "A3:", "IOU_3D:", "OCC_POINTS:"):
        assert line in out
    assert 0.0 <= r["iou_3D"] <= 1.0 and r["occ_points"] > 0
    assert set(r) == {"fps", "iou", "abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3", "iou_3D", "occ_points"}
