"""GPU: the occupancy grid pictures (csrc/occ_view.hip, soccdpt_amd/utils/occupancy_views.py) against the numpy restatements of
tests/occ_view_refs.py.  Integer arithmetic everywhere but the camera projection, which is float64 with every operation rounded on its own: every
comparison is bit for bit."""
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import occ_view_refs as R

pytestmark = pytest.mark.gpu
COLORS = [(10, 200, 30), (250, 0, 142), (220, 20, 60), (1, 2, 3), (90, 80, 70), (255, 255, 255), (0, 128, 0), (17, 34, 51)]
BG = (32, 33, 34)


def _bits(words: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(words.view(np.int32).copy()).to(dev)


def _same(got: torch.Tensor, want: np.ndarray, what=""):
    g = got.cpu().numpy()
    if want.dtype == np.uint64:
        g = g.view(np.uint64)
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
    assert g.tobytes() == np.ascontiguousarray(want).tobytes(), f"{what}: {int((g != want).sum())} elements differ"


def _patterns(rows, g, C, seed):
    shape = (rows,) + tuple(g) + (C,)
    rng = np.random.default_rng(seed)
    corners = np.zeros(shape, dtype=bool)
    for k, (i0, i1, i2) in enumerate((a, b, c) for a in (0, g[0] - 1) for b in (0, g[1] - 1) for c in (0, g[2] - 1)):
        corners[:, i0, i1, i2, k % C] = True
    return dict(empty=np.zeros(shape, dtype=bool), full=np.ones(shape, dtype=bool), corners=corners, random=rng.random(shape) < 0.1)


def _check_columns(dense, g, C, dev, garbage=(False, True)):
    from soccdpt_amd.utils.occupancy_views import occupancy_columns
    for tail in garbage:
        bits = _bits(R.pack(dense, tail_garbage=tail), dev)
        for axis in (0, 1, 2):
            for from_high in (False, True):
                got = occupancy_columns(bits, g, num_classes=C, axis=axis, from_high=from_high)
                for name, want in zip(got._fields, R.columns(dense, axis, from_high)):
                    _same(getattr(got, name), want, (name, g, C, axis, from_high, tail))


# ---- columns ----
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("g,C", [((5, 7, 3), 3), ((3, 2, 37), 1), ((4, 4, 4), 5), ((2, 3, 4), 8)])
def test_columns_every_axis_and_direction(gpu_device, g, C, rows):
    """(5,7,3) x 3: 315 cells, 10 words, a 27-bit tail, voxels across word boundaries; (3,2,37) x 1: a column longer than a word; (4,4,4) x 5: a class
    stride that does not divide 32; 8 classes.  Empty, full, one bit per corner and a seeded density of 0.1, with zeros and with garbage beyond the last cell."""
    for name, dense in _patterns(rows, g, C, seed=rows * 100 + C).items():
        _check_columns(dense, g, C, gpu_device)


def test_columns_with_each_output_left_out(gpu_device):
    from soccdpt_amd.utils.occupancy_views import _columns
    g, C = (5, 7, 3), 3
    dense = _patterns(2, g, C, seed=5)["random"]
    bits = _bits(R.pack(dense, tail_garbage=True), gpu_device)
    names = ("top", "first", "count", "classes")
    for axis in (0, 1, 2):
        want = dict(zip(names, R.columns(dense, axis, True)))
        for left_out in names:
            got = _columns(bits, g, C, axis, True, want=tuple(n for n in names if n != left_out))
            assert got[left_out] is None
            for n in names:
                if n != left_out:
                    _same(got[n], want[n], (axis, left_out, n))
    # a dense grid goes through pack_occupancy
    from soccdpt_amd.utils.occupancy_views import occupancy_columns
    got = occupancy_columns(torch.from_numpy(dense).to(gpu_device), g, num_classes=C, axis=2)
    _same(got.count, R.columns(dense, 2, False)[2])
    with pytest.raises(ValueError):
        occupancy_columns(bits, (5, 7, 4), num_classes=C)


def test_columns_default_geometry(gpu_device):
    """(256, 256, 32) x 3, two rows: 196,608 words per row, many workgroups."""
    g, C = (256, 256, 32), 3
    rng = np.random.default_rng(7)
    dense = rng.random((2,) + g + (C,)) < 0.02
    dense[1, :, 100:] = False
    _check_columns(dense, g, C, gpu_device, garbage=(False,))


# ---- paint ----
def test_paint_options(gpu_device):
    from soccdpt_amd.utils.occupancy_views import occupancy_view
    g, C = (5, 7, 3), 3
    dense = _patterns(2, g, C, seed=9)["random"]
    bits = _bits(R.pack(dense), gpu_device)
    n = 0
    for axis, from_high in ((1, False), (1, True), (0, True), (2, False)):
        top, first, _, _ = R.columns(dense, axis, from_high)
        for zoom in (1, 3):
            for shade in (0, 192, 77):
                for flip in ((False, False), (True, False), (False, True), (True, True)):
                    for transpose in (False, True):
                        got = occupancy_view(bits, g, COLORS[:C], num_classes=C, axis=axis, from_high=from_high, zoom=zoom, shade=shade, background=BG, flip=flip,
                                             transpose=transpose)
                        _same(got, R.paint(top, first, g[axis], from_high, COLORS[:C], BG, shade, zoom, flip[0], flip[1], transpose), (axis, from_high, zoom, shade, flip, transpose))
                        n += 1
    assert n == 192
    assert len(np.unique(R.paint(top, first, 3, False, COLORS[:C], BG, 192, 1, False, False, False).reshape(-1, 3), axis=0)) > 4    # shaded, not flat


def test_paint_depth_len_one_and_bird_eye_view(gpu_device):
    from soccdpt_amd.utils.occupancy_views import bird_eye_view, occupancy_view, view_size
    g, C = (4, 1, 3), 2
    dense = _patterns(1, g, C, seed=3)["corners"]
    bits = _bits(R.pack(dense), gpu_device)
    top, first, _, _ = R.columns(dense, 1, False)
    _same(occupancy_view(bits, g, COLORS[:C], num_classes=C, axis=1, shade=192, zoom=1, background=BG), R.paint(top, first, 1, False, COLORS[:C], BG, 192, 1, False, False, False))
    # camera X to the right, depth upwards: picture [g2 * zoom, g0 * zoom]
    bev = bird_eye_view(bits, g, COLORS[:C], num_classes=C, zoom=2, background=BG)
    assert tuple(bev.shape) == (1,) + view_size(g, 1, 2, True) + (3,) == (1, 6, 8, 3)
    _same(bev, R.paint(top, first, 1, False, COLORS[:C], BG, 128, 2, False, True, True))
    assert bev[0, 5, 0].tolist() == list(COLORS[0]) and bev[0, 0, 0].tolist() != list(BG)        # voxel (0, 0, 0): bottom left; (0, 0, 2): top left


def test_paint_into_a_panel_leaves_the_rest_alone(gpu_device):
    from soccdpt_amd.utils.occupancy_views import _Rect, _table, _view_into
    g, C = (5, 7, 3), 3
    dense = _patterns(1, g, C, seed=4)["random"]
    bits = _bits(R.pack(dense), gpu_device)
    top, first, _, _ = R.columns(dense, 1, False)
    tile = R.paint(top, first, 7, False, COLORS[:C], BG, 128, 2, False, False, False)[0]        # 10 x 6
    panel = torch.full((15, 11, 3), 77, dtype=torch.uint8, device=gpu_device)
    table = _table(COLORS[:C], C, gpu_device)
    _view_into(bits, g, C, table, 1, False, 2, 128, BG, (False, False), False, _Rect.tile(panel, 3, 4))
    want = np.full((15, 11, 3), 77, dtype=np.uint8)
    want[3:13, 4:10] = tile
    _same(panel, want)
    # a rectangle that does not fit: four rows too low, and a pitch below the tile's width; nothing is written
    for rect in (_Rect.tile(panel, 6, 4), _Rect(panel, 5, 0, 15 * 11)):
        before = panel.clone()
        with pytest.raises(RuntimeError, match="soccdpt_occ_view_paint"):
            _view_into(bits, g, C, table, 1, False, 2, 128, BG, (False, False), False, rect)
        assert torch.equal(panel, before)
    with pytest.raises(RuntimeError, match="soccdpt_occ_view_paint"):
        _view_into(bits, g, C, table, 1, False, 0, 128, BG, (False, False), False, _Rect.tile(panel, 0, 0))


# ---- 2-D IoU ----
def test_iou2d(gpu_device):
    from soccdpt_amd.utils.occupancy_views import bev_iou
    g, C = (5, 7, 3), 3
    pats = _patterns(3, g, C, seed=21)
    gt = pats["random"].copy()
    gt[1] = False                                   # an empty ground-truth row
    gt[2, ..., 2] = False                           # a row without class 2
    pred = _patterns(1, g, C, seed=22)["random"]
    for axis in (0, 1, 2):
        out = bev_iou(_bits(R.pack(pred), gpu_device), _bits(R.pack(gt, tail_garbage=True), gpu_device), g, num_classes=C, axis=axis)
        want = R.iou2d(R.columns(pred, axis, False)[3], R.columns(gt, axis, False)[3], C)
        _same(out["counts"], want.astype(np.int64), axis)
        w = want.astype(np.float64)
        assert np.array_equal(out["iou_per_class"].cpu().numpy(), w[..., 0] / (w[..., 1] + 1e-7))
        assert np.allclose(out["iou_2D"].cpu().numpy(), (w[..., 0] / (w[..., 1] + 1e-7)).mean(axis=1), rtol=1e-15)
    # identical maps: 1 where the class occurs, 0 (not NaN) where it does not; an empty union
    same = bev_iou(_bits(R.pack(gt), gpu_device), _bits(R.pack(gt), gpu_device), g, num_classes=C)
    iou = same["iou_per_class"].cpu().numpy()
    assert np.allclose(iou[0], 1.0) and np.array_equal(iou[1], np.zeros(3)) and np.allclose(iou[2], [1.0, 1.0, 0.0]) and np.isfinite(iou).all()
    assert same["counts"][1].abs().sum().item() == 0
    empty = np.zeros((1,) + g + (C,), dtype=bool)
    assert bev_iou(_bits(R.pack(empty), gpu_device), _bits(R.pack(empty), gpu_device), g, num_classes=C)["iou_2D"].item() == 0.0
    with pytest.raises(ValueError):
        bev_iou(_bits(R.pack(gt[:2]), gpu_device), _bits(R.pack(gt), gpu_device), g, num_classes=C)


# ---- camera view ----
OG, OC, OH, OW = (6, 5, 4), 3, 24, 40
OK_ = (12.0, 11.0, 20.0, 12.0)


def _overlay_matrices():
    from soccdpt_amd.lib import host_rotation_matrices
    from soccdpt_amd.utils.occupancy_views import model_voxel_to_camera
    # scaled identity: Z = 0.8 (i2 + 0.5) - 0.6 = -0.2 (behind the camera), 0.6, 1.4, 2.2; X / Z reaches +-2.1: u from -5 to 45
    scaled = np.array([[0.5, 0, 0, -1.5], [0, 0.5, 0, -1.2], [0, 0, 0.8, -0.6]], dtype=np.float64)
    # the model's own matrix for this grid with the 7 degree correction: cells of 1 x 1 x 2 m, irrational entries
    model = model_voxel_to_camera(OG, (6.0, 5.0, 8.0), host_rotation_matrices((7.0, 0.0, 0.0)))
    model[:, 3] = (-2.9, -2.3, 0.05)
    return dict(scaled=scaled, model=model)


@pytest.fixture(scope="module")
def overlay_scene():
    rng = np.random.default_rng(31)
    dense = rng.random((2,) + OG + (OC,)) < 0.3
    dense[0, 2, 2, 1, :] = True                      # one voxel, three classes: the same f32 depth, the lowest cell index wins
    dense[0, 2, 2, 2, 1] = dense[0, 2, 2, 3, 2] = True
    frames = rng.integers(0, 256, size=(2, OH, OW, 3), dtype=np.uint8)
    return dense, frames


@pytest.mark.parametrize("which", ["scaled", "model"])
@pytest.mark.parametrize("half,max_r,z_near", [(0.4, 3, 0.1), (0.4, 12, 0.7), (0.01, 12, 0.1), (0.12, 2, 0.1)])
def test_overlay_zbuffer_and_picture(gpu_device, overlay_scene, which, half, max_r, z_near):
    """Cells behind the camera and at Z <= z_near (0.7 drops the Z = 0.6 layer), squares outside and partly outside the 40 x 24 frame, r clamped by
    max_radius_px (0.4 / 0.6 * 12 = 8 > 3) and r = 0 (0.01), cells over each other at different and at equal depth.  zbuf and the picture equal the
    numpy float64 restatement bit for bit: a single differing pixel means the contraction pragma of occ_view.hip is not in force."""
    from soccdpt_amd.utils.occupancy_views import _grid_bits, occupancy_overlay, occupancy_zbuffer
    dense, frames = overlay_scene
    M = _overlay_matrices()[which]
    K = np.array(OK_)
    for rows in (1, 2):
        d = dense[:rows]
        want_z = R.splat(d, M, OK_, half, max_r, z_near, OH, OW)
        hit = want_z != R.EMPTY_KEY
        assert 0 < hit.sum() < hit.size
        bits, g = _grid_bits(_bits(R.pack(d, tail_garbage=True), gpu_device), OG, OC, "test")
        _same(occupancy_zbuffer(bits, g, OC, M, K, half, max_r, z_near, OH, OW), want_z, ("zbuf", which, rows))
        for frame_rows in sorted({1, rows}):
            f = frames[:frame_rows]
            for alpha in (0, 160, 256):
                got = occupancy_overlay(bits, torch.from_numpy(f).to(gpu_device), M, OK_, OG, COLORS[:OC], num_classes=OC, alpha=alpha, half_extent_m=half,
                                        max_radius_px=max_r, z_near=z_near)
                _same(got, R.resolve(want_z, f, COLORS[:OC], OC, alpha), ("picture", which, rows, frame_rows, alpha))
        got = occupancy_overlay(bits, None, M, OK_, OG, COLORS[:OC], num_classes=OC, alpha=160, half_extent_m=half, max_radius_px=max_r, z_near=z_near, size=(OH, OW))
        _same(got, R.resolve(want_z, None, COLORS[:OC], OC, 160), ("no frames", which, rows))


def _cell_geometry(dense, M, half, max_r):
    """Per occupied cell of row 0: Z, the square's centre and the unclamped and clamped half-width (plain numpy; only used to classify the cases)."""
    idx = np.argwhere(dense[0])
    P = (idx[:, 1:4] + 0.5) @ M[:, :3].T + M[:, 3]
    Z = P[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = np.floor(P[:, 0] / Z * OK_[0] + OK_[2] + 0.5), np.floor(P[:, 1] / Z * OK_[1] + OK_[3] + 0.5)
        rd = np.floor(half / Z * OK_[0])
    return Z, u, v, rd, np.minimum(rd, max_r)


def test_overlay_scene_reaches_its_cases(overlay_scene):
    """The scene and the parameter sets of the test above do contain the cases it claims to cover (checked on the host; no GPU work)."""
    dense, _ = overlay_scene
    mats = _overlay_matrices()
    seen = set()
    for which, M in mats.items():
        for half, max_r, z_near in ((0.4, 3, 0.1), (0.4, 12, 0.7), (0.01, 12, 0.1), (0.12, 2, 0.1)):
            Z, u, v, rd, r = _cell_geometry(dense, M, half, max_r)
            front = Z > z_near
            out = (u + r < 0) | (u - r > OW - 1) | (v + r < 0) | (v - r > OH - 1)
            inside = (u - r >= 0) & (u + r <= OW - 1) & (v - r >= 0) & (v + r <= OH - 1)
            for name, mask in (("behind", Z <= 0), ("near", (Z > 0) & ~front), ("outside", front & out), ("partly", front & ~out & ~inside),
                               ("clamped", front & (rd > max_r)), ("r0", front & (r == 0) & ~out)):
                if mask.any():
                    seen.add(name)
    assert seen == {"behind", "near", "outside", "partly", "clamped", "r0"}, seen
    # one voxel with three classes: the same f32 depth, the lowest cell index keeps every pixel; a farther voxel behind it loses where they overlap
    M = mats["scaled"]
    lone = np.zeros_like(dense[:1])
    lone[0, 2, 2, 1, :] = True
    zl = R.splat(lone, M, OK_, 0.4, 3, 0.1, OH, OW)
    n0 = ((2 * 5 + 2) * 4 + 1) * 3
    assert set(int(k) for k in np.unique(zl & np.uint64(0xFFFFFFFF))) == {n0, 0xFFFFFFFF}
    far = np.zeros_like(dense[:1])
    far[0, 2, 2, 3, 2] = True
    covered = zl != R.EMPTY_KEY
    assert (R.splat(far, M, OK_, 0.4, 3, 0.1, OH, OW)[covered] != R.EMPTY_KEY).any()
    assert np.array_equal(R.splat(lone | far, M, OK_, 0.4, 3, 0.1, OH, OW)[covered], zl[covered])


def test_overlay_default_half_extent(gpu_device, overlay_scene):
    from soccdpt_amd.utils.occupancy_views import default_half_extent, occupancy_overlay
    dense, frames = overlay_scene
    M = _overlay_matrices()["model"]
    assert abs(default_half_extent(M) - 1.0) < 1e-6          # cells of 1 x 1 x 2 m
    bits = _bits(R.pack(dense[:1]), gpu_device)
    got = occupancy_overlay(bits, torch.from_numpy(frames[0]).to(gpu_device), M, np.array([[12.0, 0, 20.0], [0, 11.0, 12.0], [0, 0, 1]]), OG, COLORS[:OC], num_classes=OC)
    _same(got, R.resolve(R.splat(dense[:1], M, OK_, default_half_extent(M), 12, 0.1, OH, OW), frames[:1], COLORS[:OC], OC, 160))


# ---- through the model ----
def test_model_views(gpu_device):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import class_2_color as DEFAULT_CLASS_2_COLOR
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.occupancy_views import BEV, bev_iou, occupancy_overlay, occupancy_panel, occupancy_view
    from soccdpt_amd.utils.metrics import occupancy_pictures
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    net = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True)
    net.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    net = net.eval().to(gpu_device)
    frames = torch.randint(0, 256, (net.height, net.width, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    with pytest.raises(RuntimeError, match="occupancy_overlay"):
        net.occupancy_overlay(frames)
    with pytest.raises(RuntimeError, match="occupancy_view"):
        net.occupancy_view()
    with torch.no_grad():
        _, _, _, occ = net(synth_input(2, size=256).to(gpu_device))
    g, C = net.grid_size, net.num_classes
    assert torch.equal(net.occupancy_view(), occupancy_view(net.last_occ_bits, g, DEFAULT_CLASS_2_COLOR, num_classes=C, **BEV))
    for b in (0, 1):
        assert torch.equal(net.occupancy_view(frame=b, zoom=1), occupancy_view(net.last_occ_frame_bits[b], g, DEFAULT_CLASS_2_COLOR, num_classes=C, zoom=1, **BEV))
    assert tuple(net.occupancy_view().shape) == (1, 64, 512, 3)
    want = occupancy_overlay(net.last_occ_frame_bits[1], frames, net.voxel_to_camera(), (net.fx, net.fy, net.cx, net.cy), g, DEFAULT_CLASS_2_COLOR, num_classes=C)
    over = net.occupancy_overlay(frames, frame=1)
    assert torch.equal(over, want) and tuple(over.shape) == (1, net.height, net.width, 3)
    if int(net.last_occ_frame_bits[1].ne(0).sum()):
        assert not torch.equal(over[0], frames)              # occupied voxels in front of the camera are drawn
    # the packed row and the dense row of the forward describe the same grid
    assert torch.equal(occupancy_view(occ[1], g, DEFAULT_CLASS_2_COLOR, num_classes=C, **BEV), net.occupancy_view(frame=1))
    iou = bev_iou(net.last_occ_frame_bits, net.last_occ_frame_bits, g, num_classes=C)
    present = iou["counts"][..., 1] > 0
    assert torch.equal(iou["iou_per_class"] > 0.999999, present) and torch.equal(iou["iou_per_class"] == 0, ~present)
    # the panel: each tile is the primitive's picture with R and B exchanged
    rows = net.last_occ_frame_bits
    panel = occupancy_panel(frames, rows[0], rows[1], voxel_to_camera=net.voxel_to_camera(), intrinsics=(net.fx, net.fy, net.cx, net.cy), grid_size=g,
                            class_2_color=DEFAULT_CLASS_2_COLOR, num_classes=C)
    H, W = net.height, net.width
    assert tuple(panel.shape) == (H + 32 * 7, 2 * W, 3)
    assert torch.equal(panel[:H, W:], want[0].flip(-1))
    bev = occupancy_view(rows[0], g, DEFAULT_CLASS_2_COLOR, num_classes=C, zoom=7, **BEV)[0].flip(-1)
    assert torch.equal(panel[H:, 64:64 + 1792], bev) and int(panel[H:, :64].max()) == 0
    pics = occupancy_pictures(net, frames.unsqueeze(0), occ[1:], occ[:1], DEFAULT_CLASS_2_COLOR)
    assert set(pics) == {"plot_occupancy"} and np.array_equal(pics["plot_occupancy"], panel.cpu().numpy())


# ---- through the script ----
BASE = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", "/nonexistent"]


def _png_size(path):
    head = open(path, "rb").read(24)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    return int.from_bytes(head[20:24], "big"), int.from_bytes(head[16:20], "big")      # (height, width)


def test_eval_script_occupancy_views_flag(gpu_device, capsys, tmp_path):
    from soccdpt_amd.scripts.eval_SOccDPT import OCCUPANCY_VIEW_DIRS, build_parser, main
    from tests.visualise_refs import png_decode
    assert build_parser().parse_args(BASE + ["--occupancy-views"]).occupancy_views == os.path.join("media", "occupancy_views")
    root = str(tmp_path / "views")
    r = main(build_parser().parse_args(BASE + ["--occupancy-views", root]))
    out = capsys.readouterr().out
    assert "BEV_IOU: " in out and "IOU_3D: " in out                 # the flag implies --occupancy
    assert r["occupancy_views"] == root and 0.0 <= r["bev_iou"] <= 1.0 and "iou_3D" in r
    assert sorted(os.listdir(root)) == sorted(OCCUPANCY_VIEW_DIRS) == ["Occ_BEV", "Occ_Overlay", "Occ_Panel"]
    sizes = {"Occ_BEV": (64, 1024), "Occ_Overlay": (1080, 3840), "Occ_Panel": (1080 + 224, 3840)}
    for d, size in sizes.items():
        assert sorted(os.listdir(os.path.join(root, d))) == [f"{i:04d}.png" for i in range(10)]
        for i in range(10):
            assert _png_size(os.path.join(root, d, f"{i:04d}.png")) == size, (d, i)
    # prediction left, ground truth right; the panel's overlays are the overlay picture's halves
    over = png_decode(open(os.path.join(root, "Occ_Overlay", "0000.png"), "rb").read())
    panel = png_decode(open(os.path.join(root, "Occ_Panel", "0000.png"), "rb").read())
    assert np.array_equal(panel[:1080], over)


def test_eval_script_without_the_occupancy_views_flag(gpu_device, capsys, tmp_path, monkeypatch):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    monkeypatch.chdir(tmp_path)
    assert build_parser().parse_args(BASE).occupancy_views is None
    r = main(build_parser().parse_args(BASE))
    assert "bev_iou" not in r and "occupancy_views" not in r and "BEV_IOU" not in capsys.readouterr().out
    assert not os.listdir(tmp_path)
