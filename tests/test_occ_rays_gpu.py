"""GPU: the observed-space ray caster and the masked 3-D IoU (csrc/occ_rays.hip) against tests/occ_rays_refs.py, bit for bit and count for count;
the arena around the mask and the refusals; and the path through OccupancyProcessor.process(want_observed=True), the model and the script."""
import ctypes
import math
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import occ_rays_refs as R

pytestmark = pytest.mark.gpu
CASES = [c["name"] for c in R.TABLE]
PAD = 64      # int32 words of 0xFF behind the last row


def _i32(words: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).to(dev)


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def refs():
    """The restatement's masks, computed once for every test of the module."""
    return {c["name"]: R.observed_ref(c) for c in R.TABLE}


def _launch(case, dev, arena: torch.Tensor, clear: bool):
    from soccdpt_amd.utils.occupancy_rays import observed_voxels_raw
    rows, nvw = case["rows"], R.nvw_of(case["g"])
    out = arena[: rows * nvw].view(rows, nvw)
    observed_voxels_raw(torch.from_numpy(case["depth"]).to(dev), case["N"], case["K"], case["g"], case["z_near"], case["max_depth"] or None, case["step"], out, clear)
    return out


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_restatement(gpu_device, refs, name):
    case = R.BY_NAME[name]
    rows, nvw, nvox = case["rows"], R.nvw_of(case["g"]), R.nvox_of(case["g"])
    arena = torch.full((rows * nvw + PAD,), -1, dtype=torch.int32, device=gpu_device)
    beyond = np.uint32(0) if nvox % 32 == 0 else np.uint32((0xFFFFFFFF << (nvox % 32)) & 0xFFFFFFFF)
    if case["init"] is not None:      # clear = 0 onto pre-set bits; the bits past the grid in a row's last word are set and must stay so
        init = case["init"].copy()
        init[:, -1] |= beyond
        arena[: rows * nvw] = _i32(init, gpu_device).reshape(-1)
    got = _u32(_launch(case, gpu_device, arena, clear=case["init"] is None))
    want = refs[name].copy()
    if case["init"] is not None:
        want[:, -1] |= beyond
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {got.size} words differ"
    assert bool((arena[rows * nvw:] == -1).all()), "words behind the last row were written"
    if case["init"] is None:
        assert not (got[:, -1] & beyond).any(), "a bit past the grid was set"
        # the same launch again without clearing changes nothing; onto ones it leaves ones
        again = _u32(_launch(case, gpu_device, arena, clear=False))
        assert np.array_equal(again, want)
        arena[: rows * nvw] = -1
        assert bool((_launch(case, gpu_device, arena, clear=False) == -1).all())


def test_python_entry_inverts_and_allocates(gpu_device, refs):
    from soccdpt_amd.utils.occupancy_rays import observed_voxels
    case = R.BY_NAME["processor 33x2x40, 24x16, step 2"]
    M = R.invert(case["N"])           # the inverse of an affine map, by the same formula: a voxel-centre -> camera matrix
    depth = torch.from_numpy(case["depth"]).to(gpu_device)
    got = observed_voxels(depth, M, case["K"], case["g"], z_near=case["z_near"], step=case["step"])
    assert got.dtype == torch.int32 and tuple(got.shape) == (case["rows"], R.nvw_of(case["g"]))
    again = R.observed_ref(dict(case, N=R.invert(M)))
    assert np.array_equal(_u32(got), again)
    assert np.array_equal(_u32(observed_voxels(depth[0], M, case["K"], case["g"], z_near=case["z_near"], step=case["step"])), again[:1])
    out = torch.zeros_like(got)
    out[:, 0] = 0x5
    assert observed_voxels(depth, M, case["K"], case["g"], z_near=case["z_near"], step=case["step"], out=out) is out
    want = again.copy()
    want[:, 0] |= 0x5
    assert np.array_equal(_u32(out), want)
    with pytest.raises(ValueError):
        observed_voxels(depth, M, case["K"], case["g"], out=out[:, :-1])
    K3 = np.array([[case["K"][0], 0, case["K"][2]], [0, case["K"][1], case["K"][3]], [0, 0, 1]])
    assert torch.equal(observed_voxels(depth, M, K3, case["g"], z_near=case["z_near"], step=case["step"]), got)


def test_refusals_launch_nothing_and_write_nothing(gpu_device):
    from soccdpt_amd.lib import _stream_ptr, load_library
    L = load_library()
    case = R.BY_NAME["outside 5x7x3, 65x3"]
    rows, H, W, g = case["rows"], case["H"], case["W"], case["g"]
    depth = torch.from_numpy(case["depth"]).to(gpu_device)
    mask = torch.full((rows * R.nvw_of(g) + PAD,), -1, dtype=torch.int32, device=gpu_device)
    f64 = ctypes.POINTER(ctypes.c_double)
    arr = lambda v, n: (ctypes.c_double * n)(*np.asarray(v, dtype=np.float64).reshape(-1))
    nan, inf = float("nan"), float("inf")
    ok = dict(depth=depth.data_ptr(), rows=rows, H=H, W=W, grid=(ctypes.c_int32 * 3)(*g), N=arr(case["N"], 12), K=arr(case["K"], 4), z_near=0.0, max_depth=0.0,
              step=1, clear=1, mask=mask.data_ptr())
    Nbad, Kbad = case["N"].copy(), case["K"].copy()
    Nbad[1, 2], Kbad[3] = nan, inf
    bad = [dict(depth=None), dict(mask=None), dict(grid=None), dict(N=None), dict(K=None), dict(rows=0), dict(H=0), dict(W=-1), dict(step=0),
           dict(grid=(ctypes.c_int32 * 3)(2048, 2048, 512)), dict(N=arr(Nbad, 12)), dict(K=arr(Kbad, 4)), dict(K=arr([0.0, 1.0, 0.0, 0.0], 4)),
           dict(K=arr([1.0, 0.0, 0.0, 0.0], 4)), dict(z_near=-1.0)]
    torch.cuda.synchronize(gpu_device)
    before = L.soccdpt_launch_counter()
    stream = _stream_ptr(gpu_device)
    for change in bad:
        assert L.soccdpt_occ_rays_observed(*dict(ok, **change).values(), stream) != 0, change
        assert b"soccdpt_occ_rays_observed" in L.soccdpt_last_error(None)
    counts = torch.full((rows * 3 * 4 + PAD,), -1, dtype=torch.int64, device=gpu_device)
    nobs = torch.full((rows + PAD,), -1, dtype=torch.int64, device=gpu_device)
    bits = torch.zeros((rows, (R.nvox_of(g) * 3 + 31) // 32), dtype=torch.int32, device=gpu_device)
    ok2 = dict(pred=bits.data_ptr(), pred_rows=rows, gt=bits.data_ptr(), rows=rows, nvox=R.nvox_of(g), C=3, mask=mask.data_ptr(), mask_rows=rows, include_gt=1,
               counts=counts.data_ptr(), observed=nobs.data_ptr())
    bad2 = [dict(pred=None), dict(gt=None), dict(mask=None), dict(counts=None), dict(rows=0), dict(nvox=0), dict(nvox=1 << 31), dict(C=0), dict(C=9),
            dict(pred_rows=rows + 1), dict(mask_rows=rows + 1)]
    for change in bad2:
        assert L.soccdpt_occ_iou_counts_masked(*dict(ok2, **change).values(), stream) != 0, change
        assert b"soccdpt_occ_iou_counts_masked" in L.soccdpt_last_error(None)
    assert L.soccdpt_launch_counter() == before
    torch.cuda.synchronize(gpu_device)
    assert bool((mask == -1).all()) and bool((counts == -1).all()) and bool((nobs == -1).all())
    # and the good call of each launches exactly one kernel
    assert L.soccdpt_occ_rays_observed(*ok.values(), stream) == 0 and L.soccdpt_launch_counter() == before + 1
    assert L.soccdpt_occ_iou_counts_masked(*ok2.values(), stream) == 0 and L.soccdpt_launch_counter() == before + 2
    torch.cuda.synchronize(gpu_device)
    assert bool((mask[rows * R.nvw_of(g):] == -1).all()) and bool((counts[rows * 12:] == -1).all()) and bool((nobs[rows:] == -1).all())


# ---- masked IoU ----
def _random_words(rng, rows, n, density):
    w = np.zeros((rows, n), dtype=np.uint32)
    for _ in range(density):
        w |= rng.randint(0, 2 ** 32, size=(rows, n), dtype=np.uint64).astype(np.uint32)
    return w


def _masked(pred, gt, mask, nvox, C, include_gt, dev, want_observed=True):
    from soccdpt_amd.lib import _call, _ptr
    p, q, m = _i32(pred, dev), _i32(gt, dev), _i32(mask, dev)
    rows = gt.shape[0]
    counts = torch.full((rows * C * 4 + PAD,), -1, dtype=torch.int64, device=dev)
    nobs = torch.full((rows + PAD,), -1, dtype=torch.int64, device=dev)
    _call("soccdpt_occ_iou_counts_masked", _ptr(p), pred.shape[0], _ptr(q), rows, nvox, C, _ptr(m), mask.shape[0], 1 if include_gt else 0, _ptr(counts),
          _ptr(nobs) if want_observed else None, device=dev)
    assert bool((counts[rows * C * 4:] == -1).all()) and bool((nobs[rows if want_observed else 0:] == -1).all())
    return counts[: rows * C * 4].view(rows, C, 4).cpu().numpy(), nobs[:rows].cpu().numpy()


@pytest.mark.parametrize("g,C", [((5, 7, 3), 3), ((3, 3, 3), 8), ((33, 2, 40), 1), ((9, 11, 13), 5), ((64, 64, 32), 3)])
@pytest.mark.parametrize("rows,pred_rows,mask_rows", [(1, 1, 1), (3, 3, 3), (3, 1, 3), (3, 3, 1), (2, 1, 1)])
def test_masked_iou_against_numpy(gpu_device, g, C, rows, pred_rows, mask_rows):
    from soccdpt_amd.utils.occupancy import occupancy_iou
    nvox = R.nvox_of(g)
    nwords, nvw = (nvox * C + 31) // 32, (nvox + 31) // 32
    rng = np.random.RandomState(nvox + 7 * C + rows + 3 * pred_rows + 5 * mask_rows)
    pred = _random_words(rng, pred_rows, nwords, 1) & _random_words(rng, pred_rows, nwords, 1)      # a quarter of the bits, the ones past the grid included
    gt = _random_words(rng, rows, nwords, 1) & _random_words(rng, rows, nwords, 1) & _random_words(rng, rows, nwords, 1)
    mask = _random_words(rng, mask_rows, nvw, 1)
    for include_gt in (False, True):
        counts, nobs = _masked(pred, gt, mask, nvox, C, include_gt, gpu_device)
        want_counts, want_obs = R.iou_masked_ref(pred, gt, mask, nvox, C, include_gt)
        assert np.array_equal(counts, want_counts) and np.array_equal(nobs, want_obs), (include_gt, counts, want_counts)
    assert np.array_equal(_masked(pred, gt, mask, nvox, C, True, gpu_device, want_observed=False)[0], want_counts)
    # an all-ones mask: soccdpt_occ_iou_counts exactly
    ones = np.full((1, nvw), 0xFFFFFFFF, dtype=np.uint32)
    counts, nobs = _masked(pred, gt, ones, nvox, C, False, gpu_device)
    plain = occupancy_iou(_i32(pred, gpu_device), _i32(gt, gpu_device), num_classes=C, grid_size=g)["counts"].cpu().numpy()
    assert np.array_equal(counts, plain) and nobs.tolist() == [nvox] * rows
    # an all-zero mask: nothing without include_gt, any-class(gt) with it
    zeros = np.zeros((1, nvw), dtype=np.uint32)
    counts, nobs = _masked(pred, gt, zeros, nvox, C, False, gpu_device)
    assert not counts.any() and not nobs.any()
    counts, nobs = _masked(pred, gt, zeros, nvox, C, True, gpu_device)
    anyclass = np.stack([np.packbits(np.pad(R.unpack(gt[r], nvox * C).reshape(nvox, C).any(axis=1), (0, nvw * 32 - nvox)), bitorder="little").view(np.uint32) for r in range(rows)])
    counts2, nobs2 = _masked(pred, gt, anyclass, nvox, C, False, gpu_device)
    assert np.array_equal(counts, counts2) and np.array_equal(nobs, nobs2) and np.array_equal(counts[..., 3], plain[..., 3])


def test_occupancy_iou_observed_and_apply_observed(gpu_device):
    from soccdpt_amd.utils.occupancy import occupancy_iou, pack_occupancy
    from soccdpt_amd.utils.occupancy_rays import apply_observed, occupancy_iou_observed
    g, C, rows = (5, 7, 3), 3, 2
    nvox = R.nvox_of(g)
    rng = np.random.RandomState(4)
    pd, gd = rng.rand(rows, *g, C) < 0.3, rng.rand(rows, *g, C) < 0.2
    mv = rng.rand(rows, nvox) < 0.5
    mask = np.stack([np.packbits(np.pad(mv[r], (0, R.nvw_of(g) * 32 - nvox)), bitorder="little").view(np.uint32) for r in range(rows)])
    pt, gtt, mt = torch.from_numpy(pd).to(gpu_device), torch.from_numpy(gd).to(gpu_device), _i32(mask, gpu_device)
    pb, gb = pack_occupancy(pt), pack_occupancy(gtt)
    for include_gt in (True, False):
        m = mv | gd.reshape(rows, nvox, C).any(axis=2) if include_gt else mv
        p, q = pd.reshape(rows, nvox, C) & m[..., None], gd.reshape(rows, nvox, C) & m[..., None]
        want = np.stack([(p & q).sum(1), (p | q).sum(1), p.sum(1), q.sum(1)], axis=2)
        for a, b, kw in ((pt, gtt, {}), (pb, gb, dict(grid_size=g)), (pt, gb, {})):
            res = occupancy_iou_observed(a, b, mt, num_classes=C, include_gt=include_gt, **kw)
            assert set(res) == set(occupancy_iou(pt, gtt, num_classes=C)) | {"observed_voxels", "observed_fraction"}
            assert np.array_equal(res["counts"].cpu().numpy(), want)
            assert res["observed_voxels"].tolist() == m.sum(1).tolist()
            assert np.allclose(res["observed_fraction"].cpu().numpy(), m.sum(1) / nvox, rtol=1e-15, atol=0)
            assert np.allclose(res["iou_per_class"].cpu().numpy(), want[..., 0] / (want[..., 1] + 1e-7), rtol=1e-15, atol=0)
    one_row = occupancy_iou_observed(pb[:1], gb, mt[0], num_classes=C, grid_size=g, include_gt=False)      # one prediction, one mask, two gt rows
    assert one_row["counts"].shape == (2, C, 4) and one_row["observed_voxels"].tolist() == [int(mv[0].sum())] * 2
    with pytest.raises(ValueError):
        occupancy_iou_observed(pb, gb, mt[:, :-1], num_classes=C, grid_size=g)
    with pytest.raises(ValueError):
        occupancy_iou_observed(pb, gb, mt, num_classes=C)        # 315 cells: the word count alone does not give the grid
    cleared = apply_observed(pb, mt, C, g)
    assert torch.equal(cleared, pack_occupancy(torch.from_numpy(pd & mv.reshape(rows, *g, 1)).to(gpu_device)))
    assert torch.equal(apply_observed(pt, mt, C, g), cleared)


# ---- end to end: a fronto-parallel wall through the generator ----
def test_wall_through_the_generator(gpu_device):
    """A wall at Z0 = 5 m in front of a 64 x 48 camera with f = 40 px, in a (32, 32, 16) grid of 0.5 m voxels aligned with the camera (no rotation,
    camera centre at voxel coordinate (16, 16, 0)).  The camera is chosen so that neighbouring rays are Z0 / f = 0.125 m apart at the wall: a quarter
    of a voxel, so no voxel the frustum covers can slip between two rays."""
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    from soccdpt_amd.utils.occupancy import pack_occupancy
    from soccdpt_amd.utils.occupancy_rays import occupancy_iou_observed
    H, W, f, Z0, g, cell = 48, 64, 40.0, 5.0, (32, 32, 16), 0.5
    cx, cy = W / 2 - 0.5, H / 2 - 0.5
    assert Z0 / f < cell
    proc = OccupancyProcessor(np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]]), H, W, g, scale=(1 / cell,) * 3, shift=(0, 0, 0), pc_scale=(1.0, 1.0, 1.0),
                              pc_shift=(8.0, 8.0, 0.0), point_count_threshold=0, num_classes=3, correction_angle=(0.0, 0.0, 0.0))
    disp = torch.full((2, H, W), 0.01 * f / Z0, dtype=torch.float32, device=gpu_device)
    seg = (torch.arange(W, device=gpu_device) // 22).to(torch.int32).expand(2, H, W).contiguous()
    out = proc.process(disp, seg, want_points=False, want_observed=True)
    depth, obs = out["depth"], out["observed"]
    assert tuple(obs.shape) == (2, R.nvw_of(g)) and obs.dtype == torch.int32
    assert bool((depth[:, : H // 2] == 0).all()) and bool(((depth[:, H // 2:] - Z0).abs() < 1e-5).all())
    assert "observed" not in proc.process(disp, seg, want_points=False)
    seen = np.stack([R.unpack(row, R.nvox_of(g)).reshape(g) for row in _u32(obs)])
    assert np.array_equal(seen[0], seen[1]) and seen.any()
    # camera coordinates of every voxel centre, through the generator's own matrix
    M = proc.voxel_to_camera()
    ijk = np.stack(np.meshgrid(*[np.arange(n) for n in g], indexing="ij"), axis=-1).reshape(-1, 3) + 0.5
    P = (ijk @ M[:, :3].T + M[:, 3]).reshape(*g, 3)
    diagonal = cell * math.sqrt(3.0)
    assert not seen[0][P[..., 2] > Z0 + diagonal].any(), "a voxel behind the wall was observed"
    with np.errstate(all="ignore"):
        u, v = f * P[..., 0] / P[..., 2] + cx, f * P[..., 1] / P[..., 2] + cy
    inside = (P[..., 2] > 0) & (u >= 0) & (u <= W - 1) & (v >= H // 2) & (v <= H - 1)
    must = inside & (P[..., 2] < Z0 - diagonal)
    assert must.sum() > 100 and seen[0][must].all(), "a voxel in front of the wall, inside the frustum, was not observed"
    # the hidden half of the frame observes nothing: its depth alone casts no ray, and nothing above the optical axis by more than a voxel is seen
    hidden = depth.clone()
    hidden[:, H // 2:] = 0
    assert not bool(proc.observed_voxels(hidden).any())
    assert not seen[0][P[..., 1] < -diagonal].any()
    # coarser steps see a subset
    assert not bool((proc.observed_voxels(depth, step=4) & ~obs).any())
    # the ground truth against itself over observed space: 1 per non-empty class
    gt = out["occupancy_grid"]
    res = occupancy_iou_observed(gt, gt, obs, num_classes=3)
    present = res["counts"][..., 3] > 0
    assert bool(present.any()) and bool((res["iou_per_class"][present] > 0.999999).all()) and bool((res["iou_per_class"][~present] == 0).all())
    # every occupied ground-truth voxel is observed by the rays alone here (the wall is where the rays end)
    alone = occupancy_iou_observed(gt, gt, obs, num_classes=3, include_gt=False)
    assert torch.equal(alone["counts"], res["counts"])
    assert bool((res["observed_fraction"] > 0).all()) and bool((res["observed_fraction"] < 0.5).all())


# ---- through the model and the script ----
def test_model_observed_voxels(gpu_device):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.occupancy_rays import camera_to_voxel
    from soccdpt_amd.utils.synth import write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    net = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True)
    rng = np.random.RandomState(2)
    depth = (2.0 + 40.0 * rng.rand(1, net.height, net.width)).astype(np.float32)
    depth[0, : net.height // 2] = np.inf
    step = 97
    got = net.observed_voxels(torch.from_numpy(depth).to(gpu_device), step=step, z_near=0.25, max_depth=30.0)
    case = dict(g=tuple(net.grid_size), rows=1, H=net.height, W=net.width, step=step, N=camera_to_voxel(net.voxel_to_camera()),
                K=np.array([net.fx, net.fy, net.cx, net.cy], dtype=np.float64), z_near=0.25, max_depth=30.0, depth=depth, init=None)
    want = R.observed_ref(case)
    assert want.any() and np.array_equal(_u32(got), want)


BASE = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "-d", "cuda:0", "-b", "/nonexistent"]


def test_eval_script_occupancy_observed_flag(gpu_device, capsys):
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser, main
    assert build_parser().parse_args(BASE).occupancy_observed is False
    r = main(build_parser().parse_args(BASE + ["--occupancy-observed"]))
    out = capsys.readouterr().out
    assert "IOU_3D: " in out and "IOU_3D_OBSERVED: " in out and "OBSERVED_FRACTION: " in out          # the flag implies --occupancy
    # with the ground truth's voxels in the mask the intersections are those of IOU_3D and the unions can only shrink
    assert 0.0 <= r["iou_3D"] <= r["iou_3D_observed"] <= 1.0
    assert 0.0 < r["observed_fraction"] < 1.0
