"""GPU: soccdpt_gt_occupancy (csrc/gt_occ.hip), bit for bit.

Two layers.  (1) test_gt_occupancy_matches_reference_golden / test_gt_occupancy_batch_vs_c_oracle: the processor against the golden recorded from the
reference's own OccupancyProcessor.process_frame and against the C oracle on a second, larger frame pair, at the reference's one geometry (grid
(256, 256, 32), rotation (7, 0, 0), threshold 10, C = 3, even H).  (2) One call at a time through the C entry point at the geometries and inputs of
tests/gt_occ_refs.py (tests/test_gt_occ_refs.py is the CPU companion: the numpy restatement of the reference's expressions equals the C oracle on every row,
every edge is reached, every named defect changes an output bit): frames of 2 x 1, 3 x 5 (odd H), 7 x 63, 8 x 65 with B = 3 (batch boundaries inside waves),
16 x 64 (constructed run patterns: a run of exactly 64, one ending at lane 63, one spanning two waves, every lane a head, A A x x A A), 37 x 53 (a count
equal to its threshold) and 1040 x 2048 (past the 8192-block cap: the loop's second round, most lanes idle); grids (256, 256, 32), (33, 21, 7), (2, 2, 2) and
(1, 1, 1); C = 1, 3, 5; thresholds 10, 0, 0.5, -1; rotations (7, 3, -2) and (5, -4, 9); a negative pc_scale; disparities +-0, NaN, +-inf, denormal, negative
and one that sends the voxel coordinate past 9e18; class ids -1, C, 255 and INT32_MIN (outside [0, C): they contribute nothing); and three rows recorded
from the reference's own process_frame at other cameras, grids, scales, pc_scale / pc_shift, thresholds and C (tests/golden/gt_occupancy_geoms.npz).
Depth, all points, counts and grid equal the C oracle's (and the goldens') bit for bit.

Per call: outputs are 0xFF bytes beforehand; a 4 KB 0xFF guard sits behind every operand and output; afterwards every guard and operand is untouched, a
second call gives the same bits, and the call without the optional depth / points outputs gives the same counts and grid.  A refused call launches nothing
and leaves every output at its sentinel.  A HIP error ends the session.  No kernel was found wrong."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import cref
from tests import gt_occ_refs as R
from tests.golden_inputs import gt_occ_inputs
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "gt_occupancy.npz"))
GEOMS = np.load(os.path.join(os.path.dirname(__file__), "golden", "gt_occupancy_geoms.npz"))


def _proc(K, H, W, C):
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    return OccupancyProcessor(intrinsic_matrix=K, height=H, width=W, grid_size=(256, 256, 32), scale=(2.0, 2.0, 0.666), shift=(0.0, 0.0, 0.0),
                              pc_scale=(500.0, 2500.0, 200.0), pc_shift=(100.0, 40.0, 0.0), point_count_threshold=10, num_classes=C)


def test_gt_occupancy_matches_reference_golden(gpu_device):
    disp, seg, K, H, W, C = gt_occ_inputs()
    r = _proc(K, H, W, C).process(torch.from_numpy(disp).to(gpu_device), torch.from_numpy(seg).to(gpu_device))
    torch.cuda.synchronize()
    grid = np.unpackbits(G["grid_bits"])[: int(np.prod(G["grid_shape"]))].reshape(G["grid_shape"]).astype(bool)
    assert np.array_equal(r["occupancy_grid"][0].cpu().numpy(), grid)
    assert np.array_equal(r["depth"][0].cpu().numpy().view(np.uint32), G["depth"].view(np.uint32))
    assert np.array_equal(r["points"][0].cpu().numpy()[G["point_rows"]], G["points_sample"])


def test_gt_occupancy_batch_vs_c_oracle(gpu_device):
    frames = [gt_occ_inputs(H=540, W=960, seed=s) for s in (3, 4)]
    K, H, W, C = frames[0][2], 540, 960, 3
    disp = np.stack([f[0] for f in frames])
    seg = np.stack([f[1] for f in frames])
    r = _proc(K, H, W, C).process(torch.from_numpy(disp).to(gpu_device), torch.from_numpy(seg).to(gpu_device))
    torch.cuda.synchronize()
    P = cref.gt_params(H, W, C, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    for b in range(2):
        o = cref.gt_occupancy(disp[b], seg[b].astype(np.int32), P)
        assert o["grid"].sum() > 100
        assert np.array_equal(r["occupancy_grid"][b].cpu().numpy(), o["grid"])
        assert np.array_equal(r["counts"][b].cpu().numpy().astype(np.uint32), o["counts"])
        assert np.array_equal(r["depth"][b].cpu().numpy().view(np.uint32), o["depth"].view(np.uint32))
        assert np.array_equal(r["points"][b].cpu().numpy(), o["points"])


# ---------------- one call at a time at the geometries of tests/gt_occ_refs.py ----------------
@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


def _arrays(g):
    K = R.intrinsics(g)
    arr = lambda vals, t: (t * len(vals))(*vals)
    occ_shape = [float(np.float32(float(g.grid[k] / R.scale_of(g)[k]))) for k in range(3)]
    return (arr([K[0, 0], K[1, 1], K[0, 2], K[1, 2], 1.0 * 10 ** -2], ctypes.c_double), arr(list(g.pc_scale), ctypes.c_double), arr(list(g.pc_shift), ctypes.c_double),
            arr([float(v) for v in cref.gt_rot_matrices(g.angles)], ctypes.c_double), arr(occ_shape, ctypes.c_float), arr(list(g.grid), ctypes.c_int))


def run(g, disp, seg, dev, optional=True):
    """One soccdpt_gt_occupancy over guarded buffers -> dict of host arrays (depth / points None without `optional`)."""
    from soccdpt_amd.lib import _call, load_library
    L = load_library()
    d, s = torch.from_numpy(disp), torch.from_numpy(seg)
    ins = dict(disparity=Buf(d.shape, torch.float32, dev, d), seg_class=Buf(s.shape, torch.int32, dev, s))
    cells = (g.B, *g.grid, g.C)
    outs = dict(counts=Buf(cells, torch.int32, dev), occ=Buf(cells, torch.uint8, dev))
    if optional:
        outs.update(depth=Buf((g.B, g.H, g.W), torch.float32, dev), points=Buf((g.B, g.H * g.W, 3), torch.float64, dev))
    ptr = lambda k: outs[k].ptr() if k in outs else None
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    _call("soccdpt_gt_occupancy", g.B, g.H, g.W, g.C, *_arrays(g), float(g.threshold), ins["disparity"].ptr(), ins["seg_class"].ptr(), ptr("depth"), ptr("points"),
          ptr("counts"), ptr("occ"), device=dev)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_gt_occupancy ({g.name}): {e}", returncode=3)
    assert int(L.soccdpt_launch_counter()) - before == 2
    for k, b in {**ins, **outs}.items():
        assert b.guard_untouched(), f"{g.name}: the guard behind {k} was written"
    assert R.same_bits(ins["disparity"].t.cpu().numpy(), disp) and R.same_bits(ins["seg_class"].t.cpu().numpy(), seg), f"{g.name}: an operand was written"
    got = {k: b.t.cpu().numpy() for k, b in outs.items()}
    return dict(depth=got.get("depth"), points=got.get("points"), counts=got["counts"].view(np.uint32), grid=got["occ"])


def check(name, got, want):
    assert set(np.unique(got["grid"]).tolist()) <= {0, 1}, f"{name}: the grid holds bytes other than 0 and 1"
    assert np.array_equal(got["counts"], want["counts"]), f"{name}: {int((got['counts'] != want['counts']).sum())} counts differ"
    assert np.array_equal(got["grid"].astype(bool), want["grid"]), f"{name}: the grid differs"
    if got["depth"] is not None:
        assert R.same_bits(got["depth"], want["depth"]), f"{name}: depth differs"
        assert R.same_bits(got["points"], want["points"]), f"{name}: points differ"


@pytest.mark.parametrize("name", list(R.BY_NAME))
def test_gt_occupancy_row(dev, name):
    g, disp, seg = R.inputs(name)
    want = R.c_oracle(g, disp, seg)
    got = run(g, disp, seg, dev)
    check(name, got, want)
    again = run(g, disp, seg, dev)
    assert all(R.same_bits(got[k], again[k]) for k in got), f"{name}: two calls differ"
    bare = run(g, disp, seg, dev, optional=False)
    check(name, bare, want)
    assert R.same_bits(bare["counts"], got["counts"]) and R.same_bits(bare["grid"], got["grid"])
    if name in R.NO_OCCUPIED:
        assert not got["counts"].any()
    else:
        assert got["grid"].any()
    print(f"MEASURED {name}: bitwise; {int(got['grid'].sum())} occupied cells, largest count {int(got['counts'].max())}")


@pytest.mark.parametrize("g", R.GOLDEN, ids=lambda g: g.name)
def test_gt_occupancy_reference_goldens(dev, g):
    _, disp, seg = R.inputs(g.name)
    got = run(g, disp, seg, dev)
    key = g.name.replace(" ", "_")
    shape = tuple(GEOMS[key + "/grid_shape"])
    grid = np.unpackbits(GEOMS[key + "/grid_bits"])[: int(np.prod(shape))].reshape(shape).astype(bool)
    assert np.array_equal(got["grid"][0].astype(bool), grid) and grid.any()
    assert R.same_bits(got["depth"][0], GEOMS[key + "/depth"])
    assert R.same_bits(got["points"][0], GEOMS[key + "/points"])


def test_gt_occupancy_refusals_write_nothing(dev):
    from soccdpt_amd.lib import load_library
    L = load_library()
    g = R.BY_NAME["2x1 grid 2"]
    arena = Buf((8, 1 << 16), torch.uint8, dev)                  # 0xFF; every device pointer of the refused calls points into it
    P = lambda r: arena.ptr() + (1 << 16) * r
    assert g.B * R.ncell(g) * 4 <= 1 << 16
    good = [g.B, g.H, g.W, g.C, *_arrays(g), float(g.threshold), P(0), P(1), P(2), P(3), P(4), P(5)]
    bad = {}
    for i, label in ((0, "B"), (1, "H"), (2, "W"), (3, "C")):
        for v in (0, -1):
            bad[f"{label} = {v}"] = good[:i] + [v] + good[i + 1:]
    for i, label in ((4, "intrinsics"), (5, "pc_scale"), (6, "pc_shift"), (7, "rotations"), (8, "occupancy shape"), (9, "grid size"), (11, "disparity"),
                     (12, "seg_class"), (15, "counts"), (16, "occ")):
        bad[f"null {label}"] = good[:i] + [None] + good[i + 1:]
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    for label, args in bad.items():
        assert L.soccdpt_gt_occupancy(*args, None) == 1, f"accepted: {label}"
        assert b"gt_occupancy" in L.soccdpt_last_error(None)
        torch.cuda.synchronize()
        assert int(L.soccdpt_launch_counter()) == before, f"{label}: a refused call launched a kernel"
        assert bool((arena.raw == 0xFF).all()), f"{label}: a refused call wrote"
    assert len(bad) == 18


def test_gt_processor_at_another_grid_and_class_count(dev):
    """OccupancyProcessor.process with want_occupancy_points at a grid of (33, 21, 7), C = 5 (the constructor's default and every other processor test have 3),
    threshold 0.5 and general correction angles: grid, counts, depth and points equal the C oracle's, and the point list equals the reference's own expression
    evaluated on those counts (>= threshold, class-major), with more than one class id in it."""
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    g, disp, seg = R.processor_case()
    assert g.C == 5 and g.grid == (33, 21, 7)
    want = R.c_oracle(g, disp, seg)
    proc = OccupancyProcessor(intrinsic_matrix=R.intrinsics(g), height=g.H, width=g.W, grid_size=g.grid, scale=R.scale_of(g), shift=(0.0, 0.0, 0.0), pc_scale=g.pc_scale,
                              pc_shift=g.pc_shift, point_count_threshold=g.threshold, num_classes=g.C, correction_angle=g.angles)
    r = proc.process(torch.from_numpy(disp).to(dev), torch.from_numpy(seg).to(dev), want_occupancy_points=True)
    torch.cuda.synchronize()
    assert np.array_equal(r["occupancy_grid"].cpu().numpy(), want["grid"]) and np.array_equal(r["counts"].cpu().numpy().view(np.uint32), want["counts"])
    assert R.same_bits(r["depth"].cpu().numpy(), want["depth"]) and R.same_bits(r["points"].cpu().numpy(), want["points"])
    assert len(r["occupancy_points"]) == g.B
    for b, p in enumerate(r["occupancy_points"]):
        ref = R.occupancy_points_ref(want["counts"][b], g)
        assert len(ref) > 10 and len(set(ref[:, 3].tolist())) > 1, f"row {b}: the expected point list is trivial"
        assert p.dtype == torch.float64 and R.same_bits(p.cpu().numpy(), ref), f"row {b}: the occupancy point list differs"
