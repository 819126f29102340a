"""CPU: the numpy specification of the occupancy-evaluation layer (tests/occ_eval_refs.py) is bit-equal to lists recorded from the reference's own
occupancy_grid_to_points and transform_points_to_occupancy_grid_vect (tests/golden/occ_points.npz, written by tests/tools/make_golden_occ_points.py);
the library exports the new entry points; the Python layer imports and refuses CPU tensors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import occ_eval_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "occ_points.npz"))
CASES = ("default", "odd", "small", "empty")
SYMBOLS = ("soccdpt_occ_pack", "soccdpt_occ_points_scratch_bytes", "soccdpt_occ_points_count", "soccdpt_occ_points_write", "soccdpt_occ_iou_counts")


@pytest.mark.parametrize("case", CASES)
def test_spec_equals_reference_list(case):
    grid = [int(v) for v in G[case + "_grid"]]
    want = G[case + "_points"]
    got = R.points_from_bits(G[case + "_bits"], grid[:3], tuple(G[case + "_scale"]), grid[3])
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape and want.shape[1] == 4
    assert np.array_equal(got, want)


def test_fixture_covers_what_it_should():
    assert tuple(G["default_grid"]) == (256, 256, 32, 3) and 15000 < G["default_points"].shape[0] < 23000
    assert tuple(G["odd_grid"]) == (48, 40, 12, 3) and G["odd_points"].shape[0] > 15000
    assert tuple(G["small_grid"]) == (5, 7, 3, 3) and tuple(G["small_scale"]) == (1.5, 0.7, 0.666)
    assert int(G["small_bits"][-1]) >> (315 & 31) == (1 << (32 - (315 & 31))) - 1, "the padding bits of the 315-cell grid are set on purpose"
    assert G["empty_points"].shape == (0, 4) and G["empty_points"].dtype == np.float64
    # on the non-power-of-two grid the f32 shortcut i * shape / g is NOT what the reference computes; the double form is
    g, scale = (48, 40, 12), tuple(G["odd_scale"])
    shape = R.occupancy_shape_f32(g, scale)
    differs = False
    for ax in range(3):
        i = np.arange(g[ax])
        shortcut = (i.astype(np.float32) * shape[ax] / np.float32(g[ax])).astype(np.float32)
        differs |= not np.array_equal(shortcut, (i / g[ax] * shape[ax].astype(np.float64)).astype(np.float32))
    assert differs


def test_spec_equals_reference_gt_list():
    """The list transform_points_to_occupancy_grid_vect returned for the gt_occ_inputs() frame == the spec applied to counts >= 10, with the
    counts of the C oracle of the GT-occupancy kernel; and the `>` grid of the existing golden is the strictly smaller set."""
    from oracle import cref
    from tests.golden_inputs import gt_occ_inputs
    disp, seg, K, H, W, C = gt_occ_inputs()
    o = cref.gt_occupancy(disp, seg.astype(np.int32), cref.gt_params(H, W, C, K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    counts = o["counts"].astype(np.int64)
    got = R.points_from_mask(counts >= 10, (256, 256, 32), (2.0, 2.0, 0.666), C)
    assert np.array_equal(got, G["gt_points"]) and got.dtype == G["gt_points"].dtype
    assert int((counts > 10).sum()) == int(G["gt_grid_cells"][0]) == 1810 < got.shape[0]


def test_pack_unpack_roundtrip_and_padding():
    rng = np.random.default_rng(0)
    m = rng.random(315) < 0.5
    w = R.pack_bits(m)
    assert w.dtype == np.uint32 and w.size == 10 and int(w[-1]) >> (315 & 31) == 0
    assert np.array_equal(R.unpack_bits(w, 315), m)
    assert np.array_equal(R.unpack_bits(w.view(np.int32), 315), m)
    assert np.array_equal(R.class_counts(m, 3), np.array([m[c::3].sum() for c in range(3)]))


def test_library_exports_the_occupancy_entry_points():
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(so)
    for n in SYMBOLS:
        assert hasattr(lib, n), n
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    for n in SYMBOLS:
        assert n + "(" in header, f"{n} is not declared in include/soccdpt_hip.h"
    from soccdpt_amd.lib import load_library
    L = load_library()
    assert L.soccdpt_abi_version() >= 7
    # the scratch query is host arithmetic: offsets (u64, one per (row, class, workgroup of 1024 words) + 1) and the block counts (u32)
    nblk = (256 * 256 * 32 * 3 // 32 + 1023) // 1024
    assert L.soccdpt_occ_points_scratch_bytes(2, 256 * 256 * 32 * 3, 3) == (2 * 3 * nblk + 1) * 8 + 2 * 3 * nblk * 4
    assert L.soccdpt_occ_points_scratch_bytes(1, 96, 9) == 0 and L.soccdpt_occ_points_scratch_bytes(0, 96, 3) == 0


def test_python_layer_imports_and_has_no_cpu_fallback():
    from soccdpt_amd.utils import occupancy as O
    for name in ("occupancy_grid_to_points", "occupancy_bits_to_points", "pack_occupancy", "occupancy_iou", "semantic_pc_to_colors_and_pc"):
        assert callable(getattr(O, name))
    from soccdpt_amd.model.SOccDPT import SOccDPT
    assert callable(SOccDPT.occupancy_points)
    from soccdpt_amd.utils.metrics import evaluate_occupancy
    assert callable(evaluate_occupancy)
    with pytest.raises(RuntimeError):
        O.occupancy_grid_to_points(torch.zeros(4, 4, 4, 3))
    with pytest.raises(RuntimeError):
        O.pack_occupancy(torch.zeros(4, 4, 4, 3))
    with pytest.raises(RuntimeError):
        O.occupancy_bits_to_points(torch.zeros(6, dtype=torch.int32), (4, 4, 4), (2.0, 2.0, 0.666))
    with pytest.raises(RuntimeError):
        O.occupancy_iou(torch.zeros(6, dtype=torch.int32), torch.zeros(6, dtype=torch.int32))


def test_iou_host_formula_on_two_voxel_grids():
    C = 3

    def grid(*cells):       # cells: (voxel, class) of a 2-voxel grid
        m = np.zeros((2, C), dtype=bool)
        for v, c in cells:
            m[v, c] = True
        return m
    a = grid((0, 0), (1, 0))
    same = R.iou_counts(a, a, C)
    assert same.tolist() == [[2, 2, 2, 2], [0, 0, 0, 0], [0, 0, 0, 0]]
    per, mean = R.iou_from_counts(same)
    assert per[0] == 2 / (2 + 1e-7) and per[1] == 0.0 and per[2] == 0.0 and abs(per[0] - 1.0) < 1e-7      # identical -> 1 (up to the epsilon)
    assert mean == per.mean()
    per, _ = R.iou_from_counts(R.iou_counts(grid((0, 0)), grid((1, 0)), C))                               # disjoint -> 0
    assert per.tolist() == [0.0, 0.0, 0.0]
    # 1/3 needs three voxels: class 1 predicted in {v0, v1}, true in {v1, v2}
    p = np.zeros((3, C), dtype=bool)
    g = np.zeros((3, C), dtype=bool)
    p[0, 1] = p[1, 1] = True
    g[1, 1] = g[2, 1] = True
    cnt = R.iou_counts(p, g, C)
    assert cnt[1].tolist() == [1, 3, 2, 2]
    per, mean = R.iou_from_counts(cnt)
    assert abs(per[1] - 1.0 / 3.0) < 1e-7 and per[0] == 0.0
    empty = R.iou_counts(np.zeros((2, C), bool), np.zeros((2, C), bool), C)                                # empty union -> 0, finite
    per, mean = R.iou_from_counts(empty)
    assert per.tolist() == [0.0, 0.0, 0.0] and mean == 0.0 and np.isfinite(mean)
