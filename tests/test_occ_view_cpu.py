"""CPU: what the occupancy grid pictures need without a GPU: include/soccdpt_occ_view.h against soccdpt_amd.lib.OCC_VIEW_PROTOTYPES and the built
library, that the forward path's source hash did not move, the CPU-tensor refusals, the numpy restatements of tests/occ_view_refs.py against
hand-written cases, and voxel_to_camera() of the model and of the ground-truth generator against their forward mappings in oracle/."""
import ctypes
import glob
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import occ_view_refs as R
# the header / table comparison is the one of test_prototype_table_matches_the_header, so it uses that module's two classifiers
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("soccdpt_occ_view_columns", "soccdpt_occ_view_paint", "soccdpt_occ_view_iou2d", "soccdpt_occ_view_splat", "soccdpt_occ_view_resolve")


# ---- the sixth header and its table ----
def _occ_view_header():
    text = open(os.path.join(REPO, "include", "soccdpt_occ_view.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out


def test_occ_view_prototype_table_matches_the_header():
    from soccdpt_amd import lib
    header = _occ_view_header()
    assert tuple(header) == NAMES
    assert list(lib.OCC_VIEW_PROTOTYPES) == list(header), "the table follows the header's order"
    others = set(lib.PROTOTYPES) | set(lib.VIS_PROTOTYPES) | set(lib.DATA_PROTOTYPES) | set(lib.PACK_PROTOTYPES) | set(lib.SWIN1_PROTOTYPES)
    assert not set(lib.OCC_VIEW_PROTOTYPES) & others
    for name, (restype, argtypes) in lib.OCC_VIEW_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"


def test_occ_view_symbols_exported_and_typed():
    from soccdpt_amd.lib import ABI_VERSION, LIB_PATH, OCC_VIEW_PROTOTYPES, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _occ_view_header():
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_occ_view.h but not exported"
    L = load_library()
    for name, (restype, argtypes) in OCC_VIEW_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert ABI_VERSION == 13 and L.soccdpt_abi_version() == 13      # a sixth header, not a new version of the first


def test_forward_source_hash_did_not_move_for_occ_view():
    from soccdpt_amd.lib import FORWARD_SOURCES, csrc_sha
    assert "occ_view.hip" not in FORWARD_SOURCES and "occ_view.h" not in FORWARD_SOURCES
    newest = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_pmc_traffic.json")))[-1]
    assert json.load(open(newest))["csrc_sha"] == csrc_sha()
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "occ_view.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0]


def test_bad_arguments_are_refused_before_any_launch():
    """The refusals that need no device memory: every launcher checks its scalars first and names its entry point in soccdpt_last_error(NULL)."""
    from soccdpt_amd.lib import load_library
    L = load_library()
    g = (ctypes.c_int32 * 3)(2, 3, 4)
    M, K = (ctypes.c_double * 12)(), (ctypes.c_double * 4)(1, 1, 0, 0)
    bg = (ctypes.c_uint8 * 3)(0, 0, 0)
    one = 16      # a non-null pointer value: the scalar checks come first, nothing is dereferenced
    cases = {
        "soccdpt_occ_view_columns": [(one, 1, g, 3, 3, 0, one, one, one, one, None), (one, 1, g, 0, 1, 0, one, one, one, one, None),
                                     (one, 1, g, 9, 1, 0, one, one, one, one, None), (None, 1, g, 3, 1, 0, one, one, one, one, None),
                                     (one, 0, g, 3, 1, 0, one, one, one, one, None), (one, 1, (ctypes.c_int32 * 3)(65536, 65536, 1), 3, 1, 0, one, one, one, one, None)],
        "soccdpt_occ_view_paint": [(one, one, 1, 2, 3, 4, 0, one, 3, bg, 0, 0, 0, 0, 0, one, 3, 0, 6, 6, None), (one, one, 1, 2, 3, 4, 0, one, 3, bg, 193, 1, 0, 0, 0, one, 3, 0, 6, 6, None),
                                   (one, one, 1, 2, 3, 4, 0, one, 3, bg, -1, 1, 0, 0, 0, one, 3, 0, 6, 6, None), (one, one, 1, 2, 3, 4, 0, one, 9, bg, 0, 1, 0, 0, 0, one, 3, 0, 6, 6, None),
                                   (one, one, 1, 2, 3, 4, 0, one, 3, bg, 0, 1, 0, 0, 0, one, 3, 0, 6, 5, None), (one, one, 1, 2, 3, 4, 0, one, 3, bg, 0, 1, 0, 0, 0, one, 2, 0, 6, 6, None),
                                   (None, one, 1, 2, 3, 4, 0, one, 3, bg, 0, 1, 0, 0, 0, one, 3, 0, 6, 6, None)],
        "soccdpt_occ_view_iou2d": [(one, 2, one, 3, 6, 3, one, None), (one, 1, one, 3, 6, 0, one, None), (one, 1, one, 3, 6, 3, None, None)],
        "soccdpt_occ_view_splat": [(one, 1, g, 3, M, K, 0.5, 12, 0.1, 0, 8, one, None), (one, 1, g, 3, M, K, 0.5, 12, 0.1, 8, 0, one, None),
                                   (one, 1, g, 3, M, K, 0.5, -1, 0.1, 8, 8, one, None), (one, 1, g, 3, M, K, 0.5, 257, 0.1, 8, 8, one, None),
                                   (one, 1, g, 0, M, K, 0.5, 12, 0.1, 8, 8, one, None), (one, 1, g, 3, None, K, 0.5, 12, 0.1, 8, 8, one, None)],
        "soccdpt_occ_view_resolve": [(one, None, 1, 1, 4, 4, 3, one, 257, one, 4, 0, 16, 16, None), (one, None, 1, 1, 4, 4, 3, one, -1, one, 4, 0, 16, 16, None),
                                     (one, None, 1, 1, 0, 4, 3, one, 160, one, 4, 0, 16, 16, None), (one, None, 1, 1, 4, 4, 3, one, 160, one, 4, 1, 16, 16, None),
                                     (one, one, 2, 3, 4, 4, 3, one, 160, one, 4, 0, 16, 48, None), (None, None, 1, 1, 4, 4, 3, one, 160, one, 4, 0, 16, 16, None)],
    }
    assert tuple(cases) == NAMES
    for name, argsets in cases.items():
        for args in argsets:
            assert getattr(L, name)(*args) != 0, (name, args)
            assert name.encode() in L.soccdpt_last_error(None), (name, args, L.soccdpt_last_error(None))


def test_cpu_tensors_raise():
    from soccdpt_amd.utils import occupancy_views as V
    g, colors = (2, 3, 4), {0: (1, 2, 3), 1: (4, 5, 6), 2: (7, 8, 9)}
    dense, bits = torch.zeros((1,) + g + (3,)), torch.zeros((1, 3), dtype=torch.int32)
    frame = torch.zeros((6, 8, 3), dtype=torch.uint8)
    M, K = np.eye(3, 4), (1.0, 1.0, 0.0, 0.0)
    for grid in (dense, bits):
        with pytest.raises(RuntimeError):
            V.occupancy_columns(grid, g)
        with pytest.raises(RuntimeError):
            V.occupancy_view(grid, g, colors)
        with pytest.raises(RuntimeError):
            V.bird_eye_view(grid, g, colors)
        with pytest.raises(RuntimeError):
            V.bev_iou(grid, grid, g)
        with pytest.raises(RuntimeError):
            V.occupancy_overlay(grid, frame, M, K, g, colors)
        with pytest.raises(RuntimeError):
            V.occupancy_overlay(grid, None, M, K, g, colors, size=(6, 8))
        with pytest.raises(RuntimeError):
            V.occupancy_panel(frame, grid, grid, voxel_to_camera=M, intrinsics=K, grid_size=g, class_2_color=colors)


# ---- the numpy restatements against hand-written cases ----
G, C = (2, 3, 4), 3
CORNERS = [(i0, i1, i2) for i0 in (0, 1) for i1 in (0, 2) for i2 in (0, 3)]
CORNER_CLASS = {c: k % 3 for k, c in enumerate(CORNERS)}      # (0,0,0):0 (0,0,3):1 (0,2,0):2 (0,2,3):0 (1,0,0):1 (1,0,3):2 (1,2,0):0 (1,2,3):1


def _corner_grid():
    d = np.zeros((1,) + G + (C,), dtype=bool)
    for c, k in CORNER_CLASS.items():
        d[(0,) + c + (k,)] = True
    return d


def test_refs_pack_layout():
    d = np.zeros((1, 5, 7, 3, 3), dtype=bool)
    d[0, 0, 0, 0, 1] = d[0, 0, 3, 1, 2] = d[0, 4, 6, 2, 2] = True           # cells 1, 32, 314
    for garbage in (False, True):
        w = R.pack(d, tail_garbage=garbage)
        assert w.shape == (1, 10) and w.dtype == np.uint32
        assert w[0, 0] == 2 and w[0, 1] == 1 and (w[0, 9] & ((1 << 27) - 1)) == 1 << 26 and (w[0, 9] >> 27) == (31 if garbage else 0)


def test_refs_columns_on_the_corner_grid():
    """One cell per corner of a 2 x 3 x 4 grid: a column through two corners has first = its near end, count 2, top = the near corner's class and both
    corners' class bits; every other column is empty.  Written out from the corner list, for the three axes and both directions."""
    d = _corner_grid()
    for axis in (0, 1, 2):
        rest = [i for i in range(3) if i != axis]
        for from_high in (False, True):
            top, first, count, classes = R.columns(d, axis, from_high)
            assert top.shape == first.shape == count.shape == classes.shape == (1, G[rest[0]], G[rest[1]])
            want = {}
            for corner, k in CORNER_CLASS.items():
                col = (corner[rest[0]], corner[rest[1]])
                near = corner[axis] == (G[axis] - 1 if from_high else 0)
                w = want.setdefault(col, dict(count=0, classes=0))
                w["count"] += 1
                w["classes"] |= 1 << k
                if near:
                    w["first"], w["top"] = corner[axis], k
            assert len(want) == 4
            for a in range(G[rest[0]]):
                for b in range(G[rest[1]]):
                    got = (int(top[0, a, b]), int(first[0, a, b]), int(count[0, a, b]), int(classes[0, a, b]))
                    w = want.get((a, b))
                    assert got == ((w["top"], w["first"], 2, w["classes"]) if w else (255, -1, 0, 0)), (axis, from_high, a, b, got)
    # spelled out once: looking along axis 2 from its low end
    top, first, count, classes = R.columns(d, 2, False)
    assert top[0].tolist() == [[0, 255, 2], [1, 255, 0]] and first[0].tolist() == [[0, -1, 0], [0, -1, 0]]
    assert count[0].tolist() == [[2, 0, 2], [2, 0, 2]] and classes[0].tolist() == [[0b011, 0, 0b101], [0b110, 0, 0b011]]
    top, first, _, _ = R.columns(d, 2, True)
    assert top[0].tolist() == [[1, 255, 0], [2, 255, 1]] and first[0].tolist() == [[3, -1, 3], [3, -1, 3]]
    # two classes in one cell: the highest wins
    d[0, 0, 0, 0, 2] = True
    assert R.columns(d, 2, False)[0][0, 0, 0] == 2


def test_refs_paint_by_hand():
    top = np.array([[[1, 255], [0, 2]]], dtype=np.uint8)
    first = np.array([[[3, -1], [0, 1]]], dtype=np.int32)
    colors, bg = [(10, 20, 30), (200, 100, 50), (255, 255, 255)], (32, 33, 34)
    img = R.paint(top, first, 4, False, colors, bg, 192, 1, False, False, False)
    # rank 3 of 3: w = 256 - 192 = 64 -> (200*64+128)>>8 = 50, (100*64+128)>>8 = 25, (50*64+128)>>8 = 13; rank 1: w = 192 -> (255*192+128)>>8 = 191
    assert img[0].tolist() == [[[50, 25, 13], list(bg)], [[10, 20, 30], [191, 191, 191]]]
    hi = R.paint(top, first, 4, True, colors, bg, 192, 1, False, False, False)
    assert hi[0, 0, 0].tolist() == [200, 100, 50] and hi[0, 1, 0].tolist() == [3, 5, 8]      # rank 3: (10*64+128)>>8 = 3, (20*64+128)>>8 = 5, (30*64+128)>>8 = 8
    z = R.paint(top, first, 4, False, colors, bg, 0, 2, True, False, True)
    assert z.shape == (1, 4, 4, 3) and z[0, 0, 0].tolist() == [10, 20, 30] and z[0, 1, 3].tolist() == [200, 100, 50] and z[0, 2, 2].tolist() == list(bg)
    one = R.paint(top, first, 1, False, colors, bg, 192, 1, False, False, False)              # depth_len 1: no division by zero, rank 0
    assert one[0, 0, 0].tolist() == [200, 100, 50]


def test_refs_iou2d_by_hand():
    p = np.array([[[0b011, 0b000, 0b100]]], dtype=np.uint8)
    g = np.array([[[0b001, 0b010, 0b100]], [[0, 0, 0]]], dtype=np.uint8)
    assert R.iou2d(p, g, 3).tolist() == [[[1, 1, 1, 1], [0, 2, 1, 1], [1, 1, 1, 1]], [[0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0]]]


def test_refs_overlay_two_voxels_on_one_pixel():
    """Two voxels on the optical axis (X = Y = 0 for every cell, Z = i2 + 0.5): both land on pixel (cy, cx) = (2, 3); the nearer one's key stays."""
    d = np.zeros((1, 2, 3, 4, 3), dtype=bool)
    d[0, 1, 2, 3, 0] = True       # Z = 3.5, n = ((1*3+2)*4+3)*3 + 0 = 69
    d[0, 0, 1, 1, 2] = True       # Z = 1.5, n = ((0*3+1)*4+1)*3 + 2 = 17
    M = np.zeros((3, 4))
    M[2, 2] = 1.0
    z = R.splat(d, M, (10.0, 10.0, 3.0, 2.0), 0.0, 12, 0.1, 5, 6)
    want = np.full((1, 5, 6), R.EMPTY_KEY, dtype=np.uint64)
    want[0, 2, 3] = (0x3FC00000 << 32) | 17
    assert np.array_equal(z, want)
    # the same f32 depth: the lower cell index wins; a radius of one pixel, clipped by the frame's edge
    d[0, 0, 1, 1, 0] = True       # n = 15
    z = R.splat(d, M, (10.0, 10.0, 5.0, 2.0), 0.3, 12, 0.1, 5, 6)      # r = floor(0.3 / 1.5 * 10) = floor(1.99..) = 1 for the near pair, floor(0.857) = 0 for the far voxel
    assert z[0, 2, 5] == (0x3FC00000 << 32) | 15 and (z[0, 1:4, 4:6] == z[0, 2, 5]).all() and (z[0, :, :4] == R.EMPTY_KEY).all() and (z[0, 0] == R.EMPTY_KEY).all()
    img = R.resolve(z, np.full((1, 5, 6, 3), 100, dtype=np.uint8), [(0, 0, 0), (0, 0, 0), (255, 255, 255)], 3, 128)
    assert img[0, 2, 5].tolist() == [50, 50, 50] and img[0, 0, 0].tolist() == [100, 100, 100]           # n = 15 is class 0: (100*128 + 0 + 128) >> 8 = 50
    assert R.resolve(z, None, [(9, 9, 9)] * 3, 3, 256)[0, 2, 5].tolist() == [9, 9, 9] and R.resolve(z, None, [(9, 9, 9)] * 3, 3, 256)[0, 0, 0].tolist() == [0, 0, 0]
    behind = R.splat(d, -M, (10.0, 10.0, 3.0, 2.0), 0.0, 12, 0.1, 5, 6)
    assert (behind == R.EMPTY_KEY).all()


# ---- voxel_to_camera against the forward mappings ----
ANGLES = (7.0, -3.0, 5.0)
GRID, SCALE = (256, 256, 32), (2.0, 2.0, 0.666)
HALF_DIAGONAL = 0.5 * math.sqrt(sum((1.0 / s) ** 2 for s in SCALE))       # 0.829 m


def _centres(M, ijk, offset=0.5):
    return (np.asarray(ijk, dtype=np.float64) + offset) @ M[:, :3].T + M[:, 3]


def _inside(ijk, g):
    return ((ijk > 0) & (ijk < np.asarray(g))).all(axis=1)


def test_model_voxel_to_camera_inverts_the_projection(tmp_path):
    """Seeded camera points through oracle/soccdpt_ref.py:project + points_to_occupancy give each point's voxel; voxel_to_camera() of that voxel's
    centre, rotated forward again, lies within half a cell diagonal (+ 1e-3 m for the f32 forward path) of the rotated point."""
    from oracle import soccdpt_ref as O
    from soccdpt_amd.model.SOccDPT import SOccDPT
    from soccdpt_amd.utils.occupancy_views import model_voxel_to_camera
    from soccdpt_amd.utils.synth import write_synth_calib
    assert abs(HALF_DIAGONAL - 0.829) < 1e-3
    cam = O.Camera(fx=60.0, fy=60.0, cx=2.0, cy=2.0, width=80, height=60)
    cfg = O.ProjConfig(grid_size=GRID, scale=SCALE, correction_angle=ANGLES)
    gen = torch.Generator().manual_seed(11)
    depth = 3.0 + 42.0 * torch.rand((1, cam.height, cam.width), generator=gen)
    _, _, points, occ = O.project(1.0 / depth, torch.ones((1, 3, cam.height, cam.width)), cam, cfg)
    ra, rb, rc = O.rotation_matrices(ANGLES)
    q = points.reshape(1, -1, 3)
    for r in (ra, rb, rc):                      # the einsum of project(), on the points it returned
        q = torch.einsum("bnm,mj->bnj", q, r)
    q = q[0]
    ijk = (q / torch.tensor(cfg.occupancy_shape()) * torch.tensor(GRID, dtype=torch.float32)).type(torch.int64).numpy()
    keep = _inside(ijk, GRID)
    assert set(map(tuple, ijk[keep])) == set(map(tuple, (occ[0].sum(-1) > 0).nonzero().numpy())), "the test's voxel indices are points_to_occupancy's"
    keep[:3] = False           # the three points the reference's pc_scale quirk moves: ignored by voxel_to_camera()
    assert keep.sum() > 2000
    net = SOccDPT(camera_intrinsics_yaml=write_synth_calib(str(tmp_path / "calib.yaml")), grid_size=GRID, scale=SCALE, correction_angle=ANGLES)
    M = net.voxel_to_camera()
    assert M.shape == (3, 4) and M.dtype == np.float64
    Rf = ra.double().numpy() @ rb.double().numpy() @ rc.double().numpy()
    qd = q.double().numpy()[keep]

    def worst(matrix, offset=0.5):
        return float(np.linalg.norm(qd - _centres(matrix, ijk[keep], offset) @ Rf, axis=1).max())

    bound = HALF_DIAGONAL + 1e-3
    assert worst(M) <= bound
    # two seeded defects: the rotation applied in the wrong direction, and the voxel's corner instead of its centre
    from soccdpt_amd.lib import host_rotation_matrices
    rot = host_rotation_matrices(ANGLES).reshape(3, 3, 3)
    backwards = model_voxel_to_camera(GRID, net.occupancy_shape, np.stack([r.T for r in rot]).reshape(-1))
    assert worst(backwards) > bound
    assert worst(M, offset=0.0) > bound
    reordered = model_voxel_to_camera(GRID, net.occupancy_shape, rot[::-1].reshape(-1))       # Rc Rb Ra
    assert not np.allclose(reordered, M, atol=1e-4)


def test_processor_voxel_to_camera_inverts_the_generator():
    """The same for OccupancyProcessor against oracle/cref.py's ground-truth generator: its `points` are the scaled, shifted and rotated points."""
    from oracle import cref
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    from soccdpt_amd.utils.occupancy_views import processor_voxel_to_camera
    H, W, f = 60, 80, 60.0
    pc_scale, pc_shift = (1.5, 0.8, 1.0), (10.0, 5.0, 0.5)
    P = cref.gt_params(H, W, 3, f, f, 2.0, 2.0, grid_size=GRID, scale=SCALE, pc_scale=pc_scale, pc_shift=pc_shift, threshold=0, angles=ANGLES)
    rng = np.random.default_rng(12)
    depth = 3.0 + 42.0 * rng.random((H, W))
    out = cref.gt_occupancy((P.base_focal / depth).astype(np.float32), np.zeros((H, W), dtype=np.int32), P)
    q = out["points"]
    ijk = np.trunc(q / np.array(list(P.occ_shape), dtype=np.float64) * np.array(GRID, dtype=np.float64)).astype(np.int64)
    keep = _inside(ijk, GRID)
    assert set(map(tuple, ijk[keep])) == set(map(tuple, np.argwhere(out["counts"][..., 0] > 0))), "the test's voxel indices are the generator's"
    keep[: (H // 2) * W] = False          # the hidden upper half of the frame: depth 0, every point the shift alone
    assert keep.sum() > 2000
    proc = OccupancyProcessor(intrinsic_matrix=[[f, 0, 2.0], [0, f, 2.0], [0, 0, 1]], height=H, width=W, grid_size=GRID, scale=SCALE, shift=(0, 0, 0),
                              pc_scale=pc_scale, pc_shift=pc_shift, point_count_threshold=0, correction_angle=ANGLES)
    M = proc.voxel_to_camera()
    assert M.shape == (3, 4) and M.dtype == np.float64
    T = cref.gt_rot_matrices(ANGLES).reshape(3, 3, 3)
    Tf = T[0] @ T[1] @ T[2]

    def worst(matrix, offset=0.5):
        back = (_centres(matrix, ijk[keep], offset) * np.array(pc_scale) + np.array(pc_shift)) @ Tf
        return float(np.linalg.norm(q[keep] - back, axis=1).max())

    bound = HALF_DIAGONAL + 1e-3
    assert worst(M) <= bound
    backwards = processor_voxel_to_camera(GRID, proc.occupancy_shape, pc_scale, pc_shift, np.stack([t.T for t in T]).reshape(-1))
    assert worst(backwards) > bound
    assert worst(M, offset=0.0) > bound
    # the camera-space points themselves: un-rotate, un-shift, un-scale of the generator's points
    cam = (q[keep] @ np.linalg.inv(Tf) - np.array(pc_shift)) / np.array(pc_scale)
    assert np.abs(cam[:, 2] - depth.reshape(-1)[keep]).max() < 1e-3
