"""CPU: the observed-space ray caster without a GPU.  include/soccdpt_occ_rays.h against soccdpt_amd.lib.OCC_RAYS_PROTOTYPES and the built library;
the float64 restatement of tests/occ_rays_refs.py sandwiched between exact-arithmetic bounds; the shared traversal core (csrc/occ_rays_core.h)
compiled for the host under the sanitizers and compared with the restatement bit for bit; seven planted defects that the case table refuses; and
the caster's geometry against the ground-truth generator's own CPU statement (tests/gt_occ_refs.py)."""
import ctypes
import glob
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import gt_occ_refs as G
from tests import occ_rays_refs as R
# the header / table comparison is the one of test_prototype_table_matches_the_header, so it uses that module's two classifiers
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("soccdpt_occ_rays_observed", "soccdpt_occ_iou_counts_masked")
CASES = [c["name"] for c in R.TABLE]


# ---- the seventh header and its table ----
def _occ_rays_header():
    text = open(os.path.join(REPO, "include", "soccdpt_occ_rays.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out


def test_occ_rays_prototype_table_matches_the_header():
    from soccdpt_amd import lib
    header = _occ_rays_header()
    assert tuple(header) == NAMES
    assert list(lib.OCC_RAYS_PROTOTYPES) == list(header), "the table follows the header's order"
    others = (set(lib.PROTOTYPES) | set(lib.VIS_PROTOTYPES) | set(lib.DATA_PROTOTYPES) | set(lib.PACK_PROTOTYPES) | set(lib.SWIN1_PROTOTYPES)
              | set(lib.OCC_VIEW_PROTOTYPES))
    assert not set(lib.OCC_RAYS_PROTOTYPES) & others
    for name, (restype, argtypes) in lib.OCC_RAYS_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"


def test_occ_rays_symbols_exported_and_typed():
    from soccdpt_amd.lib import ABI_VERSION, LIB_PATH, OCC_RAYS_PROTOTYPES, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _occ_rays_header():
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_occ_rays.h but not exported"
    L = load_library()
    for name, (restype, argtypes) in OCC_RAYS_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert ABI_VERSION == 13 and L.soccdpt_abi_version() == 13      # a seventh header, not a new version of the first


def test_forward_source_hash_did_not_move_for_occ_rays():
    from soccdpt_amd.lib import FORWARD_SOURCES, csrc_sha
    assert not {"occ_rays.hip", "occ_rays.h", "occ_rays_core.h"} & set(FORWARD_SOURCES)
    newest = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_pmc_traffic.json")))[-1]
    assert json.load(open(newest))["csrc_sha"] == csrc_sha()
    for name in ("occ_rays.hip", "occ_rays_core.h"):       # the contract is float64 with every operation rounded on its own, whatever the flags
        src = open(os.path.join(REPO, "soccdpt_amd", "csrc", name)).read()
        assert "#pragma clang fp contract(off)" in src.split("#include")[0], name


def test_bad_arguments_are_refused_before_any_launch():
    """The refusals need no device memory: every check comes before anything is dereferenced or launched, and soccdpt_last_error(NULL) names the entry."""
    from soccdpt_amd.lib import load_library
    L = load_library()
    g = (ctypes.c_int32 * 3)(8, 8, 4)
    N, K = (ctypes.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), (ctypes.c_double * 4)(1, 1, 0, 0)
    one, nan, inf = 16, float("nan"), float("inf")         # a non-null pointer value: nothing is dereferenced
    ok = dict(depth=one, rows=1, H=4, W=4, grid=g, N=N, K=K, z_near=0.0, max_depth=0.0, step=1, clear=1, mask=one)
    bad = [dict(depth=None), dict(mask=None), dict(grid=None), dict(N=None), dict(K=None), dict(rows=0), dict(rows=-1), dict(H=0), dict(W=0), dict(step=0),
           dict(step=-2), dict(grid=(ctypes.c_int32 * 3)(2048, 2048, 512)), dict(grid=(ctypes.c_int32 * 3)(65536, 65536, 65536)),
           dict(grid=(ctypes.c_int32 * 3)(8, 0, 4)), dict(N=(ctypes.c_double * 12)(1, 0, 0, 0, 0, nan, 0, 0, 0, 0, 1, 0)),
           dict(N=(ctypes.c_double * 12)(1, 0, 0, inf, 0, 1, 0, 0, 0, 0, 1, 0)), dict(K=(ctypes.c_double * 4)(1, 1, nan, 0)),
           dict(K=(ctypes.c_double * 4)(-inf, 1, 0, 0)), dict(K=(ctypes.c_double * 4)(0, 1, 0, 0)), dict(K=(ctypes.c_double * 4)(1, 0, 0, 0)),
           dict(z_near=-0.5), dict(z_near=nan), dict(max_depth=nan)]
    before = L.soccdpt_launch_counter()
    for change in bad:
        a = dict(ok, **change)
        assert L.soccdpt_occ_rays_observed(*a.values(), None) != 0, change
        assert b"soccdpt_occ_rays_observed" in L.soccdpt_last_error(None), (change, L.soccdpt_last_error(None))
    ok = dict(pred=one, pred_rows=1, gt=one, rows=2, nvox=100, C=3, mask=one, mask_rows=2, include_gt=1, counts=one, observed=None)
    bad = [dict(pred=None), dict(gt=None), dict(mask=None), dict(counts=None), dict(rows=0), dict(nvox=0), dict(nvox=1 << 31), dict(C=0), dict(C=9),
           dict(pred_rows=3), dict(pred_rows=0), dict(mask_rows=3), dict(mask_rows=0)]
    for change in bad:
        a = dict(ok, **change)
        assert L.soccdpt_occ_iou_counts_masked(*a.values(), None) != 0, change
        assert b"soccdpt_occ_iou_counts_masked" in L.soccdpt_last_error(None), (change, L.soccdpt_last_error(None))
    assert L.soccdpt_launch_counter() == before


def test_cpu_tensors_raise():
    from soccdpt_amd.utils import occupancy_rays as O
    g = (2, 3, 4)
    M = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    dense, bits, mask = torch.zeros((1,) + g + (3,)), torch.zeros((1, 3), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32)
    with pytest.raises(RuntimeError):
        O.observed_voxels(torch.ones((1, 4, 4)), M, (1.0, 1.0, 0.0, 0.0), g)
    for grid in (dense, bits):
        with pytest.raises(RuntimeError):
            O.occupancy_iou_observed(grid, grid, mask, grid_size=g)
        with pytest.raises(RuntimeError):
            O.apply_observed(grid, mask, 3, g)


def test_camera_to_voxel_is_the_inverse_of_the_centre_map():
    from soccdpt_amd.utils.occupancy_rays import camera_to_voxel
    from soccdpt_amd.utils.occupancy_views import processor_voxel_to_camera
    rot_t = np.concatenate([m.T.reshape(-1) for m in G.rot_matrices((7.0, 3.0, -2.0))])
    M = processor_voxel_to_camera((33, 21, 7), np.array([128.0, 100.0, 48.0], dtype=np.float32), (500.0, 2500.0, 200.0), (100.0, 40.0, 12.0), rot_t)
    N = camera_to_voxel(M)
    assert N.shape == (3, 4) and N.dtype == np.float64 and N.flags["C_CONTIGUOUS"]
    assert np.array_equal(N, R.invert(M))
    ijk = np.array([[0, 0, 0], [32, 20, 6], [5, 17, 3]], dtype=np.float64)
    centre = ijk + 0.5                                                            # M takes the voxel-centre index ...
    cam = centre @ M[:, :3].T + M[:, 3]
    back = cam @ N[:, :3].T + N[:, 3]                                             # ... and N gives coordinates in which voxel i covers [i, i + 1)
    assert np.allclose(back, centre, rtol=0, atol=1e-9) and np.array_equal(np.floor(back), ijk)
    with pytest.raises(ValueError):
        camera_to_voxel(np.eye(4))


# ---- the restatement between exact bounds ----
@pytest.mark.parametrize("name", CASES)
def test_restatement_between_exact_bounds(name):
    """L_eps <= restatement <= U_eps per ray, eps = 2^-30 voxel, in fractions.Fraction on the float64 segment ends.  Crossing parameters are never
    accumulated, so they err by a few ulps of coordinates below 2^16: under 2^-34.  A violation is a defect of the contract or of the restatement."""
    assert R.EPS == 2 ** -30
    assert R.sandwich(R.BY_NAME[name]) == []


def test_exact_bounds_by_hand():
    # along the grid line x = 2, y = 1.5 from z = 0.5 to 2.5 in a 4 x 4 x 4 grid: the shrunk cubes of the two columns beside the line do not
    # meet it, the grown ones do
    S, E = [2.0, 1.5, 0.5], [2.0, 1.5, 2.5]
    idx = lambda i, j, k: (i * 4 + j) * 4 + k
    assert R.exact_voxels(S, E, (4, 4, 4), -R.EPS) == set()
    assert R.exact_voxels(S, E, (4, 4, 4), R.EPS) == {idx(i, 1, k) for i in (1, 2) for k in (0, 1, 2)}
    S, E = [2.25, 1.5, 0.5], [2.25, 1.5, 2.5]
    assert R.exact_voxels(S, E, (4, 4, 4), -R.EPS) == R.exact_voxels(S, E, (4, 4, 4), R.EPS) == {idx(2, 1, k) for k in (0, 1, 2)}


def test_restatement_by_hand():
    g, K = (8, 8, 4), (1.0, 1.0, 3.0, 2.0)
    N = R.axis_aligned((4.0, 4.0, 0.0))
    idx = lambda i, j, k: (i * 8 + j) * 4 + k
    # the central pixel looks along the grid line x = 4, y = 4: the voxels above and to the right of the line, up to the one holding z = 3
    assert R.cast_ray(N, K, g, 0.0, 0.0, 3, 2, 3.0) == [idx(4, 4, 0), idx(4, 4, 1), idx(4, 4, 2), idx(4, 4, 3)]
    # one pixel to the right, depth 2: the diagonal (4, 4, 0) -> (6, 4, 2) through two voxel edges; at each the lower axis steps first
    assert R.cast_ray(N, K, g, 0.0, 0.0, 4, 2, 2.0) == [idx(4, 4, 0), idx(5, 4, 0), idx(5, 4, 1), idx(6, 4, 1), idx(6, 4, 2)]
    # max_depth cuts the same ray at (5, 4, 1)
    assert R.cast_ray(N, K, g, 0.0, 1.0, 4, 2, 2.0) == [idx(4, 4, 0), idx(5, 4, 0), idx(5, 4, 1)]
    for d in (np.nan, np.inf, -np.inf, 0.0, -1.0):
        assert R.cast_ray(N, K, g, 0.0, 0.0, 4, 2, d) == []
    assert R.cast_ray(N, K, g, 2.0, 0.0, 4, 2, 2.0) == [] and R.cast_ray(N, K, g, 2.0, 0.0, 4, 2, np.float32(2.0000002)) != []
    assert R.cast_pixels(7, 1) == [0, 1, 2, 3, 4, 5, 6] and R.cast_pixels(7, 2) == [1, 3, 5] and R.cast_pixels(7, 3) == [1, 4] and R.cast_pixels(1, 2) == []


def test_the_table_reaches_its_cases():
    found = set()
    for c in R.TABLE:
        found |= R.placements(c)
    assert found == set(R.PLACEMENTS)
    assert {c["g"] for c in R.TABLE} == {(8, 8, 4), (5, 7, 3), (33, 2, 40), (256, 256, 32)}
    assert {(c["W"], c["H"]) for c in R.TABLE} == {(1, 1), (7, 5), (64, 1), (65, 3), (24, 16)}
    assert {c["step"] for c in R.TABLE} == {1, 2, 3} and {c["rows"] for c in R.TABLE} == {1, 2, 3}
    assert any(c["init"] is not None for c in R.TABLE) and any(c["max_depth"] > 0 for c in R.TABLE)
    seen = np.concatenate([c["depth"].reshape(-1) for c in R.TABLE])
    assert np.isnan(seen).any() and np.isposinf(seen).any() and np.isneginf(seen).any() and (seen == 0).any() and (seen < 0).any()
    assert any((c["depth"] == np.float32(c["z_near"])).any() and c["z_near"] > 0 for c in R.TABLE)
    assert any(c["max_depth"] > 0 and (c["depth"] > c["max_depth"]).any() for c in R.TABLE)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defects_are_refused(defect):
    refused = [c["name"] for c in R.TABLE if not np.array_equal(R.observed_ref(c, defect), R.observed_ref(c))]
    assert refused, f"no case of the table tells the restatement from one with: {defect}"


# ---- the shared core on the CPU ----
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("occ_rays") / "occ_rays_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(REPO, "tests", "occ_rays_main.cpp"), "-o", out]
    # gcc links the sanitizer runtimes as shared libraries unless told otherwise; linked into the program they need nothing from the loader.  Where the
    # static archives are not installed, the default link does
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout
    if is_clang or subprocess.run([*cmd, "-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return out


def _run_core(exe, case, tmp_path):
    src, dst = tmp_path / "case.bin", tmp_path / "mask.bin"
    g = case["g"]
    with open(src, "wb") as f:
        f.write(struct.pack("<8i", g[0], g[1], g[2], case["H"], case["W"], case["rows"], case["step"], 0 if case["init"] is None else 1))
        f.write(np.concatenate([case["N"].reshape(-1), case["K"], [case["z_near"], case["max_depth"]]]).astype("<f8").tobytes())
        f.write(case["depth"].astype("<f4").tobytes())
        if case["init"] is not None:
            f.write(case["init"].astype("<u4").tobytes())
    r = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr     # a sanitizer report goes to stderr and ends the program with a non-zero status
    return np.fromfile(dst, dtype="<u4").reshape(case["rows"], R.nvw_of(g)), int(r.stdout)


@pytest.mark.parametrize("name", CASES)
def test_core_equals_restatement(exe, tmp_path, name):
    case = R.BY_NAME[name]
    got, marked = _run_core(exe, case, tmp_path)
    want = R.observed_ref(case)
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} words differ"
    new = want & ~(np.uint32(0) if case["init"] is None else case["init"])
    assert marked >= sum(len(R.mask_to_set(row)) for row in new)         # every new bit was handed to the sink at least once


def test_core_survives_hostile_matrices(exe, tmp_path):
    """NaN, infinite and enormous matrices, a zero focal length: the core is also what keeps the kernel inside its buffer when the launcher's checks
    are bypassed.  Nothing may be reported by the sanitizers, and nothing is marked outside the grid (the program's buffer is exactly the mask)."""
    base = R.BY_NAME["outside 5x7x3, 65x3"]
    for k, (N, K) in enumerate([(np.full((3, 4), np.nan), base["K"]), (np.full((3, 4), np.inf), base["K"]), (base["N"] * 1e300, base["K"]),
                                (base["N"] * 1e-320, base["K"]), (base["N"], np.array([0.0, 0.0, 1.0, 1.0])), (-base["N"] * 3e9, base["K"])]):
        case = dict(base, N=np.ascontiguousarray(N, dtype=np.float64), K=np.asarray(K, dtype=np.float64))
        got, _ = _run_core(exe, case, tmp_path)
        assert np.array_equal(got, R.observed_ref(case)), k
        assert not (got[:, -1] >> np.uint32(R.nvox_of(case["g"]) % 32)).any()


# ---- masked IoU statement ----
def test_iou_masked_ref_by_hand():
    # 5 voxels, 2 classes, one row.  cells (voxel, class): pred = {(0,0), (1,1), (3,0), (4,1)}, gt = {(0,0), (1,0), (2,1), (4,1)}
    pack = lambda cells: np.array([[sum(1 << (v * 2 + c) for v, c in cells)]], dtype=np.uint32)
    pred, gt = pack([(0, 0), (1, 1), (3, 0), (4, 1)]), pack([(0, 0), (1, 0), (2, 1), (4, 1)])
    mask = np.array([[0b01011]], dtype=np.uint32)          # voxels 0, 1, 3
    counts, obs = R.iou_masked_ref(pred, gt, mask, 5, 2, False)
    assert obs.tolist() == [3] and counts.tolist() == [[[1, 3, 2, 2], [0, 1, 1, 0]]]
    counts, obs = R.iou_masked_ref(pred, gt, mask, 5, 2, True)      # + voxels 2 and 4 from the ground truth
    assert obs.tolist() == [5] and counts.tolist() == [[[1, 3, 2, 2], [1, 3, 2, 2]]]
    counts, obs = R.iou_masked_ref(pred, gt, np.zeros((1, 1), dtype=np.uint32), 5, 2, False)
    assert obs.tolist() == [0] and not counts.any()


# ---- units: the caster's geometry against the generator's CPU statement ----
def _dilate(occ):
    out = np.zeros_like(occ)
    p = np.pad(occ, 1)
    n0, n1, n2 = occ.shape
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out |= p[a: a + n0, b: b + n1, c: c + n2]
    return out


@pytest.mark.parametrize("name", ["golden 16x64", "golden 9x20"])
def test_generator_fills_only_observed_space(name):
    """Every voxel the generator's numpy statement fills (counts >= 1 in any class) lies in the restatement's observed set dilated by one voxel
    (26-neighbourhood): the generator's point of a pixel and the end of that pixel's ray are the same point up to rounding.  No exceptions."""
    g, disp, seg = G.inputs(name)
    ref = G.numpy_ref(disp, seg, g)
    K = G.intrinsics(g)
    shape = np.array([float(g.grid[k] / G.scale_of(g)[k]) for k in range(3)], dtype=np.float32)
    from soccdpt_amd.utils.occupancy_views import processor_voxel_to_camera
    rot_t = np.concatenate([m.T.reshape(-1) for m in G.rot_matrices(g.angles)])
    N = R.invert(processor_voxel_to_camera(g.grid, shape, g.pc_scale, g.pc_shift, rot_t))
    case = dict(g=tuple(g.grid), rows=g.B, H=g.H, W=g.W, step=1, N=N, K=np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]), z_near=0.0, max_depth=0.0,
                depth=ref["depth"], init=None)
    observed = R.observed_ref(case)
    filled_any = False
    for b in range(g.B):
        occ = R.unpack(observed[b], R.nvox_of(g.grid)).reshape(g.grid)
        filled = (ref["counts"][b] >= 1).any(axis=-1)
        filled_any |= bool(filled.any())
        outside = filled & ~_dilate(occ)
        assert not outside.any(), f"{name} row {b}: generator voxels {np.argwhere(outside)[:5].tolist()} lie outside observed space"
    assert filled_any
