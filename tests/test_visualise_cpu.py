"""CPU: what the evaluation pictures need without a GPU: the committed colour table against its derivation, the PNG writer, include/soccdpt_vis.h against
soccdpt_amd.lib.VIS_PROTOTYPES and the built library, the CPU-tensor refusals, and that the forward path's source hash did not move."""
import ctypes
import glob
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import visualise_refs as R
# the header / table comparison is the one of test_prototype_table_matches_the_header, so it uses that module's two classifiers; existing test
# files are left as they are, hence the import of its helpers instead of a move (a rename there has to be followed here)
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the colour table ----
def test_plasma_table_is_the_matplotlib_derivation():
    cm = pytest.importorskip("matplotlib._cm_listed")
    from soccdpt_amd.utils.visualise import PLASMA_BGR
    want = np.rint(255.0 * np.asarray(cm._plasma_data, dtype=np.float64)).astype(np.uint8)[:, ::-1]
    assert PLASMA_BGR.dtype == np.uint8 and PLASMA_BGR.shape == (256, 3) and np.array_equal(PLASMA_BGR, want)
    assert np.array_equal(R.LUT_BGR, PLASMA_BGR)


def test_plasma_table_anchor_entries():
    from soccdpt_amd.utils.visualise import PLASMA_BGR
    assert [tuple(int(v) for v in PLASMA_BGR[i, ::-1]) for i in (0, 128, 255)] == [(13, 8, 135), (204, 71, 120), (240, 249, 33)]


def test_plasma_table_is_what_cv2_applies():
    """Skipped where cv2 is not installed: parity with cv2.applyColorMap itself is then not pinned."""
    cv2 = pytest.importorskip("cv2")
    from soccdpt_amd.utils.visualise import PLASMA_BGR
    got = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(1, 256), cv2.COLORMAP_PLASMA)[0]
    assert np.array_equal(got, PLASMA_BGR)


# ---- PNG ----
def test_png_round_trip(tmp_path):
    from soccdpt_amd.utils.visualise import write_png
    img = np.random.default_rng(0).integers(0, 256, size=(9, 13, 3), dtype=np.uint8)
    for bgr, want in ((False, img), (True, img[:, :, ::-1])):
        path = str(tmp_path / f"a{int(bgr)}.png")
        write_png(path, torch.from_numpy(img) if bgr else img, bgr=bgr)
        data = open(path, "rb").read()
        assert data[:8] == bytes([0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A])
        assert np.array_equal(R.png_decode(data), want)
        try:
            from PIL import Image
        except ImportError:
            continue
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (13, 9) and np.array_equal(np.asarray(im), want)
    with pytest.raises(ValueError):
        write_png(str(tmp_path / "b.png"), np.zeros((4, 4), dtype=np.uint8))


# ---- the second header and its table ----
def _vis_header():
    text = open(os.path.join(REPO, "include", "soccdpt_vis.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out


def test_vis_prototype_table_matches_the_header():
    from soccdpt_amd.lib import PROTOTYPES, VIS_PROTOTYPES
    header = _vis_header()
    assert len(header) == 8 and all(n.startswith("soccdpt_vis_") for n in header)
    for n in ("soccdpt_vis_minmax", "soccdpt_vis_colorize", "soccdpt_vis_color_masks", "soccdpt_vis_resize", "soccdpt_vis_shrink_half"):
        assert n in header
    assert list(VIS_PROTOTYPES) == list(header), "the table follows the header's order"
    assert not set(VIS_PROTOTYPES) & set(PROTOTYPES)
    for name, (restype, argtypes) in VIS_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"


def test_vis_symbols_exported_and_typed():
    from soccdpt_amd.lib import ABI_VERSION, LIB_PATH, VIS_PROTOTYPES, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _vis_header():
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_vis.h but not exported"
    L = load_library()
    for name, (restype, argtypes) in VIS_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert ABI_VERSION == 13 and L.soccdpt_abi_version() == 13      # a second header, not a new version of the first


def test_host_side_entry_points():
    """The two entry points that launch nothing: tap tables and the half size, against the numpy specification; errors through soccdpt_last_error."""
    from soccdpt_amd.lib import load_library
    from soccdpt_amd.utils.visualise import half_size, resize_taps
    for src, dst in ((5, 9), (9, 5), (7, 7), (1, 4), (1080, 384), (384, 1920)):
        assert np.array_equal(resize_taps(src, dst), R.resize_taps(src, dst)), (src, dst)
    ident = resize_taps(7, 7)
    assert np.array_equal(ident[:, 0], np.arange(7)) and not ident[:, 2].any()
    L = load_library()
    for H, W in ((2, 2), (5, 7), (1080, 5760), (3, 9), (6, 10)):
        h, w = ctypes.c_int32(), ctypes.c_int32()
        assert L.soccdpt_vis_half_size(H, W, ctypes.byref(h), ctypes.byref(w)) == 0
        assert (h.value, w.value) == half_size(H, W) == R.half_size(H, W)
    assert half_size(5, 7) == (2, 4)
    assert L.soccdpt_vis_minmax_scratch_bytes(2, 1080 * 1920) == 2 * 1024 * 8 and L.soccdpt_vis_minmax_scratch_bytes(1, 5) == 8
    assert L.soccdpt_vis_minmax_scratch_bytes(0, 5) == 0 and L.soccdpt_vis_minmax_scratch_bytes(1, 0) == 0
    assert L.soccdpt_vis_resize_taps(0, 4, None) != 0 and b"soccdpt_vis_resize_taps" in L.soccdpt_last_error(None)
    with pytest.raises(RuntimeError, match="soccdpt_vis_resize_taps"):
        resize_taps(0, 3)


def test_cpu_tensors_raise():
    from soccdpt_amd.utils import visualise as V
    img = torch.zeros((4, 6, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        V.colorize_disparity(torch.zeros((4, 6)))
    with pytest.raises(RuntimeError):
        V.color_masks(torch.zeros((1, 3, 4, 6)), {0: (1, 2, 3), 1: (4, 5, 6), 2: (7, 8, 9)})
    with pytest.raises(RuntimeError):
        V.color_segmentation(torch.zeros((4, 6, 3)), img, {0: (1, 2, 3), 1: (4, 5, 6), 2: (7, 8, 9)})
    with pytest.raises(RuntimeError):
        V.resize_bgr(img, (3, 2))
    with pytest.raises(RuntimeError):
        V.shrink_half(img)
    with pytest.raises(RuntimeError):
        V.evaluation_panel(img, torch.zeros((4, 6)), torch.zeros((3, 4, 6)), [(1, 2, 3)] * 3)
    with pytest.raises(RuntimeError):
        V.disparity_minmax(torch.zeros((1, 4, 6)))


def test_forward_source_hash_did_not_move():
    """visualise.hip is picked up by the Makefile's wildcard; the Makefile and every other source the forward path is built from are as the newest
    committed counter profile saw them."""
    from soccdpt_amd.lib import FORWARD_SOURCES, csrc_sha
    assert "visualise.hip" not in FORWARD_SOURCES and "capi.cpp" not in FORWARD_SOURCES
    newest = sorted(glob.glob(os.path.join(REPO, "profiles", "r*_pmc_traffic.json")))[-1]
    assert json.load(open(newest))["csrc_sha"] == csrc_sha()
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "visualise.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0]
