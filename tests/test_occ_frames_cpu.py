"""CPU: the per-frame occupancy mode's surface -- C symbols, ABI version, constructor contract, argument parsing (no GPU work)."""
import ctypes
import os
import re
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("soccdpt_voxelise_frames", "soccdpt_occ_expand_frames", "soccdpt_forward_frames")


def _calib():
    from soccdpt_amd.utils.synth import write_synth_calib
    return write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))


def test_symbols_declared_exported_and_bound():
    so = os.path.join(REPO, "soccdpt_amd", "libsoccdpt_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    raw = ctypes.CDLL(so)
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    from soccdpt_amd.lib import Engine, load_library
    L = load_library()
    for n in SYMBOLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", code), f"{n} is not declared in include/soccdpt_hip.h"
        assert hasattr(raw, n), f"{n} is not exported"
        f = getattr(L, n)
        assert f.argtypes is not None and f.restype is ctypes.c_int, f"{n} is not bound in soccdpt_amd/lib.py"
    assert len(L.soccdpt_voxelise_frames.argtypes) == 9
    assert len(L.soccdpt_occ_expand_frames.argtypes) == 5
    assert len(L.soccdpt_forward_frames.argtypes) == len(L.soccdpt_forward.argtypes) + 1       # soccdpt_forward's arguments + dev_frame_bits
    for m in ("voxelise_frames", "occ_expand_frames", "forward_frames"):
        assert callable(getattr(Engine, m))
    assert "eager" in header[header.index("soccdpt_forward_frames:"):].split("*/")[0].lower()    # the header says the call is never graph-replayed


def test_abi_version_is_13_in_all_three_places():
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    assert int(re.search(r"#define\s+SOCCDPT_ABI_VERSION\s+(\d+)", header).group(1)) == 13
    assert re.search(r"^\s*\*\s+8 \(per-frame occupancy", header, flags=re.M), "the header's version history has no line for 8"
    assert re.search(r"^\s*\*\s+9 \(soccdpt_train_layer_bwd_args", header, flags=re.M), "the header's version history has no line for 9"
    assert re.search(r"^\s*\*\s+10 \(soccdpt_train_aux_args", header, flags=re.M), "the header's version history has no line for 10"
    assert re.search(r"^\s*\*\s+11 \(soccdpt_fwd_aux_args", header, flags=re.M), "the header's version history has no line for 11"
    assert re.search(r"^\s*\*\s+12 \(soccdpt_op_attention_bwd", header, flags=re.M), "the header's version history has no line for 12"
    assert re.search(r"^\s*\*\s+13 \(soccdpt_op_gn_apply_halo", header, flags=re.M), "the header's version history has no line for 13"
    from soccdpt_amd import lib as binding
    assert binding.ABI_VERSION == 13
    assert binding.load_library().soccdpt_abi_version() == 13
    # soccdpt_config did not grow
    assert binding.load_library().soccdpt_sizeof(0) == ctypes.sizeof(binding.SoccdptConfig) == 4 * (9 + 4 + 3 + 9 + 27)


def test_new_source_is_not_a_forward_source():
    from soccdpt_amd.lib import FORWARD_SOURCES
    assert "occ_frames.hip" not in FORWARD_SOURCES and "capi.cpp" not in FORWARD_SOURCES and "internal.h" not in FORWARD_SOURCES
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "occ_frames.hip")).read()
    assert src.startswith("#pragma clang fp contract(off)\n")       # before any include: the file is not compiled with -ffp-contract=off
    assert src.index("#pragma clang fp contract(off)") < src.index("#include")


def test_constructor_contract():
    import inspect
    from soccdpt_amd.model.SOccDPT import SOccDPT, SOccDPT_V3
    assert inspect.signature(SOccDPT.__init__).parameters["occupancy_per_frame"].default is False
    assert issubclass(SOccDPT_V3, SOccDPT)
    calib = _calib()
    assert SOccDPT(camera_intrinsics_yaml=calib).occupancy_per_frame is False
    assert SOccDPT(camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True).occupancy_per_frame is True
    with pytest.raises(AssertionError):
        SOccDPT(camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True, share_occupancy_rows=True)
    assert SOccDPT(camera_intrinsics_yaml=calib, compute_occ=True, share_occupancy_rows=True).share_occupancy_rows is True


def test_v3_inherits_the_flag_and_union_mode_refuses_a_frame():
    import contextlib
    import io
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    calib = _calib()
    with contextlib.redirect_stdout(io.StringIO()):
        per = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True)
        uni = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True)
        with pytest.raises(AssertionError):
            SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True, share_occupancy_rows=True)
    assert per.occupancy_per_frame is True and uni.occupancy_per_frame is False
    with pytest.raises(RuntimeError):
        uni.occupancy_points(frame=0)
    with pytest.raises(RuntimeError):
        per.occupancy_points(frame=0)      # no forward yet
    with pytest.raises(RuntimeError):
        uni.occupancy_points()             # unchanged: needs a forward first


def test_eval_parser_accepts_the_flag():
    from soccdpt_amd.scripts.eval_SOccDPT import build_parser
    base = ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256"]
    a = build_parser().parse_args(base)
    assert a.occupancy_per_frame is False and a.occupancy is False
    a = build_parser().parse_args(base + ["--occupancy-per-frame"])
    assert a.occupancy_per_frame is True


def test_dist_docstring_says_the_rows_stay_local():
    import soccdpt_amd.dist as D
    assert "occupancy_per_frame" in D.__doc__ and "RANK-LOCAL" in D.__doc__
