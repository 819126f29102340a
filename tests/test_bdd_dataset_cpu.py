"""CPU: the Bengaluru dataset reader (soccdpt_amd/datasets/) and the batch-target entry points (include/soccdpt_data.h) as far as they go without a
GPU: the numpy specification against the reference's recorded outputs, the recording reader on a PIL-written recording, the third header against its
ctypes table, the batch index arithmetic through Subset / ConcatDataset, the messages."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import bdd_targets_refs as R
# tests/test_capi_symbols.py owns the rules by which a C declaration and a ctypes type are held to be of the same class; existing test files are left
# as they are, hence the import of its helpers
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the specification against the reference's own functions (tests/golden/bdd_targets.npz, tests/tools/make_golden_bdd_targets.py) ----
@pytest.mark.parametrize("name,shape", [("small", (5, 7)), ("odd", (37, 53))])
def test_specification_equals_the_reference(golden_dir, name, shape):
    g = np.load(os.path.join(golden_dir, "bdd_targets.npz"))
    seg = g[f"{name}_seg"]
    assert seg.shape == shape + (3,) and seg.dtype == np.uint8
    assert np.array_equal(seg, R.label_frames(1, shape[0], shape[1], {"small": 57, "odd": 3753}[name])[0])     # the inputs are reproducible
    want_bool, want_class = g[f"{name}_bool"], g[f"{name}_class"]
    got = R.onehot(seg[None], R.BDD_COLORS)[0]
    assert got.dtype == np.float32 and np.array_equal(got, np.moveaxis(want_bool, 2, 0).astype(np.float32))
    # rgb_seg_to_class flips before it compares
    assert np.array_equal(R.class_map(seg[None], R.BDD_COLORS, flip=True)[0], want_class.astype(np.int32))
    assert not np.array_equal(R.class_map(seg[None], R.BDD_COLORS, flip=False)[0], want_class)
    assert int(R.unmatched(seg[None], R.BDD_COLORS)[0]) == int((~want_bool.any(axis=2)).sum()) > 0
    # the reversed colours: no plane, but a class
    rev = np.all(seg == (142, 0, 0), axis=-1)
    assert rev.any() and not want_bool[rev].any() and (want_class[rev] == 1).all()
    # the package's own host forms say the same
    from soccdpt_amd.datasets.bdd_helper import rgb_seg_to_class
    from soccdpt_amd.datasets.bengaluru_driving_dataset import color_2_class, color_table, rgb_seg_to_bool
    assert np.array_equal(rgb_seg_to_bool(seg), want_bool) and np.array_equal(rgb_seg_to_class(seg, color_2_class), want_class)
    assert np.array_equal(color_table(), R.BDD_COLORS)


def test_specification_order_and_duplicates():
    seg = R.label_frames(2, 6, 9, 5)
    colors = np.array([(0, 0, 142), (0, 0, 0), (0, 0, 142), (220, 20, 60)], dtype=np.uint8)      # class 0 and class 2 share a colour
    one = R.onehot(seg, colors)
    assert np.array_equal(one[:, 0], one[:, 2]) and one[:, 0].any()
    cm = R.class_map(seg, colors)
    assert (cm[one[:, 0] == 1] == 2).all()                     # the last match wins
    assert (cm[one.sum(axis=1) == 0] == 0).all()
    d16 = np.array([[[0, 1, 255, 256, 65535]]], dtype=np.uint16)
    assert R.y_disp(d16).tolist() == [[[0.0, 1.0, 255.0, 256.0, 65535.0]]]
    nan = np.array([[[0x7fc01234, 0xff800000, 0x7f800001]]], dtype=np.uint32).view(np.float32)
    assert np.array_equal(R.y_disp(nan).view(np.uint32), nan.view(np.uint32))
    img = np.arange(35, dtype=np.uint8).reshape(5, 7) * 7
    from tests.visualise_refs import resize
    assert np.array_equal(R.resize_u8c1(img, (4, 9)), resize(np.repeat(img[:, :, None], 3, axis=2), (4, 9))[:, :, 0])
    assert np.array_equal(R.resize_u8c1(img, (7, 5)), img)


# ---- the recording reader ----
def _calib(tmp_path, **over):
    from soccdpt_amd.utils.synth import write_synth_calib
    return write_synth_calib(str(tmp_path / "calib.yaml"), **over)


@pytest.mark.parametrize("mode,dtype", [("L", np.uint8), ("I;16", np.uint16)])
def test_recording_reader(tmp_path, mode, dtype):
    from soccdpt_amd.datasets.bdd_helper import DATASET_BASE, DEFAULT_CALIB, DEFAULT_DATASET, BengaluruDepthDatasetIterator
    assert DEFAULT_CALIB.startswith(DATASET_BASE) and DEFAULT_DATASET.startswith(DATASET_BASE)
    rec = R.write_recording(tmp_path, "1650000000001", n=12, size=(10, 14), disp_mode=mode, seed=3)
    it = BengaluruDepthDatasetIterator(dataset_path=str(tmp_path / "1650000000001"), settings_doc=_calib(tmp_path))
    assert len(it) == 12 and it.dataset_id == "1650000000001" and (it.width, it.height) == (1920, 1080)
    assert it.intrinsic_matrix.shape == (3, 3) and it.intrinsic_matrix[0, 2] == 978.4
    for i in (0, 5, 11):
        f = it[i]
        assert set(f) >= {"rgb_frame", "disparity_frame", "seg_frame", "csv_frame", "Index", "Timestamp", "speed"}
        assert np.array_equal(f["rgb_frame"], rec["rgb"][i][:, :, ::-1]) and np.array_equal(f["seg_frame"], rec["seg"][i][:, :, ::-1])
        assert f["disparity_frame"].dtype == dtype and np.array_equal(f["disparity_frame"], rec["disp"][i])
        assert f["Timestamp"] == rec["timestamps"][i] and f["Index"] == i and f["speed"] == 0.5 * i and f["csv_frame"]["Timestamp"] == f["Timestamp"]
    assert sum(1 for _ in it) == 12
    # the reference's bounds: beyond len raises IndexError, len itself is not in the index
    with pytest.raises(IndexError, match="Out of bounds"):
        it[13]
    with pytest.raises(KeyError):
        it[12]
    os.remove(tmp_path / "1650000000001" / "seg_img" / f"{rec['timestamps'][4]}.png")
    with pytest.raises(AssertionError, match=re.escape("File missing " + str(tmp_path / "1650000000001" / "seg_img" / f"{rec['timestamps'][4]}.png"))):
        it[4]
    assert it[3]["Index"] == 3


def test_rgb_disparity_png_raises(tmp_path):
    from PIL import Image
    from soccdpt_amd.datasets.bdd_helper import BengaluruDepthDatasetIterator
    rec = R.write_recording(tmp_path, "7", n=2, size=(6, 8))
    bad = tmp_path / "7" / "depth_img" / f"{rec['timestamps'][1]}.png"
    Image.fromarray(rec["rgb"][1]).save(bad)
    it = BengaluruDepthDatasetIterator(dataset_path=str(tmp_path / "7"), settings_doc=_calib(tmp_path))
    assert it[0]["disparity_frame"].shape == (6, 8)
    with pytest.raises(ValueError, match="mode RGB") as e:
        it[1]
    assert str(bad) in str(e.value)


def test_sixteen_bit_disparity_at_another_size_is_refused_with_both_sizes(tmp_path):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BDD_Depth_Segmentation
    R.write_recording(tmp_path, "9", n=1, size=(6, 8), disp_mode="I;16")
    ds = BDD_Depth_Segmentation(dataset_path=str(tmp_path / "9"), settings_doc=_calib(tmp_path, **{"Camera.width": 16, "Camera.height": 12}), device="cuda:0")
    with pytest.raises(NotImplementedError, match=r"uint16.*8 x 6.*16 x 12"):
        ds.read_frame(0)
    R.write_recording(tmp_path, "10", n=1, size=(12, 16), disp_mode="I;16")
    same = BDD_Depth_Segmentation(dataset_path=str(tmp_path / "10"), settings_doc=ds.settings_doc, device="cuda:0")
    assert same.read_frame(0)["disparity_frame"].dtype == np.uint16


# ---- the third header and its table ----
def _data_header():
    text = open(os.path.join(REPO, "include", "soccdpt_data.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out, code


def test_data_prototype_table_matches_the_header():
    from soccdpt_amd import lib
    header, code = _data_header()
    assert list(header) == ["soccdpt_data_targets", "soccdpt_data_resize_u8c1"]
    assert list(lib.DATA_PROTOTYPES) == list(header), "the table follows the header's order"
    assert not set(lib.DATA_PROTOTYPES) & (set(lib.PROTOTYPES) | set(lib.VIS_PROTOTYPES))
    for name, (restype, argtypes) in lib.DATA_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"
        assert argtypes[-1] is ctypes.c_void_p, "the stream goes last"
    defines = dict(re.findall(r"#define\s+(SOCCDPT_DATA_\w+)\s+(\d+)", code))
    assert (int(defines["SOCCDPT_DATA_U8"]), int(defines["SOCCDPT_DATA_U16"]), int(defines["SOCCDPT_DATA_F32"])) == (lib.DATA_U8, lib.DATA_U16, lib.DATA_F32)
    assert int(defines["SOCCDPT_DATA_MAX_CLASSES"]) == lib.DATA_MAX_CLASSES == 8


def test_data_symbols_exported_and_typed():
    from soccdpt_amd.lib import ABI_VERSION, DATA_PROTOTYPES, LIB_PATH, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _data_header()[0]:
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_data.h but not exported"
    L = load_library()
    for name, (restype, argtypes) in DATA_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert ABI_VERSION == 13 and L.soccdpt_abi_version() == 13      # a third header, not a new version of the first


def test_argument_errors_need_no_gpu():
    """The checks run before anything is launched, so they can be seen without a device: each returns non-zero and names itself in soccdpt_last_error."""
    from soccdpt_amd.lib import load_library
    L = load_library()
    p = 4096      # never dereferenced: every call below fails its argument check
    for args in ((p, p, 0, None, 0, 1, 2, 2, 0, p, None, None, None, None),       # C = 0
                 (p, p, 9, None, 0, 1, 2, 2, 0, p, None, None, None, None),       # C = 9
                 (None, p, 3, None, 0, 1, 2, 2, 0, p, None, None, None, None),    # NULL seg
                 (p, p, 3, None, 0, 1, 2, 2, 0, None, None, p, None, None),       # y_disp without disp
                 (p, p, 3, p, 7, 1, 2, 2, 0, None, None, p, None, None),          # unknown dtype
                 (p, p, 3, None, 0, 0, 2, 2, 0, p, None, None, None, None),       # B = 0
                 (p, p, 3, None, 0, 1, 2, 2, 0, p + 2, None, None, None, None)):  # misaligned f32 output
        assert L.soccdpt_data_targets(*args) != 0
        assert b"soccdpt_data_targets" in L.soccdpt_last_error(None)
    assert L.soccdpt_data_resize_u8c1(None, 1, 2, 2, None, None, 2, 2, p, None) != 0 and b"soccdpt_data_resize_u8c1" in L.soccdpt_last_error(None)
    assert L.soccdpt_data_resize_u8c1(p, 1, 2, 2, None, None, 3, 3, p, None) != 0 and b"tap tables" in L.soccdpt_last_error(None)


def test_batch_targets_source_conventions():
    from soccdpt_amd.lib import FORWARD_SOURCES
    assert "batch_targets.hip" not in FORWARD_SOURCES and "capi.cpp" not in FORWARD_SOURCES
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "batch_targets.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0]


# ---- batch index arithmetic through Subset / ConcatDataset ----
class _Leaf(torch.utils.data.Dataset):
    def __init__(self, name, n):
        self.name, self.n = name, n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return (self.name, i)


def test_batch_indices_follow_the_reference_through_index_maps():
    from soccdpt_amd.datasets.bengaluru_driving_dataset import batch_indices, resolve_index
    from soccdpt_amd.scripts.train_SOccDPT import get_batch
    full = torch.utils.data.ConcatDataset([_Leaf("a", 5), _Leaf("b", 7), _Leaf("c", 3)])
    used, _ = torch.utils.data.random_split(full, [12, 3], generator=torch.Generator().manual_seed(0))
    train, val = torch.utils.data.random_split(used, [10, 2], generator=torch.Generator().manual_seed(0))
    for ds in (full, used, train, val):
        for i in range(len(ds)):
            leaf, k = resolve_index(ds, i)
            assert (leaf.name, k) == ds[i]                                  # what the index maps themselves hand out
    assert resolve_index(full, -1)[1] == 2 and resolve_index(full, 5) == (full.datasets[1], 0)
    with pytest.raises(IndexError):
        resolve_index(full, 15)
    # the reference's loop: range(batch_size, len, batch_size), the batch that ends at `index` holds [index - batch_size, index)
    batch_size = 3
    ends = list(range(batch_size, len(train), batch_size))
    assert ends == [3, 6, 9]                                                # the trailing items 9 are never run, as in the reference
    for index in ends:
        assert list(batch_indices(index, batch_size)) == [index - 3, index - 2, index - 1]
        assert [resolve_index(train, i)[0].name for i in batch_indices(index, batch_size)] == [train[i][0] for i in range(index - batch_size, index)]
    # get_batch of the training script takes the same items
    class _T(torch.utils.data.Dataset):
        def __len__(self):
            return 10

        def __getitem__(self, i):
            return [torch.full((1, 1), float(i))] * 6
    assert get_batch(_T(), 6, 3)[0].reshape(-1).tolist() == [float(i) for i in batch_indices(6, 3)]


def test_decode_pool_is_fixed_and_capped():
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    assert D.DEFAULT_WORKERS == 8 and D.MAX_WORKERS == 16
    assert D.decode_pool()._max_workers == 8 and D.decode_pool(16)._max_workers == 16 and D.decode_pool(8) is D.decode_pool()
    for bad in (0, 17, 64):
        with pytest.raises(ValueError):
            D.decode_pool(bad)
    src = open(D.__file__).read()
    assert "cpu_count" not in src


def test_default_recordings_and_names():
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    assert D.DEFAULT_RECORDINGS == ("1653972957447", "1652937970859", "1654493684259", "1654507149598", "1658384707877", "1658384924059")
    assert D.class_2_color == {0: (0, 0, 0), 1: (0, 0, 142), 2: (220, 20, 60)}
    for name in ("BDD_Depth", "BDD_Segmentation", "BDD_Depth_Segmentation", "get_bdd_dataset", "color_2_class"):
        assert hasattr(D, name)
    assert D.BDD_Depth_Segmentation.fields == ("x", "x_raw", "mask_disp", "y_disp", "mask_seg", "y_seg")


# ---- messages ----
def test_idd_is_refused_for_the_true_reason(tmp_path):
    from soccdpt_amd.scripts import eval_SOccDPT, train_SOccDPT
    with pytest.raises(NotImplementedError, match="three") as e:
        eval_SOccDPT.main(eval_SOccDPT.build_parser().parse_args(["-v", "3", "-dt", "idd", "-t", "dpt_swin2_tiny_256", "-b", str(tmp_path)]))
    assert "model/SOccDPT.py:343-349" in str(e.value) and "label tables" not in str(e.value)
    for dt in ("idd", "idd+bdd"):
        with pytest.raises(RuntimeError, match="three classes|exactly three"):
            train_SOccDPT.train_net(dataset=dt, base_path=str(tmp_path))
