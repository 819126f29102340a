"""CPU: frame packs (soccdpt_amd/datasets/frame_pack.py) as far as they go without a GPU: the index packing against its numpy
specification, the format's round trip, equality with the PNG decode, staleness, the dataset's read_frame, the packing script, and the fourth header
(include/soccdpt_pack.h) against its ctypes table.  Every comparison is exact."""
import ctypes
import math
import os
import re
import struct
import warnings

import numpy as np
import pytest

from tests import bdd_targets_refs as R
from tests import frame_pack_refs as F
# tests/test_capi_symbols.py owns the rules by which a C declaration and a ctypes type are held to be of the same class
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _calib(tmp_path, **over):
    from soccdpt_amd.utils.synth import write_synth_calib
    return write_synth_calib(str(tmp_path / "calib.yaml"), **over)


def make_recording(base, rec_id, palette, size, n=2, disp_mode="L", seed=0):
    """bdd_targets_refs.write_recording, then the label PNGs written again so that every colour of `palette` occurs in the DECODED frames (when the
    recording has that many pixels), and for disp_mode 'F' the disparity files written again as float images.  -> the frames as the files hold them."""
    from PIL import Image
    H, W = size
    rec = R.write_recording(base, rec_id, n=n, size=size, disp_mode="L" if disp_mode == "F" else disp_mode, seed=seed, palette=palette, blocky=False)
    rng = np.random.default_rng(seed + 1)
    idx = rng.permutation(n * H * W) % len(palette)
    assert n * H * W < len(palette) or len(set(idx.tolist())) == len(palette)
    # the reader flips the channel axis: the files hold the reversed colours, so that a decoded label frame is palette[idx]
    rec["seg"] = np.ascontiguousarray(np.asarray(palette, dtype=np.uint8)[idx].reshape(n, H, W, 3)[..., ::-1])
    root = os.path.join(str(base), str(rec_id))
    for i, t in enumerate(rec["timestamps"]):
        Image.fromarray(rec["seg"][i]).save(os.path.join(root, "seg_img", f"{t}.png"))
    if disp_mode == "F":
        d = rng.standard_normal((n, H, W)).astype(np.float32)
        d.reshape(-1)[0] = np.array([0x7fc01234], dtype=np.uint32).view(np.float32)[0]      # a NaN with a payload
        rec["disp"] = d
        for i, t in enumerate(rec["timestamps"]):      # PIL finds the format in the file, not in its name
            Image.fromarray(d[i], mode="F").save(os.path.join(root, "depth_img", f"{t}.png"), format="TIFF")
    return rec


# ---- the index packing ----
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_index_packing_equals_the_specification(k):
    from soccdpt_amd.datasets import frame_pack as P
    for n in (1, 3, 31, 32, 33, 35, 1961):
        idx = np.random.default_rng(n + k).integers(0, 1 << k, size=n)
        words = P.pack_indices(idx, k)
        assert words.dtype == np.dtype("<u4") and words.size == F.record_words(n, k) == P.record_words(n, k) == math.ceil(n * k / 32)
        assert np.array_equal(words, F.pack(idx, k))
        assert np.array_equal(P.unpack_indices(words, k, n), idx) and np.array_equal(F.unpack(words, k, n), idx)
        if (n * k) % 32:      # unused high bits are zero
            assert int(words[-1]) >> ((n * k) % 32) == 0
    # the sentence of the format, by hand: k = 2, pixels 0 .. 16 -> pixel 16 opens the second word
    assert F.pack([3, 0, 1] + [0] * 13 + [2], 2).tolist() == [0b010011, 2]
    assert [P.index_bits(p) for p in (1, 2, 3, 4, 5, 16, 17, 256)] == [F.index_bits(p) for p in (1, 2, 3, 4, 5, 16, 17, 256)] == [1, 1, 2, 2, 4, 4, 8, 8]


# ---- the format ----
@pytest.mark.parametrize("size", [(1, 1), (5, 7), (37, 53)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("P", [1, 2, 3, 4, 5, 16, 17, 256])
def test_format_round_trip(tmp_path, P, size):
    from soccdpt_amd.datasets import frame_pack as FP
    from soccdpt_amd.datasets.bdd_helper import decode_color, decode_disparity
    H, W = size
    n = max(2, math.ceil(P / (H * W)))
    palette = F.random_palette(P, seed=P, include=R.BDD_COLORS)
    rec = make_recording(tmp_path, "77", palette, size, n=n, seed=P + H)
    out = FP.write_pack(str(tmp_path / "77"))
    assert out == FP.pack_path(str(tmp_path / "77"), True) == str(tmp_path / "77" / "77.sfp")
    assert not [f for f in os.listdir(tmp_path / "77") if ".tmp" in f]
    pack = FP.FramePack(out)
    pack.check_current(str(tmp_path / "77"))
    assert len(pack) == n and pack.P == P and pack.k == F.index_bits(P) and not pack.raw_labels
    assert np.array_equal(pack.palette, F.palette_of(rec["seg"][..., ::-1])) and np.array_equal(pack.palette, palette)
    assert pack.shapes == {"rgb": size, "disparity": size, "labels": size} and pack.disp_dtype == np.uint8
    assert pack.words_per_frame == F.record_words(H * W, pack.k)
    assert os.path.getsize(out) % FP.ALIGN == 0 and not (pack.offsets % FP.ALIGN).any()
    # the header as DESIGN.md 12.4 states it, read with nothing but struct
    raw = open(out, "rb").read()
    assert raw[:8] == b"SOCCFPK\0" and struct.unpack_from("<II", raw, 8) == (1, n)
    assert struct.unpack_from("<12I", raw, 16) == (H, W, 0, 0, H, W, 0, 0, H, W, 0, pack.k) and struct.unpack_from("<I", raw, 64) == (P,)
    assert struct.unpack_from("<Q", raw, 128) == (len(raw),)
    assert raw[144: 144 + 3 * P] == palette.tobytes() and not any(raw[144 + 3 * P: 912])
    root = str(tmp_path / "77")
    for i, t in enumerate(rec["timestamps"]):
        f = pack.frame(i)
        rgb, disp, seg = (decode_color(f"{root}/rgb_img/{t}.png"), decode_disparity(f"{root}/depth_img/{t}.png"), decode_color(f"{root}/seg_img/{t}.png"))
        assert f["rgb"].dtype == np.uint8 and f["rgb"].tobytes() == rgb.tobytes() and f["rgb"].shape == rgb.shape
        assert f["disparity"].dtype == disp.dtype and f["disparity"].tobytes() == disp.tobytes() and f["disparity"].shape == disp.shape
        assert np.array_equal(f["labels"], F.pack(F.indices_of(seg, palette), pack.k))
        got = pack.labels_rgb(i)
        assert got.dtype == np.uint8 and got.shape == seg.shape and got.tobytes() == seg.tobytes()
        assert np.array_equal(F.expand(f["labels"], pack.k, palette, 1, H, W)[0], seg)
        off = int(pack.offsets[i, 2])
        assert raw[off: off + 4 * pack.words_per_frame] == f["labels"].tobytes()
    with pytest.raises(IndexError):
        pack.frame(n)


@pytest.mark.parametrize("mode,dtype", [("L", np.uint8), ("I;16", np.uint16), ("F", np.float32)])
def test_frames_equal_the_png_decode_for_every_disparity_mode(tmp_path, mode, dtype):
    from soccdpt_amd.datasets import frame_pack as FP
    from soccdpt_amd.datasets.bdd_helper import decode_color, decode_disparity
    rec = make_recording(tmp_path, "5", R.PALETTE, (10, 14), n=3, disp_mode=mode, seed=2)
    out = FP.write_pack(str(tmp_path / "5"), out_dir=str(tmp_path / "packs"))
    assert out == str(tmp_path / "packs" / "5.sfp") == FP.pack_path(str(tmp_path / "5"), str(tmp_path / "packs"))
    pack = FP.open_current(str(tmp_path / "5"), str(tmp_path / "packs"))
    assert pack.disp_dtype == dtype and pack.P == len(R.PALETTE) == 7 and pack.k == 4
    for i, t in enumerate(rec["timestamps"]):
        f = pack.frame(i)
        want = decode_disparity(str(tmp_path / "5" / "depth_img" / f"{t}.png"))
        assert want.dtype == dtype and f["disparity"].dtype == dtype and f["disparity"].tobytes() == want.tobytes() == rec["disp"][i].tobytes()
        assert f["rgb"].tobytes() == decode_color(str(tmp_path / "5" / "rgb_img" / f"{t}.png")).tobytes()
        assert pack.labels_rgb(i).tobytes() == decode_color(str(tmp_path / "5" / "seg_img" / f"{t}.png")).tobytes()
    assert FP.verify_pack(str(tmp_path / "5"), str(tmp_path / "packs")) == 3


def test_more_than_256_colours_are_stored_raw(tmp_path):
    from soccdpt_amd.datasets import frame_pack as FP
    from soccdpt_amd.datasets.bdd_helper import decode_color
    rec = make_recording(tmp_path, "8", F.random_palette(257, seed=1), (37, 53), n=2)
    pack = FP.FramePack(FP.write_pack(str(tmp_path / "8")))
    assert pack.raw_labels and pack.k == 0 and pack.P == 0 and pack.rec_bytes[2] == 37 * 53 * 3
    for i, t in enumerate(rec["timestamps"]):
        want = decode_color(str(tmp_path / "8" / "seg_img" / f"{t}.png"))
        assert pack.frame(i)["labels"].shape == (37, 53, 3) and pack.frame(i)["labels"].tobytes() == want.tobytes() == pack.labels_rgb(i).tobytes()


# ---- staleness ----
def _dataset(tmp_path, rec_id, **kw):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BDD_Segmentation
    return BDD_Segmentation(dataset_path=str(tmp_path / rec_id), settings_doc=_calib(tmp_path), device="cuda:0", **kw)


def test_a_rewritten_png_is_detected_and_named(tmp_path):
    from PIL import Image
    from soccdpt_amd.datasets import frame_pack as FP
    rec = make_recording(tmp_path, "3", R.PALETTE, (6, 8), n=3)
    root = str(tmp_path / "3")
    FP.write_pack(root)
    FP.open_current(root)
    # the same bytes, another mtime_ns
    touched = os.path.join(root, "depth_img", f"{rec['timestamps'][1]}.png")
    st = os.stat(touched)
    os.utime(touched, ns=(st.st_atime_ns, st.st_mtime_ns + 1))
    with pytest.raises(FP.FramePackError, match="stale") as e:
        FP.open_current(root)
    assert e.value.path == touched and touched in str(e.value)
    os.utime(touched, ns=(st.st_atime_ns, st.st_mtime_ns))
    FP.open_current(root)
    # another size; an earlier file in the table's order is the one named
    grown = os.path.join(root, "rgb_img", f"{rec['timestamps'][0]}.png")
    Image.fromarray(np.zeros((6, 8, 3), dtype=np.uint8)).save(grown)
    os.utime(touched, ns=(st.st_atime_ns, st.st_mtime_ns + 1))
    with pytest.raises(FP.FramePackError) as e:
        FP.open_current(root)
    assert e.value.path == grown and grown in str(e.value)
    # a PNG that is gone
    os.remove(grown)
    with pytest.raises(FP.FramePackError, match="gone") as e:
        FP.open_current(root)
    assert e.value.path == grown


def test_truncated_and_foreign_packs_are_detected_and_named(tmp_path):
    from soccdpt_amd.datasets import frame_pack as FP
    make_recording(tmp_path, "4", R.PALETTE, (6, 8), n=3)
    root = str(tmp_path / "4")
    out = FP.write_pack(root)
    good = open(out, "rb").read()
    for keep in (len(good) - 1, len(good) - FP.ALIGN, 1000, 100):      # inside the last record, a record short, inside the tables, inside the header
        open(out, "wb").write(good[:keep])
        with pytest.raises(FP.FramePackError, match="truncated") as e:
            FP.open_current(root)
        assert e.value.path == out and out in str(e.value)
    # the header's size agrees with the file but a record of the offset table does not fit
    bad = bytearray(good[: len(good) - FP.ALIGN])
    struct.pack_into("<Q", bad, 128, len(bad))
    open(out, "wb").write(bytes(bad))
    with pytest.raises(FP.FramePackError, match="truncated.*offset table") as e:
        FP.open_current(root)
    assert e.value.path == out
    # another version
    bad = bytearray(good)
    struct.pack_into("<I", bad, 8, FP.VERSION + 1)
    open(out, "wb").write(bytes(bad))
    with pytest.raises(FP.FramePackError, match=f"version {FP.VERSION + 1}.*version {FP.VERSION}") as e:
        FP.open_current(root)
    assert e.value.path == out and out in str(e.value)
    open(out, "wb").write(b"not a pack at all" * 20)
    with pytest.raises(FP.FramePackError, match="not a frame pack"):
        FP.open_current(root)
    os.remove(out)
    with pytest.raises(FP.FramePackError, match="no such frame pack") as e:
        FP.open_current(root)
    assert e.value.path == out


def test_required_raises_and_the_default_warns_once_and_reads_the_pngs(tmp_path):
    from soccdpt_amd.datasets import frame_pack as FP
    rec = make_recording(tmp_path, "6", R.PALETTE, (6, 8), n=3)
    root = str(tmp_path / "6")
    with pytest.raises(FP.FramePackError, match="no such frame pack"):
        _dataset(tmp_path, "6", frame_pack=True, frame_pack_required=True)
    FP.write_pack(root)
    assert _dataset(tmp_path, "6", frame_pack=True, frame_pack_required=True).pack is not None
    touched = os.path.join(root, "seg_img", f"{rec['timestamps'][2]}.png")
    st = os.stat(touched)
    os.utime(touched, ns=(st.st_atime_ns, st.st_mtime_ns + 5))
    with pytest.raises(FP.FramePackError, match="stale"):
        _dataset(tmp_path, "6", frame_pack=True, frame_pack_required=True)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ds = _dataset(tmp_path, "6", frame_pack=True)
        png = _dataset(tmp_path, "6")
        for i in range(3):
            a, b = ds.read_frame(i), png.read_frame(i)
            assert set(a) == set(b) and all(np.array_equal(a[key], b[key]) for key in ("rgb_frame", "disparity_frame", "seg_frame"))
            assert "_pooled" not in ds.batch_frame(i) and "seg_index" not in ds.batch_frame(i)
    mine = [w for w in seen if issubclass(w.category, RuntimeWarning) and "stale" in str(w.message)]
    assert len(mine) == 1 and touched in str(mine[0].message) and "reading the PNGs" in str(mine[0].message)
    assert ds.pack is None and png.pack is None


@pytest.mark.parametrize("colours", [7, 257], ids=["indexed", "raw"])
def test_read_frame_from_a_pack_equals_read_frame_from_pngs(tmp_path, colours):
    from soccdpt_amd.datasets import frame_pack as FP
    palette = R.PALETTE if colours == 7 else F.random_palette(colours, seed=3)
    make_recording(tmp_path, "9", palette, (12, 20), n=4, disp_mode="I;16")
    FP.write_pack(str(tmp_path / "9"), out_dir=str(tmp_path / "elsewhere"))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        packed, png = _dataset(tmp_path, "9", frame_pack=str(tmp_path / "elsewhere"), frame_pack_required=True), _dataset(tmp_path, "9")
    assert packed.pack is not None and packed.pack.raw_labels == (colours == 257) and len(packed) == len(png) == 4
    for i in range(4):
        a, b = packed.read_frame(i), png.read_frame(i)
        assert list(a) == list(b)
        for key in b:
            if isinstance(b[key], np.ndarray):
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
            else:
                assert a[key] == b[key] and type(a[key]) is type(b[key]), key
        fast = packed.batch_frame(i)
        assert fast["_pooled"] and fast["rgb_frame"].tobytes() == b["rgb_frame"].tobytes()
        if colours == 7:
            assert "seg_frame" not in fast and np.array_equal(fast["seg_index"].view(np.uint32), F.pack(F.indices_of(b["seg_frame"], packed.pack.palette), 4))
        else:
            assert fast["seg_frame"].tobytes() == b["seg_frame"].tobytes()
    with pytest.raises(IndexError, match="Out of bounds"):
        packed.read_frame(5)
    with pytest.raises(KeyError):
        packed.read_frame(4)


# ---- the packing script ----
def test_pack_recordings_verify_passes_on_a_good_pack_and_fails_on_a_corrupted_record(tmp_path, capsys):
    from soccdpt_amd.datasets import frame_pack as FP
    from soccdpt_amd.scripts import pack_recordings
    rec = make_recording(tmp_path, "11", R.PALETTE, (9, 13), n=3)
    make_recording(tmp_path, "12", R.PALETTE[:2], (9, 13), n=2)
    parse = pack_recordings.build_parser().parse_args
    common = ["-b", str(tmp_path), "--recordings", "11", "12", "--workers", "4"]
    assert pack_recordings.main(parse(common)) == 0
    assert "7 label colours at 4 bits" in capsys.readouterr().out
    assert pack_recordings.main(parse(common + ["--verify"])) == 0
    out = str(tmp_path / "11" / "11.sfp")
    pack = FP.FramePack(out)
    at = int(pack.offsets[1, 1]) + 5      # one byte of frame 1's disparity record
    pack.close()
    raw = bytearray(open(out, "rb").read())
    raw[at] ^= 0x40
    open(out, "wb").write(bytes(raw))
    assert pack_recordings.main(parse(common + ["--verify"])) == 1
    err = capsys.readouterr().err
    assert "FAILED" in err and os.path.join(str(tmp_path), "11", "depth_img", f"{rec['timestamps'][1]}.png") in err
    # --out: packs beside the recordings
    assert pack_recordings.main(parse(common + ["--out", str(tmp_path / "packs")])) == 0
    assert sorted(os.listdir(tmp_path / "packs")) == ["11.sfp", "12.sfp"]
    assert pack_recordings.main(parse(common + ["--out", str(tmp_path / "packs"), "--verify"])) == 0


def test_script_flags_default_to_off():
    from soccdpt_amd.scripts import eval_SOccDPT, train_SOccDPT
    for mod, head in ((eval_SOccDPT, ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256"]),
                      (train_SOccDPT, ["-v", "3", "-dt", "bdd", "-t", "dpt_swin2_tiny_256", "--sweep_json", "x.json"])):
        parse = mod.build_parser().parse_args
        assert parse(head).frame_pack is None and parse(head).frame_pack_required is False
        assert parse(head + ["--frame_pack"]).frame_pack is True and parse(head + ["--frame_pack", "/p", "--frame_pack_required"]).frame_pack == "/p"
        assert parse(head + ["--frame_pack", "/p", "--frame_pack_required"]).frame_pack_required is True


# ---- the fourth header and its table ----
def _pack_header():
    text = open(os.path.join(REPO, "include", "soccdpt_pack.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        plist = [] if params.strip() in ("", "void") else [" ".join(p.split()) for p in params.split(",")]
        out[name] = (_c_class(ret, False), [_c_class(p, True) for p in plist])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out


def test_pack_prototype_table_matches_the_header():
    from soccdpt_amd import lib
    header = _pack_header()
    assert list(header) == ["soccdpt_pack_targets", "soccdpt_pack_expand"]
    assert list(lib.PACK_PROTOTYPES) == list(header), "the table follows the header's order"
    assert not set(lib.PACK_PROTOTYPES) & (set(lib.PROTOTYPES) | set(lib.VIS_PROTOTYPES) | set(lib.DATA_PROTOTYPES))
    for name, (restype, argtypes) in lib.PACK_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, f"{name}: returns {want_ret} in the header, {restype} in the table"
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"
        assert argtypes[-1] is ctypes.c_void_p, "the stream goes last"
    assert lib.PACK_INDEX_BITS == (1, 2, 4, 8)


def test_pack_symbols_exported_and_typed():
    from soccdpt_amd.lib import ABI_VERSION, LIB_PATH, PACK_PROTOTYPES, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _pack_header():
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_pack.h but not exported"
    L = load_library()
    for name, (restype, argtypes) in PACK_PROTOTYPES.items():
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == argtypes, name
    assert ABI_VERSION == 13 and L.soccdpt_abi_version() == 13      # a fourth header, not a new version of the first


def test_argument_errors_need_no_gpu():
    """The checks run before anything is launched, so they can be seen without a device: each returns non-zero and names itself in soccdpt_last_error."""
    from soccdpt_amd.lib import load_library
    L = load_library()
    p = 4096      # never dereferenced: every call below fails its argument check
    # (idx, k, words, palette, P, colors, C, disp, dtype, B, H, W, flip, onehot, class_map, y_disp, unmatched, stream); 2 x 2 pixels at k = 2: one word
    good = [p, 2, 1, p, 3, p, 3, None, 0, 1, 2, 2, 0, p, None, None, None, None]
    def bad(**over):
        names = ("idx", "k", "words", "palette", "P", "colors", "C", "disp", "dtype", "B", "H", "W", "flip", "onehot", "class_map", "y_disp", "unmatched", "stream")
        args = list(good)
        for key, v in over.items():
            args[names.index(key)] = v
        return args
    cases = {"k = 3": (bad(k=3), b"1, 2, 4 or 8"), "k = 0": (bad(k=0), b"1, 2, 4 or 8"), "k = 16": (bad(k=16), b"1, 2, 4 or 8"),
             "P = 0": (bad(P=0), b"2^k"), "P = 5 at k = 2": (bad(P=5), b"2^k"), "P = 257 at k = 8": (bad(k=8, P=257), b"2^k"),
             "words too small": (bad(H=5, W=7), b"words_per_frame"), "words = 0": (bad(words=0), b"words_per_frame"),
             "idx off by 2": (bad(idx=p + 2), b"aligned to 4"), "NULL idx": (bad(idx=None), b"null"), "NULL palette": (bad(palette=None), b"null"),
             "C = 0": (bad(C=0), b"classes"), "C = 9": (bad(C=9), b"classes"), "NULL colors": (bad(colors=None), b"null colors"),
             "y_disp without disp": (bad(y_disp=p), b"without disp"), "unknown dtype": (bad(disp=p, dtype=7, y_disp=p), b"disp_dtype"),
             "B = 0": (bad(B=0), b"B <= 65535"), "H = 0": (bad(H=0), b"B <= 65535"), "misaligned f32 output": (bad(onehot=p + 2), b"not aligned"),
             "misaligned u16 disparity": (bad(disp=p + 1, dtype=1, y_disp=p), b"not aligned"), "misaligned counters": (bad(unmatched=p + 4), b"not aligned")}
    for what, (args, says) in cases.items():
        assert L.soccdpt_pack_targets(*args) != 0, what
        msg = L.soccdpt_last_error(None)
        assert b"soccdpt_pack_targets" in msg and says in msg, (what, msg)
    # (idx, k, words, palette, P, B, H, W, dst, stream)
    for what, args, says in (("k", (p, 5, 1, p, 3, 1, 2, 2, p, None), b"1, 2, 4 or 8"), ("P", (p, 1, 1, p, 3, 1, 2, 2, p, None), b"2^k"),
                             ("words", (p, 8, 0, p, 3, 1, 2, 2, p, None), b"words_per_frame"), ("idx", (p + 1, 8, 1, p, 3, 1, 2, 2, p, None), b"aligned to 4"),
                             ("dst", (p, 8, 1, p, 3, 1, 2, 2, None, None), b"null dst"), ("B", (p, 8, 1, p, 3, 70000, 2, 2, p, None), b"B <= 65535")):
        assert L.soccdpt_pack_expand(*args) != 0, what
        msg = L.soccdpt_last_error(None)
        assert b"soccdpt_pack_expand" in msg and says in msg, (what, msg)


def test_frame_pack_source_conventions():
    from soccdpt_amd.lib import FORWARD_SOURCES
    assert "frame_pack.hip" not in FORWARD_SOURCES
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "frame_pack.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0]
    py = open(os.path.join(REPO, "soccdpt_amd", "datasets", "frame_pack.py")).read()
    assert "cpu_count" not in py
