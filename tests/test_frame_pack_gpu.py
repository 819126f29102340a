"""GPU: soccdpt_pack_targets / soccdpt_pack_expand (include/soccdpt_pack.h) through the C ABI, and the datasets reading frame packs.
soccdpt_pack_expand is held against the numpy specification (tests/frame_pack_refs.py); soccdpt_pack_targets against soccdpt_data_targets on the
expanded frames (itself held against numpy by tests/test_bdd_targets_gpu.py); batches from packs against batches from the PNGs.  All comparisons are
of bits."""
import os

import numpy as np
import pytest
import torch

from tests import bdd_targets_refs as R
from tests import frame_pack_refs as F

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (1, 48, 64), (2, 64, 256)]      # as tests/test_bdd_targets_gpu.py
COLORS8 = np.array([(0, 0, 0), (0, 0, 142), (220, 20, 60), (142, 0, 0), (0, 0, 142), (60, 20, 220), (0, 0, 141), (9, 9, 9)], dtype=np.uint8)   # 1 and 4: listed twice
P_OF_K = {1: (2, 1), 2: (4, 3), 4: (16, 5), 8: (256, 17)}      # P equal to 2^k, and below it (indices >= P occur and are clamped)
OUTPUTS = ("onehot", "class_map", "y_disp", "unmatched")


def _disp(dtype, B, H, W, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)
    if dtype == np.uint16:
        d = rng.integers(0, 65536, size=(B, H, W)).astype(np.uint16)
        d.reshape(-1)[:5] = np.array([0, 1, 255, 256, 65535], dtype=np.uint16)[: d.size]
        return d
    d = rng.standard_normal((B, H, W)).astype(np.float32)
    special = np.array([0x7fc01234, 0xffc00001, 0x7f800000, 0xff800000, 0x80000000, 0x00000001], dtype=np.uint32).view(np.float32)   # NaNs with payloads, +-inf, -0, a denormal
    d.reshape(-1)[: min(6, d.size)] = special[: d.size]
    return d


def _packed(B, H, W, k, P, seed, extra_words=0):
    """Random indices over the whole range of k bits (so values >= P occur when P < 2^k) -> (u32 [B, words] host, palette u8 [P,3] host).  The palette
    holds the class colours and their channel-reversed forms as far as they fit, and random colours that match no class."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 1 << k, size=(B, H * W))
    words = F.record_words(H * W, k) + extra_words
    host = np.stack([F.pack(idx[b], k, words) for b in range(B)])
    if extra_words:
        host[:, -extra_words:] = 0xdeadbeef      # never read as pixels
    return host, F.random_palette(P, seed + 1, include=R.PALETTE)


def _dev(a, device):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(device)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_targets(got, want):
    for key in OUTPUTS:
        assert (got[key] is None) == (want[key] is None), key
        if got[key] is not None:
            assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype and torch.equal(_bits(got[key]), _bits(want[key])), key


@pytest.mark.parametrize("k", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_targets_equal_data_targets_on_the_expanded_frames(gpu_device, shape, k):
    from soccdpt_amd.lib import op_data_targets, op_pack_expand, op_pack_targets
    B, H, W = shape
    col_d = _dev(R.BDD_COLORS, gpu_device)
    for P, dtype in zip(P_OF_K[k] + P_OF_K[k][:1], (np.uint8, np.uint16, np.float32)):
        host, palette = _packed(B, H, W, k, P, seed=H * W + k + P)
        idx_d, pal_d, disp = _dev(host, gpu_device), _dev(palette, gpu_device), _disp(dtype, B, H, W, seed=B + W)
        disp_d = torch.from_numpy(disp).to(gpu_device)
        seg_d = op_pack_expand(idx_d, k, pal_d, H, W)
        want_seg = F.expand(host, k, palette, B, H, W)
        assert np.array_equal(seg_d.cpu().numpy(), want_seg)
        if P < (1 << k):
            assert (F.unpack(host[0], k, H * W) >= P).any() or H * W < 4      # the clamp is exercised
        for flip in (False, True):
            want = op_data_targets(seg_d, col_d, disp_d, flip=flip, want_class_map=True)
            got = op_pack_targets(idx_d, k, pal_d, col_d, H, W, disp_d, flip=flip, want_class_map=True)
            assert all(got[key] is not None for key in OUTPUTS)
            _same_targets(got, want)
        # and against numpy directly, once
        assert np.array_equal(got["onehot"].cpu().numpy(), R.onehot(want_seg, R.BDD_COLORS))
        assert np.array_equal(got["class_map"].cpu().numpy(), R.class_map(want_seg, R.BDD_COLORS, True))
        assert np.array_equal(got["unmatched"].cpu().numpy().astype(np.uint64), R.unmatched(want_seg, R.BDD_COLORS))
        assert np.array_equal(got["y_disp"].cpu().numpy().view(np.uint32), R.y_disp(disp).view(np.uint32))


@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_class_counts_and_a_colour_listed_twice(gpu_device, C):
    from soccdpt_amd.lib import op_data_targets, op_pack_expand, op_pack_targets
    colors = COLORS8[:C] if C != 4 else COLORS8[[1, 0, 1, 2]]      # C = 4: classes 0 and 2 share a colour; C = 8: classes 1 and 4 do
    B, H, W, k, P = 2, 37, 53, 4, 12
    host, palette = _packed(B, H, W, k, P, seed=C)
    assert len({tuple(c) for c in palette} & {tuple(c) for c in COLORS8}) >= 5 and len({tuple(c) for c in palette} - {tuple(c) for c in COLORS8}) >= 5
    idx_d, pal_d, col_d = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(colors, gpu_device)
    seg_d = op_pack_expand(idx_d, k, pal_d, H, W)
    for flip in (False, True):
        got = op_pack_targets(idx_d, k, pal_d, col_d, H, W, flip=flip, want_class_map=True)
        _same_targets(got, op_data_targets(seg_d, col_d, flip=flip, want_class_map=True))
    assert int(got["unmatched"].sum()) > 0      # palette colours that match no class
    if C in (4, 8):
        a, b = (0, 2) if C == 4 else (1, 4)
        one = got["onehot"].cpu().numpy()
        assert one[:, a].any() and np.array_equal(one[:, a], one[:, b])


def test_each_output_alone(gpu_device):
    from soccdpt_amd.lib import op_pack_targets
    B, H, W, k, P = 2, 37, 53, 2, 3
    host, palette = _packed(B, H, W, k, P, seed=5)
    idx_d, pal_d, col_d = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(R.BDD_COLORS, gpu_device)
    disp_d = torch.from_numpy(_disp(np.float32, B, H, W, seed=6)).to(gpu_device)
    both = op_pack_targets(idx_d, k, pal_d, col_d, H, W, disp_d, flip=True, want_class_map=True)
    for alone in OUTPUTS:
        got = op_pack_targets(idx_d, k, pal_d, col_d, H, W, disp_d if alone == "y_disp" else None, flip=True, want_onehot=alone == "onehot",
                              want_class_map=alone == "class_map", want_y_disp=alone == "y_disp", want_unmatched=alone == "unmatched")
        assert [key for key, v in got.items() if v is not None] == [alone]
        assert torch.equal(_bits(got[alone]), _bits(both[alone]))


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unaligned_output_pointers_and_longer_records_give_the_same_bytes(gpu_device, shape, offset):
    """Output base pointers `offset` elements into larger buffers (the guarded path), disparity `offset` elements in, and records `offset` words longer
    than needed."""
    from soccdpt_amd.lib import _call, op_pack_expand, op_pack_targets
    B, H, W = shape
    n = B * H * W
    k = (1, 2, 4, 8)[(H + offset) % 4]
    P = P_OF_K[k][1]
    host, palette = _packed(B, H, W, k, P, seed=7 * H + W, extra_words=offset)
    tight = np.ascontiguousarray(host[:, : host.shape[1] - offset])
    idx_d, pal_d, col_d = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(R.BDD_COLORS, gpu_device)
    assert torch.equal(op_pack_expand(idx_d, k, pal_d, H, W), op_pack_expand(_dev(tight, gpu_device), k, pal_d, H, W))
    dst = torch.full((3 * n + 16,), 0xEE, dtype=torch.uint8, device=gpu_device)      # expand to an odd address
    _call("soccdpt_pack_expand", idx_d.data_ptr(), k, host.shape[1], pal_d.data_ptr(), P, B, H, W, dst.data_ptr() + offset, device=gpu_device)
    assert np.array_equal(dst[offset: offset + 3 * n].cpu().numpy().reshape(B, H, W, 3), F.expand(host, k, palette, B, H, W))
    assert bool((dst[:offset] == 0xEE).all()) and bool((dst[offset + 3 * n:] == 0xEE).all())
    for dtype, code in ((np.uint8, 0), (np.uint16, 1), (np.float32, 2)):
        disp = _disp(dtype, B, H, W, seed=offset)
        want = op_pack_targets(_dev(tight, gpu_device), k, pal_d, col_d, H, W, torch.from_numpy(disp).to(gpu_device), flip=True, want_class_map=True)
        disp_host = np.zeros((n + 16,), dtype=dtype)
        disp_host[offset: offset + n] = disp.reshape(-1)
        disp_buf = torch.from_numpy(disp_host).to(gpu_device)
        one = torch.full((3 * n + 16,), -5.0, dtype=torch.float32, device=gpu_device)
        cm = torch.full((n + 16,), -5, dtype=torch.int32, device=gpu_device)
        yd = torch.full((n + 16,), -5.0, dtype=torch.float32, device=gpu_device)
        um = torch.full((B + 2,), -5, dtype=torch.int64, device=gpu_device)
        _call("soccdpt_pack_targets", idx_d.data_ptr(), k, host.shape[1], pal_d.data_ptr(), P, col_d.data_ptr(), 3, disp_buf.data_ptr() + offset * disp_buf.element_size(),
              code, B, H, W, 1, one.data_ptr() + 4 * offset, cm.data_ptr() + 4 * offset, yd.data_ptr() + 4 * offset, um.data_ptr() + 8, device=gpu_device)
        assert torch.equal(one[offset: offset + 3 * n], want["onehot"].reshape(-1)) and torch.equal(cm[offset: offset + n], want["class_map"].reshape(-1))
        assert torch.equal(yd[offset: offset + n].view(torch.int32), want["y_disp"].reshape(-1).view(torch.int32))
        assert torch.equal(um[1: 1 + B], want["unmatched"])
        for buf, lo, hi, fill in ((one, offset, offset + 3 * n, -5.0), (cm, offset, offset + n, -5), (yd, offset, offset + n, -5.0), (um, 1, 1 + B, -5)):
            assert bool((buf[:lo] == fill).all()) and bool((buf[hi:] == fill).all())      # nothing outside the outputs was written


@pytest.mark.parametrize("shape,k", [((1024, 48, 64), 2), ((2500, 37, 53), 4)], ids=["1024x48x64", "2500x37x53"])
def test_frames_longer_than_their_share_of_the_grid(gpu_device, shape, k):
    """The launch caps its grid at 2048 workgroups shared among the frames and walks the rest of a frame with a grid stride, as soccdpt_data_targets
    does: at B = 1024 a frame gets 2 workgroups for its 3 x 1024 pixels, at B = 2500 one workgroup for 1961 pixels (a last group of one pixel)."""
    from soccdpt_amd.lib import op_data_targets, op_pack_expand, op_pack_targets
    B, H, W = shape
    P = P_OF_K[k][1]
    rng = np.random.default_rng(B)
    idx = rng.integers(0, 1 << k, size=(B, H * W))
    words = F.record_words(H * W, k)
    host = np.stack([F.pack(idx[b], k, words) for b in range(16)])      # 16 packed by the specification, the rest by the package's packer (held to it on the CPU)
    from soccdpt_amd.datasets.frame_pack import pack_indices
    host = np.concatenate([host, np.stack([pack_indices(idx[b], k) for b in range(16, B)])])
    palette = F.random_palette(P, B, include=R.PALETTE)
    idx_d, pal_d, col_d = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(R.BDD_COLORS, gpu_device)
    disp_d = torch.from_numpy(_disp(np.uint8, B, H, W, seed=H)).to(gpu_device)
    seg_d = op_pack_expand(idx_d, k, pal_d, H, W)
    assert np.array_equal(seg_d[:16].cpu().numpy(), F.expand(host[:16], k, palette, 16, H, W))
    assert np.array_equal(seg_d[-1].cpu().numpy(), F.expand(host[-1:], k, palette, 1, H, W)[0])
    _same_targets(op_pack_targets(idx_d, k, pal_d, col_d, H, W, disp_d, flip=True, want_class_map=True),
                  op_data_targets(seg_d, col_d, disp_d, flip=True, want_class_map=True))


def test_side_stream(gpu_device):
    from soccdpt_amd.lib import op_data_targets, op_pack_expand, op_pack_targets
    B, H, W, k, P = 2, 37, 53, 8, 200
    host, palette = _packed(B, H, W, k, P, seed=3)
    idx_d, pal_d, col_d = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(R.BDD_COLORS, gpu_device)
    disp_d = torch.from_numpy(_disp(np.uint16, B, H, W, seed=4)).to(gpu_device)
    torch.cuda.synchronize(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        seg_d = op_pack_expand(idx_d, k, pal_d, H, W)
        got = op_pack_targets(idx_d, k, pal_d, col_d, H, W, disp_d, want_class_map=True)
    side.synchronize()
    assert np.array_equal(seg_d.cpu().numpy(), F.expand(host, k, palette, B, H, W))
    _same_targets(got, op_data_targets(seg_d, col_d, disp_d, want_class_map=True))


def test_errors_leave_the_outputs_untouched(gpu_device):
    from soccdpt_amd.lib import load_library
    L = load_library()
    B, H, W, k, P = 1, 5, 7, 2, 3
    host, palette = _packed(B, H, W, k, P, seed=1)
    idx, pal, col = _dev(host, gpu_device), _dev(palette, gpu_device), _dev(R.BDD_COLORS, gpu_device)
    one = torch.full((3 * H * W,), 7.0, dtype=torch.float32, device=gpu_device)
    um = torch.full((B,), 7, dtype=torch.int64, device=gpu_device)
    dst = torch.full((3 * H * W,), 7, dtype=torch.uint8, device=gpu_device)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    tail = (col.data_ptr(), 3, None, 0, B, H, W, 0, one.data_ptr(), None, None, um.data_ptr(), st)
    for what, head in {"k = 3": (idx.data_ptr(), 3, 3, pal.data_ptr(), P), "P = 5": (idx.data_ptr(), k, 3, pal.data_ptr(), 5),
                       "two words": (idx.data_ptr(), k, 2, pal.data_ptr(), P), "idx + 2": (idx.data_ptr() + 2, k, 3, pal.data_ptr(), P)}.items():
        assert L.soccdpt_pack_targets(*head, *tail) != 0 and b"soccdpt_pack_targets" in L.soccdpt_last_error(None), what
        assert L.soccdpt_pack_expand(*head, B, H, W, dst.data_ptr(), st) != 0 and b"soccdpt_pack_expand" in L.soccdpt_last_error(None), what
    torch.cuda.synchronize(gpu_device)
    assert bool((one == 7.0).all()) and bool((um == 7).all()) and bool((dst == 7).all())
    assert L.soccdpt_pack_targets(idx.data_ptr(), k, 3, pal.data_ptr(), P, *tail) == 0      # and the same call, valid, does write
    torch.cuda.synchronize(gpu_device)
    assert not bool((one == 7.0).any()) and not bool((um == 7).any())


# ---- the datasets on packs ----
CAM_W, CAM_H = 64, 48
REC_K2, REC_OTHER, REC_RAW = "1650000000001", "1650000000002", "1650000000003"      # camera size, 4 label colours / 30 x 34, 7 colours / camera size, > 256 colours


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    from soccdpt_amd.datasets.frame_pack import FramePack, write_pack
    from soccdpt_amd.utils.synth import write_synth_calib
    base = tmp_path_factory.mktemp("packed")
    calib = write_synth_calib(str(base / "calibration" / "pocoX3" / "calib.yaml"), **{"Camera.width": CAM_W, "Camera.height": CAM_H})
    R.write_recording(base, REC_K2, n=8, size=(CAM_H, CAM_W), disp_mode="I;16", seed=1, palette=R.PALETTE[:4])
    R.write_recording(base, REC_OTHER, n=8, size=(30, 34), disp_mode="L", seed=2, t0=1650000100000)
    R.write_recording(base, REC_RAW, n=8, size=(CAM_H, CAM_W), disp_mode="I;16", seed=3, t0=1650000200000, blocky=False,
                      palette=F.random_palette(300, 9, include=R.PALETTE))
    packs = {r: FramePack(write_pack(str(base / r))) for r in (REC_K2, REC_OTHER, REC_RAW)}
    assert (packs[REC_K2].k, packs[REC_OTHER].k, packs[REC_RAW].raw_labels) == (2, 4, True)
    return dict(base=str(base), calib=calib)


def _transform(device):
    from soccdpt_amd.model.loader import load_transforms
    t, _, _ = load_transforms("dpt_swin2_tiny_256")
    t.device = device
    return t


def _pair(cls, recordings, rec_id, device):
    kw = dict(dataset_path=os.path.join(recordings["base"], rec_id), settings_doc=recordings["calib"], transform=_transform(device), device=device)
    packed, png = cls(frame_pack=True, frame_pack_required=True, **kw), cls(**kw)
    assert packed.pack is not None and png.pack is None
    packed.keep_class_map = png.keep_class_map = True
    return packed, png


def _same_batch(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), f"field {k} differs"


def _same_diagnostics(a, b):
    for g, w in ((a.last_unmatched, b.last_unmatched), (a.last_class_map, b.last_class_map)):
        assert (g is None) == (w is None) and (g is None or torch.equal(g, w))


@pytest.mark.parametrize("name", ["BDD_Depth", "BDD_Segmentation", "BDD_Depth_Segmentation"])
def test_batches_from_a_pack_equal_batches_from_pngs(gpu_device, recordings, name):
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    for rec_id in (REC_K2, REC_RAW):
        packed, png = _pair(getattr(D, name), recordings, rec_id, gpu_device)
        for idx in ([5, 0, 7], [3]):
            got, want = packed.batch(idx), png.batch(idx)
            _same_batch(got, want)
            _same_diagnostics(packed, png)
        assert (packed.last_unmatched is not None) == (name != "BDD_Depth")
        if name != "BDD_Depth":
            assert int(packed.last_unmatched.sum()) > 0 and packed.last_class_map is not None
        _same_batch(packed[2], png[2])


def test_labels_at_another_size_take_the_expand_and_resize_path(gpu_device, recordings):
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    packed, png = _pair(D.BDD_Depth_Segmentation, recordings, REC_OTHER, gpu_device)
    assert packed.pack.shapes["labels"] == (30, 34) and not packed.pack.raw_labels
    got, want = packed.batch([1, 6, 2, 7]), png.batch([1, 6, 2, 7])
    assert tuple(got[5].shape) == (4, 3, CAM_H, CAM_W)
    _same_batch(got, want)
    _same_diagnostics(packed, png)
    assert bool((packed.last_unmatched > 0).all())      # blended colours at the label blocks' borders
    # the classes that do not resize read the same pack at its stored size
    for cls in (D.BDD_Segmentation, D.BDD_Depth):
        a, b = _pair(cls, recordings, REC_OTHER, gpu_device)
        _same_batch(a.batch([0, 4]), b.batch([0, 4]))
        _same_diagnostics(a, b)


def _concat(recordings, device, **kw):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BDD_Depth_Segmentation, get_bdd_dataset
    return get_bdd_dataset(BDD_Depth_Segmentation, _transform(device), recordings["base"], recordings=[REC_K2, REC_RAW, REC_OTHER], device=device, **kw)


def test_a_batch_mixing_indexed_and_raw_label_recordings(gpu_device, recordings):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import dataset_batch
    packed, png = _concat(recordings, gpu_device, frame_pack=True, frame_pack_required=True), _concat(recordings, gpu_device)
    assert all(d.pack is not None for d in packed.datasets) and all(d.pack is None for d in png.datasets)
    for d in packed.datasets + png.datasets:
        d.keep_class_map = True
    for idx in ([6, 9, 7, 8], [15, 16, 2, 17, 9]):      # k = 2 with raw; raw, another size and k = 2
        _same_batch(dataset_batch(packed, idx), dataset_batch(png, idx))
        _same_diagnostics(packed.datasets[0 if idx[0] < 8 else 1], png.datasets[0 if idx[0] < 8 else 1])      # the leaf of the first frame assembles


def test_the_prefetcher_over_packs_yields_the_batches_of_the_pngs(gpu_device, recordings):
    from soccdpt_amd.datasets.bengaluru_driving_dataset import BatchPrefetcher, dataset_batch
    packed, png = _concat(recordings, gpu_device, frame_pack=True, frame_pack_required=True), _concat(recordings, gpu_device)
    batches = [[0, 1, 2], [6, 7, 8], [9, 10, 11], [14, 15, 16, 17], [20, 3, 12]]
    want = [(dataset_batch(png, b), resolve_unmatched(png, b)) for b in batches]
    n = 0
    prefetch = BatchPrefetcher(packed, batches, depth=2)
    for got, (tensors, unmatched) in zip(prefetch, want):
        _same_batch(got, tensors)
        assert torch.equal(prefetch.last_unmatched, unmatched)
        n += 1
    assert n == len(batches)


def resolve_unmatched(dataset, indices):
    """last_unmatched of the batch `indices` that dataset_batch has just assembled: it is left on the leaf of the batch's first frame."""
    from soccdpt_amd.datasets.bengaluru_driving_dataset import resolve_index
    return resolve_index(dataset, indices[0])[0].last_unmatched
