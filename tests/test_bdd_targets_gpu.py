"""GPU: soccdpt_data_targets and soccdpt_data_resize_u8c1 through the C ABI against the numpy specification (tests/bdd_targets_refs.py), exactly."""
import numpy as np
import pytest
import torch

from tests import bdd_targets_refs as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 7), (2, 37, 53), (1, 48, 64), (2, 64, 256)]      # shorter than a wave; rows ending inside a 4-pixel group; frame strides off 16 bytes
COLORS8 = np.array([(0, 0, 0), (0, 0, 142), (220, 20, 60), (142, 0, 0), (0, 0, 142), (60, 20, 220), (0, 0, 141), (9, 9, 9)], dtype=np.uint8)   # 1 and 4: listed twice


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


def _check(got, seg, colors, disp, flip):
    if got["onehot"] is not None:
        assert np.array_equal(got["onehot"].cpu().numpy(), R.onehot(seg, colors))
    if got["class_map"] is not None:
        assert np.array_equal(got["class_map"].cpu().numpy(), R.class_map(seg, colors, flip))
    if got["y_disp"] is not None:
        assert np.array_equal(got["y_disp"].cpu().numpy().view(np.uint32), R.y_disp(disp).view(np.uint32))      # bits: NaN payloads too
    if got["unmatched"] is not None:
        assert np.array_equal(got["unmatched"].cpu().numpy().astype(np.uint64), R.unmatched(seg, colors))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32], ids=["u8", "u16", "f32"])
def test_all_outputs_together_and_alone(gpu_device, shape, dtype):
    from soccdpt_amd.lib import op_data_targets
    B, H, W = shape
    seg, disp = R.label_frames(B, H, W, seed=H * W), _disp(dtype, B, H, W, seed=B + W)
    seg_d, disp_d, col_d = torch.from_numpy(seg).to(gpu_device), torch.from_numpy(disp).to(gpu_device), torch.from_numpy(R.BDD_COLORS).to(gpu_device)
    for flip in (False, True):
        both = op_data_targets(seg_d, col_d, disp_d, flip=flip, want_class_map=True)
        _check(both, seg, R.BDD_COLORS, disp, flip)
        assert all(both[k] is not None for k in ("onehot", "class_map", "y_disp", "unmatched"))
    for alone in ("onehot", "class_map", "y_disp", "unmatched"):
        got = op_data_targets(seg_d, col_d, disp_d if alone == "y_disp" else None, flip=True, want_onehot=alone == "onehot", want_class_map=alone == "class_map",
                              want_y_disp=alone == "y_disp", want_unmatched=alone == "unmatched")
        assert [k for k, v in got.items() if v is not None] == [alone]
        _check(got, seg, R.BDD_COLORS, disp, True)


@pytest.mark.parametrize("C", [1, 3, 4, 8])
def test_class_counts_and_a_colour_listed_twice(gpu_device, C):
    from soccdpt_amd.lib import op_data_targets
    colors = COLORS8[:C] if C != 4 else COLORS8[[1, 0, 1, 2]]      # C = 4: classes 0 and 2 share a colour; C = 8: classes 1 and 4 do
    seg = R.label_frames(2, 37, 53, seed=C)
    for flip in (False, True):
        got = op_data_targets(torch.from_numpy(seg).to(gpu_device), torch.from_numpy(np.ascontiguousarray(colors)).to(gpu_device), flip=flip, want_class_map=True)
        _check(got, seg, colors, None, flip)
    if C in (4, 8):
        a, b = (0, 2) if C == 4 else (1, 4)
        one = got["onehot"].cpu().numpy()
        assert one[:, a].any() and np.array_equal(one[:, a], one[:, b])


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unaligned_base_pointers_give_the_same_bytes(gpu_device, shape, offset):
    """The same inputs through base pointers `offset` bytes (u8 inputs) / elements (everything wider) into larger buffers: the guarded path."""
    from soccdpt_amd.lib import _call, op_data_targets
    B, H, W = shape
    n = B * H * W
    seg = R.label_frames(B, H, W, seed=7 * H + W)
    col_d = torch.from_numpy(R.BDD_COLORS).to(gpu_device)
    for dtype, code in ((np.uint8, 0), (np.uint16, 1), (np.float32, 2)):
        disp = _disp(dtype, B, H, W, seed=offset)
        want = op_data_targets(torch.from_numpy(seg).to(gpu_device), col_d, torch.from_numpy(disp).to(gpu_device), flip=True, want_class_map=True)
        seg_host = np.full((3 * n + 16,), 0xEE, dtype=np.uint8)
        seg_host[offset: offset + 3 * n] = seg.reshape(-1)
        disp_host = np.zeros((n + 16,), dtype=dtype)
        disp_host[offset: offset + n] = disp.reshape(-1)
        seg_buf, disp_buf = torch.from_numpy(seg_host).to(gpu_device), torch.from_numpy(disp_host).to(gpu_device)
        one = torch.full((3 * n + 16,), -5.0, dtype=torch.float32, device=gpu_device)
        cm = torch.full((n + 16,), -5, dtype=torch.int32, device=gpu_device)
        yd = torch.full((n + 16,), -5.0, dtype=torch.float32, device=gpu_device)
        um = torch.full((B + 2,), -5, dtype=torch.int64, device=gpu_device)
        es = disp_buf.element_size()
        _call("soccdpt_data_targets", seg_buf.data_ptr() + offset, col_d.data_ptr(), 3, disp_buf.data_ptr() + offset * es, code, B, H, W, 1,
              one.data_ptr() + 4 * offset, cm.data_ptr() + 4 * offset, yd.data_ptr() + 4 * offset, um.data_ptr() + 8, device=gpu_device)
        assert torch.equal(one[offset: offset + 3 * n], want["onehot"].reshape(-1)) and torch.equal(cm[offset: offset + n], want["class_map"].reshape(-1))
        assert torch.equal(yd[offset: offset + n].view(torch.int32), want["y_disp"].reshape(-1).view(torch.int32))
        assert torch.equal(um[1: 1 + B], want["unmatched"])
        # nothing outside the outputs was written
        for buf, lo, hi, fill in ((one, offset, offset + 3 * n, -5.0), (cm, offset, offset + n, -5), (yd, offset, offset + n, -5.0), (um, 1, 1 + B, -5)):
            assert bool((buf[:lo] == fill).all()) and bool((buf[hi:] == fill).all())


def test_unmatched_is_exact_and_repeatable_and_needs_no_zeroing(gpu_device):
    from soccdpt_amd.lib import _call
    B, H, W = 2, 64, 256
    seg = R.label_frames(B, H, W, seed=11)
    seg[1] = (5, 5, 5)                                   # a frame without any class colour: H * W unmatched
    seg_d, col_d = torch.from_numpy(seg).to(gpu_device), torch.from_numpy(R.BDD_COLORS).to(gpu_device)
    runs = []
    for fill in (0, 12345, -1):
        um = torch.full((B,), fill, dtype=torch.int64, device=gpu_device)      # whatever the caller left there
        _call("soccdpt_data_targets", seg_d.data_ptr(), col_d.data_ptr(), 3, None, 0, B, H, W, 0, None, None, None, um.data_ptr(), device=gpu_device)
        runs.append(um.cpu().numpy().astype(np.uint64))
    assert np.array_equal(runs[0], R.unmatched(seg, R.BDD_COLORS)) and int(runs[0][1]) == H * W
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_side_stream(gpu_device):
    from soccdpt_amd.lib import op_data_targets
    B, H, W = 2, 37, 53
    seg, disp = R.label_frames(B, H, W, seed=3), _disp(np.uint16, B, H, W, seed=4)
    seg_d, disp_d, col_d = torch.from_numpy(seg).to(gpu_device), torch.from_numpy(disp).to(gpu_device), torch.from_numpy(R.BDD_COLORS).to(gpu_device)
    torch.cuda.synchronize(gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    with torch.cuda.stream(side):
        got = op_data_targets(seg_d, col_d, disp_d, flip=False, want_class_map=True)
    side.synchronize()
    _check(got, seg, R.BDD_COLORS, disp, False)


def test_errors_leave_the_outputs_untouched(gpu_device):
    from soccdpt_amd.lib import load_library
    L = load_library()
    B, H, W = 1, 5, 7
    seg = torch.from_numpy(R.label_frames(B, H, W, seed=1)).to(gpu_device)
    col = torch.from_numpy(COLORS8).to(gpu_device)
    one = torch.full((9 * H * W,), 7.0, dtype=torch.float32, device=gpu_device)
    cm = torch.full((H * W,), 7, dtype=torch.int32, device=gpu_device)
    yd = torch.full((H * W,), 7.0, dtype=torch.float32, device=gpu_device)
    um = torch.full((B,), 7, dtype=torch.int64, device=gpu_device)
    disp = torch.zeros((B, H, W), dtype=torch.uint8, device=gpu_device)
    st = torch.cuda.current_stream(gpu_device).cuda_stream
    outs = (one.data_ptr(), cm.data_ptr(), yd.data_ptr(), um.data_ptr())
    cases = {"C = 0": (seg.data_ptr(), col.data_ptr(), 0, disp.data_ptr(), 0),
             "C = 9": (seg.data_ptr(), col.data_ptr(), 9, disp.data_ptr(), 0),
             "NULL seg": (None, col.data_ptr(), 3, disp.data_ptr(), 0),
             "y_disp without disp": (seg.data_ptr(), col.data_ptr(), 3, None, 0),
             "unknown dtype": (seg.data_ptr(), col.data_ptr(), 3, disp.data_ptr(), 3)}
    for what, head in cases.items():
        assert L.soccdpt_data_targets(*head, B, H, W, 0, *outs, st) != 0, what
        assert b"soccdpt_data_targets" in L.soccdpt_last_error(None), what
    torch.cuda.synchronize(gpu_device)
    assert bool((one == 7.0).all()) and bool((cm == 7).all()) and bool((yd == 7.0).all()) and bool((um == 7).all())
    assert L.soccdpt_data_targets(seg.data_ptr(), col.data_ptr(), 8, disp.data_ptr(), 0, B, H, W, 0, *outs, st) == 0      # and the same call, valid, does write
    torch.cuda.synchronize(gpu_device)
    assert not bool((cm == 7).any()) and not bool((one[: 8 * H * W] == 7.0).any()) and bool((one[8 * H * W:] == 7.0).all())


@pytest.mark.parametrize("src,dst", [((5, 7), (9, 4)), ((37, 53), (48, 64)), ((37, 53), (37, 53))], ids=["5x7-9x4", "37x53-48x64", "identity"])
def test_one_channel_resize(gpu_device, src, dst):
    from soccdpt_amd.lib import op_data_resize_u8c1
    from soccdpt_amd.utils.visualise import resize_taps
    rng = np.random.default_rng(src[0] + dst[1])
    img = rng.integers(0, 256, size=(3,) + src, dtype=np.uint8)
    img[0, 0, :] = (0, 255) * (src[1] // 2) + (0,) * (src[1] % 2)           # hardest rows for the rounding
    yt = xt = None
    if src != dst:
        yt, xt = torch.from_numpy(resize_taps(src[0], dst[0])).to(gpu_device), torch.from_numpy(resize_taps(src[1], dst[1])).to(gpu_device)
        assert np.array_equal(resize_taps(src[0], dst[0]), R.resize_taps(src[0], dst[0]))
    got = op_data_resize_u8c1(torch.from_numpy(img).to(gpu_device), dst[0], dst[1], yt, xt).cpu().numpy()
    for b in range(3):
        assert np.array_equal(got[b], R.resize_u8c1(img[b], (dst[1], dst[0]))), b
    if src != dst:      # an unaligned destination and source: one byte into larger buffers
        from soccdpt_amd.lib import _call
        n_s, n_d = 3 * src[0] * src[1], 3 * dst[0] * dst[1]
        sbuf = torch.zeros((n_s + 8,), dtype=torch.uint8, device=gpu_device)
        sbuf[1: 1 + n_s] = torch.from_numpy(img).to(gpu_device).reshape(-1)
        dbuf = torch.full((n_d + 8,), 0xEE, dtype=torch.uint8, device=gpu_device)
        _call("soccdpt_data_resize_u8c1", sbuf.data_ptr() + 1, 3, src[0], src[1], yt.data_ptr(), xt.data_ptr(), dst[0], dst[1], dbuf.data_ptr() + 1, device=gpu_device)
        assert np.array_equal(dbuf[1: 1 + n_d].cpu().numpy().reshape(got.shape), got)
        assert int(dbuf[0]) == 0xEE and bool((dbuf[1 + n_d:] == 0xEE).all())


@pytest.mark.parametrize("shape", [(1024, 48, 64), (2500, 37, 53)], ids=lambda s: "x".join(map(str, s)))
def test_frames_longer_than_their_share_of_the_grid(gpu_device, shape):
    """The launch caps its grid at 2048 workgroups shared among the frames and walks the rest of a frame with a grid stride: at B = 1024 a frame gets 2
    workgroups for its 3 x 1024 pixels, at B = 2500 one workgroup for 1961 pixels (a last group of one pixel)."""
    from soccdpt_amd.lib import op_data_targets
    B, H, W = shape
    seg, disp = R.label_frames(B, H, W, seed=B), _disp(np.uint8, B, H, W, seed=H)
    got = op_data_targets(torch.from_numpy(seg).to(gpu_device), torch.from_numpy(R.BDD_COLORS).to(gpu_device), torch.from_numpy(disp).to(gpu_device), flip=True,
                          want_class_map=True)
    _check(got, seg, R.BDD_COLORS, disp, True)
