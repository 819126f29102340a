"""CPU: the float64 references and helpers of tests/layer_bwd_refs.py against float64 autograd, naive loops and bit patterns."""
import pytest
import torch
import torch.nn.functional as F

from tests import layer_bwd_refs as LR


def _g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("with_res", [False, True])
def test_linear_formulas_match_float64_autograd(with_res):
    g = _g(1)
    M, N, K = 37, 12, 20
    x = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    res = torch.randn(M, K, generator=g, dtype=torch.float64) if with_res else None
    F.linear(x, w, b).backward(dy)
    got = LR.linear_bwd_ref(dy, x.detach(), w.detach(), res)
    torch.testing.assert_close(got["dX"], x.grad + (res if with_res else 0), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got["dW"], w.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got["db"], b.grad, rtol=1e-13, atol=1e-13)


def _naive_conv(x, w, stride, lo):
    """x [B][H][W][C] NHWC, w [N][C][3][3]; output pixel (oy, ox) reads input (oy stride + ky - lo, ox stride + kx - lo), zero outside."""
    B, H, Wd, C = x.shape
    Ho = (H + (2 * lo if lo else 1) - 3) // stride + 1 if stride == 2 else H
    y = torch.zeros(B, Ho, Ho, w.shape[0], dtype=x.dtype)
    for oy in range(Ho):
        for ox in range(Ho):
            for ky in range(3):
                for kx in range(3):
                    iy, ix = oy * stride + ky - lo, ox * stride + kx - lo
                    if 0 <= iy < H and 0 <= ix < Wd:
                        y[:, oy, ox] += x[:, iy, ix] @ w[:, :, ky, kx].t()
    return y


@pytest.mark.parametrize("stride,pad,H", [(1, 1, 5), (2, 1, 6), (2, 1, 5), (2, 0, 6)])
def test_conv_references_are_the_gradients_of_a_naive_convolution(stride, pad, H):
    """<dY, conv(X, W)> differentiated by hand: the references' dX, dW, db reproduce the directional derivatives of a loop-written convolution
    (pad 0 = 'SAME' at stride 2 on an even image: one zero row / column behind it), and conv3_bwd_ref equals conv_gen_bwd_ref at stride 1."""
    g = _g(2)
    B, C, N = 2, 3, 4
    x = torch.randn(B, H, H, C, generator=g, dtype=torch.float64)
    w = torch.randn(N, C, 3, 3, generator=g, dtype=torch.float64)
    y = _naive_conv(x, w, stride, pad)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    ref = LR.conv_gen_bwd_ref(dy, x, LR.to_tap_major(w), stride, pad)
    assert ref["dX"].shape == x.shape and ref["dW"].shape == (N, 9, C)
    vx = torch.randn(x.shape, generator=g, dtype=torch.float64)
    vw = torch.randn(w.shape, generator=g, dtype=torch.float64)
    # the convolution is bilinear in (x, w): the directional derivatives are exact differences
    torch.testing.assert_close((ref["dX"] * vx).sum(), (dy * (_naive_conv(x + vx, w, stride, pad) - y)).sum(), rtol=1e-11, atol=1e-11)
    torch.testing.assert_close((LR.from_tap_major(ref["dW"]) * vw).sum(), (dy * (_naive_conv(x, w + vw, stride, pad) - y)).sum(), rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(ref["db"], dy.sum((0, 1, 2)), rtol=1e-13, atol=1e-13)
    if stride == 1:
        res = torch.randn(x.shape, generator=g, dtype=torch.float64)
        c3 = LR.conv3_bwd_ref(dy, x, w, res)
        assert LR.conv3_bwd_ref(dy.float(), x.float(), w.float(), None, torch.float32)["dW"].dtype == torch.float32
        w32 = w.float()
        for dt in (torch.float32, torch.float64, torch.float32):     # the caller's tensors stay leaves without a gradient
            assert LR.conv3_bwd_ref(dy, x, w32, None, dt)["dW"] is not None and not w32.requires_grad
        torch.testing.assert_close(c3["dX"], ref["dX"] + res, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(LR.to_tap_major(c3["dW"]), ref["dW"], rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(c3["db"], ref["db"], rtol=1e-13, atol=1e-13)


def test_layout_conversions_against_naive_loops():
    g = _g(3)
    B, H, Wd, C, N = 2, 3, 4, 5, 3
    t = torch.randn(B, H, Wd, C, generator=g)
    h = LR.halo(t)
    assert h.shape == (B, H + 2, Wd + 2, C) and h.is_contiguous()
    for b in range(B):
        for y in range(H + 2):
            for x in range(Wd + 2):
                inside = 1 <= y <= H and 1 <= x <= Wd
                assert torch.equal(h[b, y, x], t[b, y - 1, x - 1] if inside else torch.zeros(C))
    assert torch.equal(LR.nchw(LR.nhwc(t.permute(0, 3, 1, 2))), t.permute(0, 3, 1, 2))
    w = torch.randn(N, C, 3, 3, generator=g)
    wt = LR.to_tap_major(w)
    assert wt.shape == (N, 9, C) and wt.is_contiguous()
    for n in range(N):
        for c in range(C):
            for ky in range(3):
                for kx in range(3):
                    assert wt[n, 3 * ky + kx, c] == w[n, c, ky, kx]
    assert torch.equal(LR.from_tap_major(wt), w)
    # the tap slices of both layouts are the same nine matrices
    for (la, a), (lb, b) in zip(LR.dw_tap_slices(w, False), LR.dw_tap_slices(wt, True)):
        assert la == lb and torch.equal(a, b)


def test_slices_partition_their_tensors():
    dx = torch.arange(2 * 5 * 5 * 3, dtype=torch.float64).reshape(2, 5, 5, 3)
    parts = dict(LR.dx_image_slices(dx))
    assert sorted(parts) == ["img0.interior", "img0.ring", "img1.interior", "img1.ring"]
    assert parts["img0.ring"].numel() == 16 * 3 and parts["img0.interior"].numel() == 9 * 3
    assert torch.equal(torch.cat([v.reshape(-1) for v in parts.values()]).sort().values, dx.reshape(-1))
    assert torch.equal(parts["img1.interior"], dx[1, 1:4, 1:4].reshape(-1, 3))
    rows = dict(LR.linear_row_slices(torch.zeros(577, 4)))
    assert rows["rows.last_partial_block"].shape[0] == 1 and rows["rows.full_blocks"].shape[0] == 576
    assert list(dict(LR.linear_row_slices(torch.zeros(256, 4)))) == ["rows.full_blocks"]
    assert list(dict(LR.linear_row_slices(torch.zeros(40, 4)))) == ["rows.last_partial_block"]
    assert [k for k, _ in LR.slices("conv3", "dW", torch.zeros(4, 3, 3, 3))] == ["whole"] + [f"tap{k}" for k in range(9)]
    assert [k for k, _ in LR.slices("linear", "dW", torch.zeros(4, 3))] == ["whole"]
    assert [k for k, _ in LR.slices("conv3", "db", torch.zeros(4))] == ["whole"]


@pytest.mark.parametrize("fmt,dt", [("bf16", torch.bfloat16), ("f16", torch.float16)])
def test_round_to_is_idempotent_and_survives_the_round_trip(fmt, dt):
    g = _g(4)
    t = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-3, torch.tensor([0.0, -0.0, 1.0, 65504.0 if fmt == "f16" else 3e38])])
    r = LR.round_to(fmt, t)
    assert r.dtype == torch.float32
    assert torch.equal(LR.round_to(fmt, r).view(torch.int32), r.view(torch.int32))
    assert torch.equal(r.to(dt).to(torch.float32).view(torch.int32), r.view(torch.int32))
    assert torch.equal(r.to(dt).view(torch.int16), t.to(dt).view(torch.int16))
    assert float((r - t).abs().max()) > 0            # it does round
    for f in ("f32", "x3"):
        assert LR.round_to(f, t) is t or torch.equal(LR.round_to(f, t).view(torch.int32), t.view(torch.int32))


def test_f16_operands_stay_in_the_normal_range():
    t = LR.operand("f16", (1 << 16,), _g(5))
    assert float(t.abs().min()) >= 2.0 ** -10 and float(t.abs().max()) <= 2.0 ** 10
    assert torch.equal(LR.round_to("f16", t), t)
    b = LR.operand("bf16", (4096,), _g(5))
    assert torch.equal(LR.round_to("bf16", b), b)


def test_route_bits_of_the_binding_are_the_header_s():
    import os
    import re
    from soccdpt_amd.lib import ROUTE_ALL, ROUTE_BITS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "soccdpt_hip.h")).read()
    defs = {k.lower(): int(v, 16) for k, v in re.findall(r"#define\s+SOCCDPT_ROUTE_(\w+)\s+(0x[0-9a-fA-F]+)u", header)}
    assert defs.pop("all") == ROUTE_ALL == sum(defs.values())
    assert {k.lower(): v for k, v in ROUTE_BITS.items()} == defs and len(defs) == 16
    assert all(v & (v - 1) == 0 for v in defs.values())          # one bit each


def test_scratch_bytes_of_every_gpu_case_and_of_bad_arguments():
    """soccdpt_op_train_layer_bwd_scratch_bytes launches nothing: every case of the GPU module gets a size inside that module's one scratch buffer,
    bad arguments get 0 and an error text."""
    import ctypes
    from soccdpt_amd.lib import TrainLayerBwdArgs, load_library, op_train_layer_bwd_scratch_bytes
    from tests import test_train_layer_bwd_gpu as G
    L = load_library()
    keep = ctypes.create_string_buffer(64)
    p = ctypes.addressof(keep)
    for kind, table in (("conv3", G.CONV3), ("linear", G.LINEAR), ("conv_gen", G.CONV_GEN)):
        for case, (shape, routes) in table.items():
            assert sorted(routes) == sorted(LR.FORMATS)
            for stage, defer in ((0, 0), (1, 1)):
                a = TrainLayerBwdArgs(**G._shape_fields(kind, shape))
                a.dY = a.X = a.W = a.dW = p
                a.stage_weight, a.defer = stage, defer
                need = op_train_layer_bwd_scratch_bytes(a)
                assert (36 << 20) < need <= (96 << 20), (kind, case, need)      # 32 MB of split-K partials + 4 MB of column-sum scratch are fixed
    bad = TrainLayerBwdArgs(kind=0, M=64, N=64, C=30)
    bad.dY = bad.X = bad.W = bad.dW = p
    assert L.soccdpt_op_train_layer_bwd_scratch_bytes(ctypes.byref(bad)) == 0
    assert b"multiples of 4" in L.soccdpt_last_error(None)
    assert L.soccdpt_op_train_layer_bwd_scratch_bytes(None) == 0
    with pytest.raises(RuntimeError):
        op_train_layer_bwd_scratch_bytes(bad)
