"""CPU: the float64 references and bounds of tests/fused_refs.py are tight enough to catch subtle faults.

Each reference's own output stands in for the kernel's (rounded to f32, as the kernels store it) and must pass its check; the same output
with one injected fault must be rejected: one 8 x 16 tile off by 1 %, a border row re-sampled with align_corners=False, a batch row
computed from another row's input, classes 1 and 2 swapped, the second partial plane dropped, LayerNorm without its residual, an x3 lo
half zeroed."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import fused_refs as FR


def _rejects(got, ref, bound, what):
    with pytest.raises(AssertionError):
        FR.check_bound(got, ref, bound, what)


def test_bilinear_sample_is_torch_interpolate():
    """The sampling reference equals F.interpolate(align_corners=True) in float64, and the position allowance is small and non-zero only
    where f32 cannot represent the position."""
    g = torch.Generator().manual_seed(1)
    for (h, w, H, W) in ((8, 16, 16, 32), (5, 1, 16, 16), (96, 96, 192, 192), (7, 3, 14, 6)):
        src = torch.randn(2, h, w, 3, generator=g, dtype=torch.float64)
        b = torch.arange(2)[:, None, None].expand(2, H, W)
        Y = torch.arange(H)[None, :, None].expand(2, H, W)
        X = torch.arange(W)[None, None, :].expand(2, H, W)
        v, e = FR.bilinear_sample(src, b, Y, X, H, W)
        ref = F.interpolate(src.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        assert float((v - ref).abs().max()) < 1e-12
        assert float((e / (src.abs().max() + 1)).max()) < 2e-4


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_depth_tail_bound_rejects_faults(fmt):
    B, h, w = 2, 8, 16
    d1, wt, bias, w4, b4 = FR.depth_tail_inputs(B, h, w, fmt, seed=3)
    n, tx_n, ty_n = FR.depth_tail_tiles(B, h, w)
    tiles = torch.arange(n)
    ref, bnd = FR.depth_tail_ref(d1, wt, bias, w4, b4, fmt)
    assert ref.shape == (n, 8, 16)
    assert float((ref > 0).double().mean()) > 0.5, "the inputs must leave most outputs positive for the faults to be visible"
    FR.check_bound(ref.float(), ref, bnd, "unmodified")
    # one 8 x 16 tile off by 1 %
    got = ref.float().clone()
    got[5] *= 1.01
    _rejects(got, ref, bnd, "tile off by 1 %")
    # one border row re-sampled with align_corners=False (the up-sampled patch rows next to it differ)
    ref_hp, _ = FR.depth_tail_ref(d1, wt, bias, w4, b4, fmt, align_corners=False)
    got = ref.float().clone()
    top = (tiles // tx_n) % ty_n == 0
    got[top & (tiles < n // B), 0] = ref_hp[top & (tiles < n // B), 0].float()
    _rejects(got, ref, bnd, "border row with align_corners=False")
    # batch row 1 computed from batch row 0's input
    d1x = d1.clone()
    d1x[1] = d1[0]
    ref_x, _ = FR.depth_tail_ref(d1x, wt, bias, w4, b4, fmt)
    got = ref.float().clone()
    got[n // B:] = ref_x[n // B:].float()
    _rejects(got, ref, bnd, "batch row from another row's input")
    # the tile picker covers borders, batch-row ends and workgroup boundaries
    sel = FR.pick_tiles(3, 16, 32, n_random=4)
    assert {0, 15, 511, 512, 1023, 1024, 1535, 255, 256, 767, 768}.issubset(set(sel.tolist()))


def test_seg_bounds_reject_faults():
    fmt, B, H, W = "bf16", 1, 8, 8
    xh, wt, bias, dot_w, sbias = FR.seg_inputs(B, H, W, fmt, Cin=64, N=256, seed=2)
    M = B * H * W
    ms = torch.arange(M)
    part, pb = FR.dot3_ref(xh, wt, bias, dot_w, fmt, 128, ms, H, W)   # [2][M][3]
    FR.check_bound(part.float(), part, pb, "dot3 unmodified")
    sw = part.float().clone()
    sw[..., [1, 2]] = sw[..., [2, 1]]
    _rejects(sw, part, pb, "dot3 classes 1 and 2 swapped")
    # the finishing sum: kernel planes [T][M][4] with a NaN padding lane that must not be read
    kp = torch.cat([part.float(), torch.full((2, M, 1), float("nan"))], dim=2)
    logits, lb = FR.seg_logits_ref(kp, sbias)
    FR.check_bound(logits.float(), logits, lb, "logits unmodified")
    dropped = (kp[0, :, :3].double() + sbias).float()
    _rejects(dropped, logits, lb, "second partial plane dropped")
    # logits against the operands (dot3 bound + finishing sum)
    full = part.sum(0) + sbias
    FR.check_bound(logits.float(), full, pb.sum(0) + lb, "logits vs operands")
    for sigmoid in (0, 1):
        act, ab = FR.seg_up_act_ref(logits.float().double(), B, H, W, sigmoid)
        assert act.shape == (B, 3, 2 * H, 2 * W)
        FR.check_bound(act.float(), act, ab, "activation unmodified")
        sw = act.float().clone()
        sw[:, [1, 2]] = sw[:, [2, 1]]
        _rejects(sw, act, ab, "classes 1 and 2 swapped")


def test_ln_bound_rejects_missing_residual():
    g = torch.Generator().manual_seed(4)
    M, K, N = 100, 96, 96
    x = FR.round16(torch.randn(M, K, generator=g, dtype=torch.float64), "f16")
    wt = FR.round16(torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K), "f16")
    bias = torch.randn(N, generator=g, dtype=torch.float64).float().double()
    lg = (1 + 0.3 * torch.randn(N, generator=g, dtype=torch.float64)).float().double()
    lb = (0.2 * torch.randn(N, generator=g, dtype=torch.float64)).float().double()
    xres = torch.randn(M, N, generator=g, dtype=torch.float64).float().double()
    o, ob = FR.ln_epilogue_ref(x, wt, bias, lg, lb, xres, "f16", True)
    FR.check_bound(o.float(), o, ob, "LN unmodified")
    _rejects((o - xres).float(), o, ob, "LN without the residual")
    got = o.float().clone()
    got[17, 5] = got[17, 5] * (1 + 2e-4)
    _rejects(got, o, ob, "LN one element off by 2e-4")


def test_operand_copy_checks_reject_faults():
    from soccdpt_amd.lib import x3_encode
    g = torch.Generator().manual_seed(5)
    v = torch.randn(6, 32, generator=g) * 3
    raw = x3_encode(v)
    FR.check_x3(raw, v.shape, v, "x3 unmodified")
    hi, lo = FR.x3_parts(raw, v.shape)
    assert float(lo.abs().max()) > 0
    bad = raw.clone().reshape(-1, 2, 8)
    odd = (torch.arange(bad.shape[0]) & 1).bool()
    bad[~odd, 1] = 0          # the lo chunk of every even unit (half16.h: hi first in even units)
    bad[odd, 0] = 0
    with pytest.raises(AssertionError):
        FR.check_x3(bad.reshape(-1), v.shape, v, "x3 lo zeroed")
    for fmt in ("bf16", "f16"):
        c = v.to(torch.bfloat16 if fmt == "bf16" else torch.float16)
        FR.check_copy16(c, v, fmt, "copy unmodified")
        c2 = c.clone()
        c2.view(torch.int16)[3, 7] += 1
        with pytest.raises(AssertionError):
            FR.check_copy16(c2, v, fmt, "copy one ulp off")
