"""GPU: the fused kernels and igemm epilogues of the 16-bit heads, element by element against the float64 references and a-priori bounds of
tests/fused_refs.py (the depth tail, the seg classifier in the conv epilogue and its finishing pass, the LayerNorm epilogue, the sampled
residual, the cross-format operand stores).  Outputs are pre-filled with NaN (halo borders with a sentinel), every launch runs three times
and must give the same bits, and each check prints its worst error as a fraction of its bound."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import fused_refs as FR

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _prec(fmt):
    from soccdpt_amd import lib
    return {"bf16": lib.PREC_BF16, "f16": lib.PREC_F16, "f32": lib.PREC_F32, "x3": lib.PREC_F16X3, "x2w": lib.PREC_F16X2W}[fmt]


def _report(what, ratio):
    print(f"{what}: worst error / bound = {ratio:.3g}")


def _dev(t, fmt, dev):
    """float64 operand values -> the device tensor the kernel reads in format fmt (x3: the split-fp16 bytes)."""
    from soccdpt_amd.lib import x3_encode
    if fmt in DT:
        return t.to(DT[fmt]).contiguous().to(dev)
    if fmt == "f32":
        return t.float().contiguous().to(dev)
    return x3_encode(t.float()).to(dev)


def _operand_values(t, fmt):
    """The exact values the kernel multiplies: 16-bit / f32 rounding, or the decoded x3 pair."""
    from soccdpt_amd.lib import x3_decode, x3_encode
    if fmt in DT:
        return FR.round16(t, fmt)
    if fmt == "f32":
        return t.float().double()
    return x3_decode(x3_encode(t.float()), t.shape)


def _three_runs(launch, outs):
    """Run `launch` three times; every tensor in `outs` must come out bitwise the same each time.  Returns CPU copies of the last run."""
    first = None
    for _ in range(3):
        launch()
        torch.cuda.synchronize()
        cur = [o.cpu().clone() for o in outs]
        if first is None:
            first = cur
        else:
            for a, b in zip(first, cur):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.is_floating_point() else torch.equal(a, b), "a rerun changed bits"
    return first


# ---------------------------------------------------------------------------------------------------------------------------------
# depth tail
# ---------------------------------------------------------------------------------------------------------------------------------
DEPTH_CASES = [(B, r, r) for r in (128, 192) for B in (1, 2, 3, 5, 8)] + [
    (2, 48, 96),     # non-square, wide
    (3, 96, 40),     # non-square, tall
    (1, 8, 8),       # 2 tiles: a grid smaller than 256 workgroups, one tile each, no successor
    (1, 1028, 8),    # 257 tiles: workgroup 0 runs tiles 0 and 256
]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("B,h,w", DEPTH_CASES)
def test_depth_tail(gpu_device, fmt, B, h, w):
    from soccdpt_amd.lib import op_depth_tail
    d1, wt, bias, w4, b4 = FR.depth_tail_inputs(B, h, w, fmt, seed=B * 1000 + h + w)
    n, tx_n, ty_n = FR.depth_tail_tiles(B, h, w)
    d1_d, wt_d = _dev(d1, fmt, gpu_device), _dev(wt, fmt, gpu_device)
    bias_d, w4_d = bias.float().to(gpu_device), w4.float().to(gpu_device)
    out = torch.full((B, 2 * h, 2 * w), float("nan"), device=gpu_device)
    (got,) = _three_runs(lambda: op_depth_tail(d1_d, wt_d, bias_d, w4_d, b4, out, B, h, w, precision=_prec(fmt)), [out])
    assert bool(torch.isfinite(got).all()), "depth tail left output pixels unwritten"
    tiles = torch.arange(n) if n <= 512 else FR.pick_tiles(B, tx_n, ty_n, n_random=48, seed=B + h)
    ref, bnd = FR.depth_tail_ref(d1, wt, bias, w4, b4, fmt, tiles)
    _report(f"depth_tail {fmt} B={B} {h}x{w} ({tiles.numel()} of {n} tiles)",
            FR.check_bound(FR.gather_tiles(got, tiles, tx_n, ty_n), ref, bnd, f"depth_tail {fmt} B={B} {h}x{w}"))


def test_depth_tail_refuses_bad_arguments(gpu_device):
    from soccdpt_amd.lib import PREC_F16X3, PREC_F32, op_depth_tail
    d1 = torch.zeros(1, 8, 8, 128, dtype=torch.bfloat16, device=gpu_device)
    wt = torch.zeros(32, 1152, dtype=torch.bfloat16, device=gpu_device)
    v = torch.zeros(32, device=gpu_device)
    out = torch.full((1, 16, 16), 7.0, device=gpu_device)
    for prec in (PREC_F32, PREC_F16X3, 99):
        with pytest.raises(RuntimeError, match="precision"):
            op_depth_tail(d1, wt, v, v, 0.0, out, 1, 8, 8, precision=prec)
    with pytest.raises(RuntimeError, match="multiple of 8 x 16"):
        op_depth_tail(d1, wt, v, v, 0.0, out, 1, 8, 4)      # 2w = 8 is not a multiple of 16
    with pytest.raises(RuntimeError, match="multiple of 8 x 16"):
        op_depth_tail(d1, wt, v, v, 0.0, out, 1, 6, 8)      # 2h = 12 is not a multiple of 8
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call launched"


# ---------------------------------------------------------------------------------------------------------------------------------
# seg classifier (dot3) + finishing pass
# ---------------------------------------------------------------------------------------------------------------------------------
def _seg_pixels(B, H, W, bm, seed):
    """The pixels a large seg case compares: whole bm-row M tiles (the first and last of every batch row, those at workgroup-count
    boundaries 255, 256, 511, ... and a seeded random set) plus every image-border pixel."""
    M, HW = B * H * W, H * W
    nt = M // bm
    tiles = [0, nt - 1] + [t for b in range(B) for t in (b * HW // bm, (b + 1) * HW // bm - 1)]
    tiles += [t for k in range(256, nt + 1, 256) for t in (k - 1, k) if t < nt]
    tiles += torch.randint(0, nt, (6,), generator=torch.Generator().manual_seed(seed)).tolist()
    ms = [torch.arange(t * bm, (t + 1) * bm) for t in sorted(set(tiles))]
    y, x = torch.arange(HW) // W, torch.arange(HW) % W
    edge = torch.nonzero((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).flatten()
    ms += [b * HW + edge for b in range(B)]
    return torch.unique(torch.cat(ms))


SEG_CASES = [(1, 128), (3, 128), (4, 128), (1, 192)]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("tune", [21, 47])
@pytest.mark.parametrize("B,r", SEG_CASES)
def test_seg_classifier(gpu_device, fmt, tune, B, r):
    from soccdpt_amd.lib import op_igemm, op_seg_tail
    H = W = r
    Cin, N = 256, 256
    xh, wt, bias, dot_w, sbias = FR.seg_inputs(B, H, W, fmt, Cin=Cin, N=N, seed=B * 7 + r + tune)
    M = B * H * W
    bn = 128 if tune == 21 else 256
    T = N // bn
    xh_d, wt_d = _dev(xh, fmt, gpu_device), _dev(wt, fmt, gpu_device)
    bias_d, dw_d = bias.float().to(gpu_device), dot_w.float().contiguous().to(gpu_device)
    part = torch.full((2, M, 4), float("nan"), device=gpu_device)    # room for two planes: a 256-wide launch must leave the second alone
    (kp,) = _three_runs(lambda: op_igemm(xh_d, wt_d, M, N, Cin, taps=9, H=H, W=W, bias=bias_d, act=1, dot_w=dw_d, out_dot=part, dot3=1, tune=tune,
                                         precision=_prec(fmt)), [part])
    assert bool(torch.isnan(kp[T:]).all()), "the launch wrote more partial planes than its channel tile implies"
    assert bool((kp[:T, :, 3] == 0).all()), "padding lane of a partial plane"
    ms = torch.arange(M) if M <= 4096 else _seg_pixels(B, H, W, 128, seed=B + r)
    ref, bnd = FR.dot3_ref(xh, wt, bias, dot_w, fmt, bn, ms, H, W)
    what = f"seg dot3 {fmt} tune {tune} B={B} {r}x{r}"
    _report(what, FR.check_bound(kp[:T, ms, :3], ref, bnd, what))
    # the finishing pass reads the planes the kernel wrote; their padding lane is poisoned and must not leak
    kp_in = kp[:T].clone()
    kp_in[..., 3] = float("nan")
    part_in = kp_in.to(gpu_device)
    sbias_d = sbias.float().to(gpu_device)
    logits_full = ref.sum(0) + sbias
    for sigmoid in (0, 1):
        tmp = torch.full((M, 3), float("nan"), device=gpu_device)
        seg = torch.full((B, 3, 2 * H, 2 * W), float("nan"), device=gpu_device)
        lg, sg = _three_runs(lambda: op_seg_tail(part_in, T, sbias_d, tmp, seg, B, H, W, sigmoid), [tmp, seg])
        lref, lb = FR.seg_logits_ref(kp_in, sbias)
        w2 = f"{what} sigmoid={sigmoid}"
        _report(w2 + " logits (finishing sum)", FR.check_bound(lg, lref, lb, w2 + " logits"))
        _report(w2 + " logits (vs operands)", FR.check_bound(lg[ms], logits_full, bnd.sum(0) + lb[ms], w2 + " logits vs operands"))
        aref, ab = FR.seg_up_act_ref(lg.double(), B, H, W, sigmoid)
        _report(w2 + " up-sampled activation", FR.check_bound(sg, aref, ab, w2 + " activation"))


def test_seg_classifier_refuses_bad_descriptors(gpu_device):
    from soccdpt_amd.lib import PREC_F16X3, op_igemm
    B, H, W, Cin, N = 1, 8, 8, 64, 256
    M = B * H * W
    xh = torch.zeros(B, H + 2, W + 2, Cin, dtype=torch.bfloat16, device=gpu_device)
    wt = torch.zeros(N, 9 * Cin, dtype=torch.bfloat16, device=gpu_device)
    dw = torch.zeros(3, N, device=gpu_device)
    part = torch.full((2, M, 4), 7.0, device=gpu_device)
    with pytest.raises(RuntimeError, match="dot3"):
        op_igemm(xh, wt, M, 192, Cin, taps=9, H=H, W=W, act=1, dot_w=dw, out_dot=part, dot3=1)            # N % 128
    with pytest.raises(RuntimeError, match="dot3"):
        op_igemm(xh, wt, M, N, 96, taps=9, H=H, W=W, act=1, dot_w=dw, out_dot=part, dot3=1)               # Cin % 64
    with pytest.raises(RuntimeError, match="dot3"):
        op_igemm(xh.view(M + 36, -1)[:, :Cin], wt, M, N, Cin, taps=1, ldx=Cin, act=1, dot_w=dw, out_dot=part, dot3=1)   # not a 3x3 conv
    with pytest.raises(RuntimeError, match="dot3"):
        op_igemm(xh, wt, M, N, Cin, taps=9, H=H, W=W, act=1, dot_w=dw, out_dot=part, dot3=1, precision=PREC_F16X3)
    torch.cuda.synchronize()
    assert bool((part == 7.0).all()), "a refused call launched"


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
SENT16 = 0x5A5A
SENT32 = 0x5A5A5A5A


def _op_buffer(fmt_out, shape, dev, sentinel=False):
    """Operand-copy buffer of format fmt_out ('bf16' / 'f16' / 'f32' / 'x3'), NaN-filled (or a sentinel bit pattern)."""
    n = math.prod(shape)
    if fmt_out in DT:
        t = torch.full((n,), float("nan"), dtype=DT[fmt_out], device=dev)
        if sentinel:
            t.view(torch.int16).fill_(SENT16)
        return t
    if fmt_out == "f32":
        t = torch.full((n,), float("nan"), device=dev)
        if sentinel:
            t.view(torch.int32).fill_(SENT32)
        return t
    t = torch.full((2 * n,), float("nan"), dtype=torch.float16, device=dev)   # x3: two fp16 words per element
    if sentinel:
        t.view(torch.int16).fill_(SENT16)
    return t


def _check_copy(raw, fmt_out, shape, f32_vals, what):
    """The operand copy raw (flat, format fmt_out) of the kernel's f32 values f32_vals (of `shape`)."""
    if fmt_out in DT:
        FR.check_copy16(raw.cpu().reshape(shape), f32_vals, fmt_out, what)
    elif fmt_out == "f32":
        assert torch.equal(raw.cpu().reshape(shape), f32_vals.float()), what
    else:
        _report(what, FR.check_x3(raw, shape, f32_vals, what))


def _halo_interior(raw, fmt_out, B, H, W, N):
    """True when every word of the one-pixel border of the flat halo buffer raw still holds the sentinel."""
    words = raw.cpu().view(torch.int32 if fmt_out == "f32" else torch.int16)
    img = words.reshape(B, H + 2, W + 2, -1)
    border = torch.ones(B, H + 2, W + 2, dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    return bool((img[border] == (SENT32 if fmt_out == "f32" else SENT16)).all())


LN_FMTS = ["bf16", "f16", "x2w", "x3", "f32"]
# (launch format, out_fmt, halo_fmt): the same-format launches and the mixed-mode cross-format stores
LN_MODES = [(f, -1, -1) for f in LN_FMTS] + [("f16", 3, 3), ("f16", -1, 3), ("x2w", 3, -1), ("x3", 1, 1), ("x3", -1, 1)]


def _store_fmt(fmt, code):
    if code == 3:
        return "x3"
    if code == 1:
        return "f16"
    return {"x2w": "f16"}.get(fmt, fmt)


@pytest.mark.parametrize("fmt,out_fmt,halo_fmt", LN_MODES)
@pytest.mark.parametrize("N", [96, 128])
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("residual", [0, 1])
def test_ln_epilogue(gpu_device, fmt, out_fmt, halo_fmt, N, halo, residual):
    from soccdpt_amd.lib import op_igemm, x3_encode
    g = torch.Generator().manual_seed(N + 10 * halo + 100 * residual + 1000 * LN_MODES.index((fmt, out_fmt, halo_fmt)))
    B, H, W = (3, 6, 6) if halo else (1, 0, 0)
    M = B * H * W if halo else 200          # 108 / 200 rows: not a multiple of the 64-row tile
    K = N
    x = torch.randn(M, K, generator=g, dtype=torch.float64) + 0.2
    wt = torch.randn(N, K, generator=g, dtype=torch.float64) / math.sqrt(K)
    xfmt, wfmt = {"x2w": ("f16", "x3")}.get(fmt, (fmt, fmt))
    xv, wv = _operand_values(x, xfmt), _operand_values(wt, wfmt)
    bias = torch.randn(N, generator=g, dtype=torch.float64).float().double()
    lg = (1 + 0.3 * torch.randn(N, generator=g, dtype=torch.float64)).float().double()
    lb = (0.2 * torch.randn(N, generator=g, dtype=torch.float64)).float().double()
    xres = torch.randn(M, N, generator=g, dtype=torch.float64).float().double()
    x_d = _dev(xv, xfmt, gpu_device) if xfmt != "x3" else x3_encode(xv.float()).to(gpu_device)
    w_d = _dev(wv, wfmt, gpu_device) if wfmt != "x3" else x3_encode(wv.float()).to(gpu_device)
    b_d, g_d, e_d = bias.float().to(gpu_device), lg.float().to(gpu_device), lb.float().to(gpu_device)
    xf = torch.empty(M, N, device=gpu_device)
    ofmt, hfmt = _store_fmt(fmt, out_fmt), _store_fmt(fmt, halo_fmt)
    op = _op_buffer(ofmt, (M, N), gpu_device) if fmt != "f32" else None       # f32 launches keep ln_xf only (model.cpp: no operand copy)
    hb = _op_buffer(hfmt, (B, H + 2, W + 2, N), gpu_device, sentinel=True) if halo else None
    outs = [xf] + ([op] if op is not None else []) + ([hb] if hb is not None else [])

    def launch():
        xf.copy_(xres.float().to(gpu_device) if residual else torch.full((M, N), float("nan"), device=gpu_device))
        op_igemm(x_d, w_d, M, N, K, ldx=K, H=H, W=W, bias=b_d, out_bf16=op, ln_g=g_d, ln_b=e_d, ln_xf=xf, ln_halo=hb, ln_residual=residual,
                 out_fmt=out_fmt, halo_fmt=halo_fmt if halo else -1, precision=_prec(fmt))
    got = _three_runs(launch, outs)
    o, ob = FR.ln_epilogue_ref(xv, wv, bias, lg, lb, xres, fmt, residual)
    what = f"LN {fmt} out_fmt={out_fmt} halo_fmt={halo_fmt} N={N} M={M} halo={halo} residual={residual}"
    _report(what, FR.check_bound(got[0], o, ob, what))
    i = 1
    if op is not None:
        _check_copy(got[i], ofmt, (M, N), got[0], what + " operand copy")
        i += 1
    if halo:
        assert _halo_interior(got[i], hfmt, B, H, W, N), what + ": the halo border changed"
        raw = got[i]
        if hfmt == "x3":
            words = raw.view(torch.int16).reshape(B, H + 2, W + 2, 2 * N)[:, 1:-1, 1:-1].reshape(-1).view(torch.float16)
            # the x3 unit layout is over flat element indices: rows of N % 16 == 0 elements keep whole units, so the interior decodes alone
            _check_copy(words, "x3", (M, N), got[0], what + " halo copy")
        else:
            dt = {"f32": torch.float32}.get(hfmt, DT.get(hfmt))
            img = raw.view(dt).reshape(B, H + 2, W + 2, N)[:, 1:-1, 1:-1].reshape(M, N)
            _check_copy(img.reshape(-1), hfmt, (M, N), got[0], what + " halo copy")


def test_ln_epilogue_refuses_bad_descriptors(gpu_device):
    from soccdpt_amd.lib import PREC_BF16, op_igemm
    M, K = 64, 128
    x = torch.zeros(M, K, dtype=torch.bfloat16, device=gpu_device)
    wt = torch.zeros(160, K, dtype=torch.bfloat16, device=gpu_device)
    v = torch.zeros(160, device=gpu_device)
    xf = torch.full((M, 160), 7.0, device=gpu_device)
    with pytest.raises(RuntimeError, match="LayerNorm"):
        op_igemm(x, wt, M, 160, K, ldx=K, ln_g=v, ln_b=v, ln_xf=xf)                                   # N > 128
    with pytest.raises(RuntimeError, match="LayerNorm"):
        op_igemm(x, wt, M, 128, K, ldx=K, ln_g=v, ln_b=v, ln_xf=xf, ln_halo=xf)                       # ln_halo without H, W
    with pytest.raises(RuntimeError, match="LayerNorm"):
        op_igemm(x, wt, M, 128, K, ldx=K, ln_g=v, ln_b=v, ln_xf=xf, out_f32=xf)                       # no generic outputs
    with pytest.raises(RuntimeError, match="out_fmt"):
        op_igemm(x, wt, M, 128, K, ldx=K, ln_g=v, ln_b=v, ln_xf=xf, out_bf16=xf, out_fmt=3, precision=PREC_BF16)   # bf16 -> x3
    torch.cuda.synchronize()
    assert bool((xf == 7.0).all()), "a refused call launched"


# ---------------------------------------------------------------------------------------------------------------------------------
# sampled residual (FeatureFusionBlock interpolate fused into the RCU's second convolution) and cross-format stores
# ---------------------------------------------------------------------------------------------------------------------------------
RES2_CASES = [(2, 8, 8, 16, 16), (2, 16, 16, 32, 32), (1, 32, 32, 64, 64), (1, 64, 64, 128, 128), (1, 96, 96, 192, 192),
              (2, 5, 5, 16, 16),     # a non-2x ratio
              (2, 4, 1, 8, 16)]      # a source of width 1


def _conv_case(fmt, B, H, W, Cin, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64) + 0.1 * torch.arange(B, dtype=torch.float64)[:, None, None, None]
    xh = F.pad(_operand_values(x, fmt), (0, 0, 1, 1, 1, 1))
    wt = _operand_values(torch.randn(N, 9 * Cin, generator=g, dtype=torch.float64) / math.sqrt(9 * Cin), fmt)
    bias = torch.randn(N, generator=g, dtype=torch.float64).float().double()
    return g, xh, wt, bias


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32", "x3"])
@pytest.mark.parametrize("B,rh,rw,H,W", RES2_CASES)
def test_sampled_residual(gpu_device, fmt, B, rh, rw, H, W):
    from soccdpt_amd.lib import op_igemm
    Cin, N = 64, 64
    g, xh, wt, bias = _conv_case(fmt, B, H, W, Cin, N, seed=B + rh * 3 + rw * 5 + H)
    M = B * H * W
    res1 = torch.randn(M, N, generator=g, dtype=torch.float64).float().double()
    res2 = (2 * torch.randn(B, rh, rw, N, generator=g, dtype=torch.float64)).float().double()
    xh_d, w_d = _dev(xh, fmt, gpu_device), _dev(wt, fmt, gpu_device)
    b_d, r1_d, r2_d = bias.float().to(gpu_device), res1.float().to(gpu_device), res2.float().contiguous().to(gpu_device)
    out = torch.full((M, N), float("nan"), device=gpu_device)
    hb = _op_buffer(fmt, (B, H + 2, W + 2, N), gpu_device, sentinel=True)
    got, gh = _three_runs(lambda: op_igemm(xh_d, w_d, M, N, Cin, taps=9, H=H, W=W, bias=b_d, res1=r1_d, res2=r2_d, res2_h=rh, res2_w=rw, act=1,
                                           out_f32=out, out_bf16=hb, out_halo=1, precision=_prec(fmt)), [out, hb])
    ms = torch.arange(M) if M <= 8192 else torch.unique(torch.cat([torch.arange(0, M, 7), torch.arange(M - W, M)]))
    v, vb = FR.conv_res2_ref(xh, wt, bias, res1, res2, fmt, H, W, ms)
    what = f"sampled residual {fmt} B={B} {rh}x{rw} -> {H}x{W}"
    _report(what, FR.check_bound(got[ms], v, vb, what))
    assert _halo_interior(gh, fmt, B, H, W, N), what + ": the halo border changed"
    relu = got.clamp(min=0)
    if fmt == "x3":
        words = gh.view(torch.int16).reshape(B, H + 2, W + 2, 2 * N)[:, 1:-1, 1:-1].reshape(-1).view(torch.float16)
        _check_copy(words, "x3", (M, N), relu, what + " halo copy")
    else:
        dt = {"f32": torch.float32}.get(fmt, DT.get(fmt))
        img = gh.view(dt).reshape(B, H + 2, W + 2, N)[:, 1:-1, 1:-1].reshape(-1)
        _check_copy(img, fmt, (M, N), relu, what + " halo copy")


CROSS_CASES = [("f16", 3, 0, 64), ("f16", 3, 1, 64), ("x3", 1, 0, 64), ("x3", 1, 1, 64), ("x3", 1, 0, 52)]   # 52: N % 16 != 0 (fp16 rows)


@pytest.mark.parametrize("fmt,out_fmt,halo,N", CROSS_CASES)
def test_cross_format_store(gpu_device, fmt, out_fmt, halo, N):
    """An fp16 launch writing its operand copy as x3 for an x3 launch next, and an x3 launch writing fp16: plain [M][N] (a GEMM, 200 rows)
    and zero-halo (a 3x3 conv); the copy is the target format's rounding of the launch's own f32 output (relu'd)."""
    from soccdpt_amd.lib import op_igemm
    Cin = 64
    B, H, W = 2, 12, 10
    g, xh, wt, bias = _conv_case(fmt, B, H, W, Cin, N, seed=N + halo + out_fmt)
    tfmt = "x3" if out_fmt == 3 else "f16"
    if halo:
        M = B * H * W
        x_d = _dev(xh, fmt, gpu_device)
        w_d = _dev(wt, fmt, gpu_device)
        kw = dict(taps=9, H=H, W=W, out_halo=1)
        cols = torch.arange(M)
        v_ref, vb = FR.conv_res2_ref(xh, wt, bias, None, None, fmt, H, W, cols)
        buf = _op_buffer(tfmt, (B, H + 2, W + 2, N), gpu_device, sentinel=True)
    else:
        M, K = 200, 9 * Cin
        xp = _operand_values(torch.randn(M, K, generator=g, dtype=torch.float64), fmt)
        x_d = _dev(xp, fmt, gpu_device)
        w_d = _dev(wt, fmt, gpu_device)
        kw = dict(taps=1, ldx=K)
        acc = xp @ wt.t()
        v_ref = acc + bias
        vb = FR.gemm_gamma(fmt, K) * (xp.abs() @ wt.abs().t()) + FR.U * (acc.abs() + bias.abs())
        buf = _op_buffer(tfmt, (M, N), gpu_device)
    out = torch.full((M, N), float("nan"), device=gpu_device)
    b_d = bias.float().to(gpu_device)
    got, gb = _three_runs(lambda: op_igemm(x_d, w_d, M, N, Cin if halo else 9 * Cin, bias=b_d, act=1, act_on_f32=1, out_f32=out, out_bf16=buf,
                                           out_fmt=out_fmt, precision=_prec(fmt), **kw), [out, buf])
    what = f"cross-format {fmt} -> {tfmt} N={N} halo={halo}"
    _report(what, FR.check_bound(got, v_ref.clamp(min=0), vb, what))
    if halo:
        assert _halo_interior(gb, tfmt, B, H, W, N), what + ": the halo border changed"
        if tfmt == "x3":
            words = gb.view(torch.int16).reshape(B, H + 2, W + 2, 2 * N)[:, 1:-1, 1:-1].reshape(-1).view(torch.float16)
            _check_copy(words, "x3", (M, N), got, what + " copy")
        else:
            img = gb.view(torch.float16).reshape(B, H + 2, W + 2, N)[:, 1:-1, 1:-1].reshape(-1)
            _check_copy(img, "f16", (M, N), got, what + " copy")
    else:
        _check_copy(gb, tfmt, (M, N), got, what + " copy")
