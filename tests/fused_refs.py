"""Float64 references of the fused epilogues and tails that only the 16-bit modes run, each with an a-priori per-element error bound.

Every reference starts from the exact operand values the kernel reads (16-bit, x3 / x2w pairs decoded, or f32) and returns
(expected output, bound): |kernel - expected| <= bound must hold element by element.  The bounds are derived from the operands and a stated
model of the kernel's f32 arithmetic, never fitted to measured errors:

* f32 unit roundoff u = 2^-24; a chain of n roundings is bounded by gamma(n) = n u / (1 - n u) times the sum of the magnitudes involved.
* 16-bit MFMA (v_mfma_f32_*_{bf16,f16}): one k-step adds 32 exact products to the f32 accumulator.  Model: at most MFMA_ROUNDINGS = 6
  roundings per k-step (a pairwise f32 sum of the 32 products, 5 levels, plus the accumulator add), so a K-long dot product is within
  gamma(6 ceil(K / 32)) sum |w x|.  x2w (fp16 x times an x3 weight pair) runs two such chains, x3 three (hi hi, and the cross terms
  scaled by 2^-11) and drops lo lo (<= 2^-24 |w x| per product, half16.h).  The f32 MFMA (16x16x4) rounds once per product: gamma(K).
* Bilinear sampling (align_corners=True) is computed with the exact source position p = i (n_in - 1) / (n_out - 1).  The kernels form p in
  f32 (scale = f32 division, f32 product, possibly contracted): _f32_position_error bounds |p_kernel - p| over those variants, and the
  sampled value moves by at most that times the neighbouring differences of the source (the two segments around p, so a position that
  crosses an integer is covered).  The f32 lerp itself (<= 4 roundings, weights 1 - l rounded) is allowed LERP_SLACK = 2^-20 of sum |w a|.
* A value the kernel rounds to 16 bits (the depth tail's up-sampled patch) may land on either neighbour when the float64 value lies within
  the sampling allowance of a rounding midpoint: those elements get one 16-bit ulp, propagated through |W|; all others are exact.
* ReLU is 1-Lipschitz (no special case for a flipped mask); a linear tail propagates the bound through |w|.
* LayerNorm: the bound on v = acc + bias is propagated by |g| / sigma_row (first-order sensitivity of the normalisation), plus the f32
  arithmetic of the statistics, rsqrtf and the affine tail.
* Activations: sigmoid / 0.5 tanh + 0.5 are monotone, so the bound on their argument maps to an interval; expf / tanhf add a few f32 ulps.

Operand copies are checked against the kernel's own f32 output: a 16-bit copy must be its round-to-nearest-even value exactly, an x3 copy
must carry hi = RN16(v) and decode to v within 2^-23 |v| + 2^-36 (half16.h: the pair holds 22+ significand bits).
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MFMA_ROUNDINGS = 6
LERP_SLACK = 2.0 ** -20


def gamma(n: float) -> float:
    return n * U / (1.0 - n * U)


def gemm_gamma(fmt: str, K: int, mf: int = 16) -> float:
    """Relative bound (times sum |w x|) of a K-long dot product of the igemm / depth-tail kernels in operand format fmt.
    mf = 32: the v_mfma_f32_32x32x16 forms of the 16-bit tiles add 16 exact products per k-step -- by the same rule a pairwise sum of 4 levels plus the
    accumulator add, 5 roundings per ceil(K / 16) steps."""
    steps = -(-K // 32)
    if fmt in ("bf16", "f16") and mf == 32:
        return gamma((MFMA_ROUNDINGS - 1) * -(-K // 16))
    if mf != 16:
        raise ValueError((fmt, mf))
    if fmt in ("bf16", "f16"):
        return gamma(MFMA_ROUNDINGS * steps)
    if fmt == "x2w":
        return gamma(MFMA_ROUNDINGS * 2 * steps + 2)
    if fmt == "x3":
        return gamma(MFMA_ROUNDINGS * 3 * steps + 2) + 2.0 ** -24
    if fmt == "f32":
        return gamma(K + 2)
    raise ValueError(fmt)


DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}


def round16(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 -> the nearest bf16 / fp16 value (round to nearest even, through f32), as float64."""
    return x.to(torch.float32).to(DT16[fmt]).to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# bilinear sampling, align_corners=True
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_position_error(n_in: int, n_out: int) -> torch.Tensor:
    """max over the kernels' f32 ways of forming the source position (scale = (n_in-1)/(n_out-1) in f32, or one ulp either side; position =
    f32(scale * i), or i0 + f32(scale * i - i0) when the subtraction is contracted) of |p_f32 - p_exact|, per output index i."""
    i = np.arange(n_out, dtype=np.float64)
    exact = i * (n_in - 1) / (n_out - 1) if n_out > 1 else np.zeros_like(i)
    if n_out <= 1:
        return torch.zeros(n_out, dtype=torch.float64)
    s = np.float32(n_in - 1) / np.float32(n_out - 1)
    dp = np.zeros_like(i)
    for sc in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(np.inf))):
        prod = np.float64(sc) * i                     # exact: 24 x 17 significant bits
        f = prod.astype(np.float32).astype(np.float64)
        i0 = np.floor(f)
        fused = i0 + (prod - i0).astype(np.float32).astype(np.float64)
        dp = np.maximum(dp, np.maximum(np.abs(f - exact), np.abs(fused - exact)))
    return torch.from_numpy(dp)


def _f32_halfpixel_error(n_in: int, n_out: int) -> torch.Tensor:
    """The same for the half-pixel form p = max((i + 0.5) n_in / n_out - 0.5, 0) (hybrid.hip pos_embed_resize_kernel): scale = n_in / n_out in f32 or
    one ulp either side, i + 0.5 exact, then the product rounded and 0.5 subtracted (rounded again), or both in one fma."""
    i = np.arange(n_out, dtype=np.float64)
    exact = np.maximum((i + 0.5) * n_in / n_out - 0.5, 0.0)
    s = np.float32(n_in) / np.float32(n_out)
    dp = np.zeros_like(i)
    for sc in (s, np.nextafter(s, np.float32(0)), np.nextafter(s, np.float32(np.inf))):
        prod = np.float64(sc) * (i + 0.5)             # exact: 24 x 18 significant bits
        two = (prod.astype(np.float32).astype(np.float64) - 0.5).astype(np.float32).astype(np.float64)
        fused = (prod - 0.5).astype(np.float32).astype(np.float64)
        for f in (two, fused):
            dp = np.maximum(dp, np.abs(np.maximum(f, 0.0) - exact))
    return torch.from_numpy(dp)


def _axis(n_in: int, n_out: int, align_corners: bool = True):
    """Per output index: i0, i1 (clamped), im = i0 - 1 (clamped), weight l of i1, and the position allowance dp."""
    i = torch.arange(n_out, dtype=torch.float64)
    if align_corners:
        p = i * ((n_in - 1) / (n_out - 1)) if n_out > 1 else torch.zeros_like(i)
        dp = _f32_position_error(n_in, n_out)
    else:   # torch's half-pixel form (the position-embedding resize; the align_corners kernels' self-tests build faults with it)
        p = ((i + 0.5) * (n_in / n_out) - 0.5).clamp(min=0)
        dp = _f32_halfpixel_error(n_in, n_out)
    i0 = p.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), (i0 - 1).clamp(min=0), p - i0, dp


def bilinear_sample(src: torch.Tensor, b: torch.Tensor, Y: torch.Tensor, X: torch.Tensor, H: int, W: int, align_corners: bool = True):
    """src [B][h][w][C] (float64, or float32 holding exact operand values) sampled at output pixels (b, Y, X) of an H x W map (index tensors of one shape S).
    Returns (v [S][C] float64, allowance [S][C]) with |kernel's f32 bilinear value - v| <= allowance."""
    _, h, w, _ = src.shape
    y0, y1, ym, ly, dpy = (t[Y] for t in _axis(h, H, align_corners))
    x0, x1, xm, lx, dpx = (t[X] for t in _axis(w, W, align_corners))
    ly, lx, dpy, dpx = ly[..., None], lx[..., None], dpy[..., None], dpx[..., None]
    a00, a01, a10, a11 = (src[b, yy, xx].double() for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    am0, am1, a0m, a1m = (src[b, yy, xx].double() for yy, xx in ((ym, x0), (ym, x1), (y0, xm), (y1, xm)))
    hy, hx = 1 - ly, 1 - lx
    v = hy * (hx * a00 + lx * a01) + ly * (hx * a10 + lx * a11)
    S = hy * (hx * a00.abs() + lx * a01.abs()) + ly * (hx * a10.abs() + lx * a11.abs())
    vert = (a10 - a00).abs() + (a11 - a01).abs() + (a00 - am0).abs() + (a01 - am1).abs()
    horiz = (a01 - a00).abs() + (a11 - a10).abs() + (a00 - a0m).abs() + (a10 - a1m).abs()
    return v, dpy * vert + dpx * horiz + LERP_SLACK * S


# ---------------------------------------------------------------------------------------------------------------------------------
# fused depth tail (csrc/depth_tail.hip): up2 (align_corners) -> 16-bit patch -> conv3x3 128->32 + bias -> ReLU -> 1x1 32->1 + b4 -> ReLU
# ---------------------------------------------------------------------------------------------------------------------------------
def depth_tail_tiles(B: int, h: int, w: int):
    """(number of 8 x 16 output tiles, tiles per row, tiles per column) of the depth tail at B x (2h x 2w)."""
    tx, ty = (2 * w) // 16, (2 * h) // 8
    return B * tx * ty, tx, ty


def depth_tail_ref(d1, wt, bias, w4, b4, fmt, tiles=None, align_corners=True, chunk=48):
    """d1 [B][h][w][128] (the 16-bit values, float32 or float64), wt [32][9*128] (tap-major, tap = 3 ky + kx), bias / w4 [32], b4: float.
    tiles: 1-D LongTensor of output tile ids (id = (b * tiles_y + ty) * tiles_x + tx), default all.
    Returns (ref [T][8][16], bound [T][8][16]), tile t covering out[b, 8 ty : 8 ty + 8, 16 tx : 16 tx + 16].

    Accumulation model: the conv is 9 taps x 4 k-steps = 36 MFMA k-steps per output channel (gemm_gamma('bf16'/'f16', 1152)) over the
    kernel's patch, which differs from round16(v) only where v is within the sampling allowance of a 16-bit midpoint (one ulp there);
    bias add: one rounding; 1x1 + b4: <= 12 roundings along any path (4-term fma chains, two shuffles, the cross-wave add, + b4)."""
    B, h, w, C = d1.shape
    assert C == 128
    H, W = 2 * h, 2 * w
    n, tx_n, ty_n = depth_tail_tiles(B, h, w)
    if tiles is None:
        tiles = torch.arange(n)
    Wk = wt.reshape(32, 9, 128)
    g_acc = gemm_gamma(fmt, 9 * 128)
    refs, bnds = [], []
    for ch in tiles.split(chunk):
        T = ch.numel()
        tx, ty, b = ch % tx_n, (ch // tx_n) % ty_n, ch // (tx_n * ty_n)
        Y = ty[:, None] * 8 - 1 + torch.arange(10)
        X = tx[:, None] * 16 - 1 + torch.arange(18)
        valid = (((Y >= 0) & (Y < H))[:, :, None] & ((X >= 0) & (X < W))[:, None, :])[..., None].double()
        bb = b[:, None, None].expand(T, 10, 18)
        YY = Y.clamp(0, H - 1)[:, :, None].expand(T, 10, 18)
        XX = X.clamp(0, W - 1)[:, None, :].expand(T, 10, 18)
        v, e = bilinear_sample(d1, bb, YY, XX, H, W, align_corners)
        P = round16(v, fmt)
        allow = torch.maximum(round16(v + e, fmt) - P, P - round16(v - e, fmt))
        P, allow = P * valid, allow * valid
        acc = torch.zeros(T, 8, 16, 32, dtype=torch.float64)
        mag = torch.zeros_like(acc)
        amb = torch.zeros_like(acc)
        for ky in range(3):
            for kx in range(3):
                wk = Wk[:, ky * 3 + kx, :]
                p = P[:, ky:ky + 8, kx:kx + 16]
                acc += p @ wk.t()
                mag += p.abs() @ wk.abs().t()
                amb += allow[:, ky:ky + 8, kx:kx + 16] @ wk.abs().t()
        e_acc = g_acc * (mag + amb) + amb
        pre = acc + bias
        e_pre = e_acc + U * (acc.abs() + bias.abs())
        r = pre.clamp(min=0)
        o = (r * w4).sum(-1) + b4
        e_o = (e_pre * w4.abs()).sum(-1) + gamma(12) * (((r + e_pre) * w4.abs()).sum(-1) + abs(b4))
        refs.append(o.clamp(min=0))
        bnds.append(e_o)
    return torch.cat(refs), torch.cat(bnds)


def gather_tiles(out, tiles, tx_n, ty_n):
    """out [B][H][W] -> [T][8][16] of the given depth-tail tile ids."""
    tx, ty, b = tiles % tx_n, (tiles // tx_n) % ty_n, tiles // (tx_n * ty_n)
    Y = (ty[:, None] * 8 + torch.arange(8))[:, :, None]
    X = (tx[:, None] * 16 + torch.arange(16))[:, None, :]
    return out[b[:, None, None], Y, X]


def pick_tiles(B, tiles_x, tiles_y, n_random=48, seed=0, wg=256):
    """The output tiles a large-shape test compares: every border tile of every image, the first and last tile of every batch row, the
    tiles at workgroup-count boundaries (ids 255, 256, 511, 512, ...) and a seeded random set of interior tiles.  Sorted, unique."""
    per = tiles_x * tiles_y
    sel = []
    for b in range(B):
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                if ty in (0, tiles_y - 1) or tx in (0, tiles_x - 1):
                    sel.append(b * per + ty * tiles_x + tx)
        sel += [b * per, b * per + per - 1]
    n = B * per
    k = wg
    while k - 1 < n:
        sel += [k - 1] + ([k] if k < n else [])
        k += wg
    g = torch.Generator().manual_seed(seed)
    sel += torch.randint(0, n, (n_random,), generator=g).tolist()
    return torch.tensor(sorted(set(sel)), dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------------------------
# seg head: conv3x3 + bias + ReLU with the three-class classifier in the epilogue (igemm dot3), the finishing sum, up2 + activation
# ---------------------------------------------------------------------------------------------------------------------------------
def im2col3x3(xh, ms, H, W):
    """Rows [len(ms)][9 * Cin] (tap-major) of output pixels ms of a zero-halo NHWC image xh [B][H+2][W+2][Cin]."""
    b, rem = ms // (H * W), ms % (H * W)
    y, x = rem // W, rem % W
    return torch.cat([xh[b, y + ky, x + kx] for ky in range(3) for kx in range(3)], dim=1)


def dot3_ref(xh, wt, bias, dot_w, fmt, bn, ms, H, W):
    """Partial logits of a dot3 launch at pixels ms: [N / bn][len(ms)][3] and their bound.  xh [B][H+2][W+2][Cin], wt [N][9 Cin],
    bias [N], dot_w [3][N], all float64 operand values.  v = relu(acc + bias) per channel; plane t = sum over channels [t bn, (t+1) bn) of
    v dot_w; the classifier sum is bounded by gamma(bn + 8) (every lane's 4-channel fma chains, two shuffles, the cross-wave adds)."""
    cols = im2col3x3(xh, ms, H, W)
    N = wt.shape[0]
    acc = cols @ wt.t()
    e_acc = gemm_gamma(fmt, wt.shape[1]) * (cols.abs() @ wt.abs().t())
    a = (acc + bias).clamp(min=0)
    e_a = e_acc + U * (acc.abs() + bias.abs())
    refs, bnds = [], []
    for t in range(N // bn):
        sl = slice(t * bn, (t + 1) * bn)
        dw = dot_w[:, sl].t()
        refs.append(a[:, sl] @ dw)
        bnds.append(e_a[:, sl] @ dw.abs() + gamma(bn + 8) * ((a[:, sl] + e_a[:, sl]) @ dw.abs()))
    return torch.stack(refs), torch.stack(bnds)


def seg_logits_ref(part, bias):
    """The finishing sum (seg_logits_finish_kernel) from the kernel's own partial planes part [T][M][4] (lane 3 is padding and is not
    read): logits [M][3] = bias + sum over t in tile order, bound gamma(T + 1) times the magnitudes."""
    p = part[..., :3].double()
    return p.sum(0) + bias, gamma(p.shape[0] + 1) * (p.abs().sum(0) + bias.abs())


def seg_activation(v, sigmoid):
    """oracle/soccdpt_ref.py seg_head: torch.sigmoid, or ScaledTanh 0.5 tanh + 0.5 (model/scaled_tanh.py)."""
    return torch.sigmoid(v) if sigmoid else 0.5 * torch.tanh(v) + 0.5


def seg_up_act_ref(logits, B, h, w, sigmoid):
    """logits [B*h*w][3] float64 (the values the kernel reads) -> seg_head's interpolation (x2, bilinear, align_corners) and activation in
    float64: [B][3][2h][2w] and bound.  The activation is monotone: the interval v +- e maps to [act(v - e), act(v + e)]; expf / tanhf and
    the f32 tail add 8 ulps (relative for the sigmoid, whose relative error is that of expf; of 1 for 0.5 tanh + 0.5)."""
    src = logits.reshape(B, h, w, 3)
    H, W = 2 * h, 2 * w
    b = torch.arange(B)[:, None, None].expand(B, H, W)
    Y = torch.arange(H)[None, :, None].expand(B, H, W)
    X = torch.arange(W)[None, None, :].expand(B, H, W)
    v, e = bilinear_sample(src, b, Y, X, H, W)
    a = seg_activation(v, sigmoid)
    spread = torch.maximum(seg_activation(v + e, sigmoid) - a, a - seg_activation(v - e, sigmoid))
    ulps = 8 * U * (a if sigmoid else (1 + a))
    return a.permute(0, 3, 1, 2), (spread + ulps).permute(0, 3, 1, 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# igemm: generic epilogue with the sampled residual, and the Swin-V2 post-norm LayerNorm epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_res2_ref(xh, wt, bias, res1, res2, fmt, H, W, ms):
    """v = conv3x3(x) + bias (+ res1) (+ bilinear(res2)) at pixels ms ([len(ms)][N]) and its bound.  res1 [M][N], res2 [B][rh][rw][N]
    (f32 values), either may be None; the epilogue adds them in that order (<= 3 roundings)."""
    cols = im2col3x3(xh, ms, H, W)
    acc = cols @ wt.t()
    e = gemm_gamma(fmt, wt.shape[1]) * (cols.abs() @ wt.abs().t())
    v = acc + bias
    mag = acc.abs() + bias.abs()
    if res1 is not None:
        v = v + res1[ms]
        mag = mag + res1[ms].abs()
    if res2 is not None:
        b, rem = ms // (H * W), ms % (H * W)
        up, e_up = bilinear_sample(res2, b, rem // W, rem % W, H, W)
        v = v + up
        mag = mag + up.abs()
        e = e + e_up
    return v, e + gamma(3) * mag


def ln_epilogue_ref(x, wt, bias, g, b, xres, fmt, residual):
    """o = (residual ? xres : 0) + LayerNorm(x @ wt^T + bias) * g + b (eps 1e-5, biased variance) and its bound; x [M][K], wt [N][K]."""
    N = wt.shape[0]
    acc = x @ wt.t()
    e_v = gemm_gamma(fmt, x.shape[1]) * (x.abs() @ wt.abs().t()) + U * (acc.abs() + bias.abs())
    v = acc + bias
    mean = v.mean(1, keepdim=True)
    sigma = ((v - mean) ** 2).mean(1, keepdim=True).add(1e-5).sqrt()
    yh = (v - mean) / sigma
    o = yh * g + b + (xres if residual else 0)
    emax = e_v.max(1, keepdim=True).values
    prop = g.abs() / sigma * (e_v + emax * (1 + yh.abs()))
    arith = g.abs() * ((yh.abs() + 1) * gamma(2 * N + 8) + gamma(N + 2) * v.abs().max(1, keepdim=True).values / sigma)
    tail = gamma(4) * ((yh * g).abs() + b.abs() + (xres.abs() if residual else 0))
    return o, prop + arith + tail


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------
def check_bound(got, ref, bound, what):
    """Assert |got - ref| <= bound element-wise (NaN fails); return the worst error as a fraction of its bound."""
    got = got.double().cpu()
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = float((err / bound.clamp(min=1e-300)).nan_to_num(float("inf")).max()) if err.numel() else 0.0
    if bad.any():
        idx = bad.nonzero()[0].tolist()
        t = tuple(idx)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements exceed the bound; first at {t}: got {float(got[t])!r}, "
                             f"expected {float(ref[t])!r}, bound {float(bound[t]):.3e} (worst error / bound {ratio:.3g})")
    return ratio


def check_copy16(got, f32_vals, fmt, what):
    """A 16-bit operand copy must be the round-to-nearest-even value of the kernel's own f32 output (fp16 saturates at 65504)."""
    v = f32_vals.float().cpu()
    if fmt == "f16":
        v = v.clamp(-65504.0, 65504.0)
    exp = v.to(torch.bfloat16 if fmt == "bf16" else torch.float16)
    g = got.cpu()
    same = (g.view(torch.int16) == exp.view(torch.int16)) | ((g == 0) & (exp == 0))
    if not bool(same.all()):
        t = tuple((~same).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.numel()} operand words differ from RN16 of the f32 value; first at {t}: "
                             f"got {float(g[t])!r}, f32 {float(f32_vals[t])!r}")


def x3_parts(raw, shape):
    """Flat fp16 x3 storage -> (hi, lo) float64 tensors of `shape` (half16.h layout: hi chunk first in even 8-element units)."""
    r = raw.cpu().view(torch.float16).reshape(-1, 2, 8).double()
    odd = (torch.arange(r.shape[0]) & 1).bool()[:, None]
    hi = torch.where(odd, r[:, 1], r[:, 0])
    lo = torch.where(odd, r[:, 0], r[:, 1])
    return hi.reshape(shape), lo.reshape(shape)


def check_x3(raw, shape, f32_vals, what):
    """An x3 operand copy: hi = RN16(v) exactly and hi + lo / 2048 within 2^-23 |v| + 2^-36 of the kernel's f32 value v."""
    return check_x3_parts(*x3_parts(raw, shape), f32_vals, what)


def check_x3_parts(hi, lo, f32_vals, what):
    """The same on decoded (hi, lo) values -- for a part of an x3 tensor, such as the interior of a zero-halo image."""
    v = f32_vals.double().cpu()
    exp_hi = v.float().to(torch.float16).double()
    bad_hi = ~(hi == exp_hi)
    if bad_hi.any():
        t = tuple(bad_hi.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad_hi.sum())} x3 hi words differ from RN16(v); first at {t}: hi {float(hi[t])!r}, v {float(v[t])!r}")
    return check_bound(hi + lo / 2048.0, v, 2.0 ** -23 * v.abs() + 2.0 ** -36, what + " (x3 decode)")


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by the GPU tests and the CPU self-test (float64 tensors holding exact operand values)
# ---------------------------------------------------------------------------------------------------------------------------------
def depth_tail_inputs(B, h, w, fmt, seed=0):
    """d1 with a distinct offset per batch row, exact zeros (one source row, one channel block), a large-magnitude block (|d1| up to ~1e3),
    weights ~ 1 / sqrt(1152), a bias that switches channels 0-7 off (and 8-15 partly), a 1x1 with mixed signs (positive on average) and b4 > 0."""
    g = torch.Generator().manual_seed(seed)
    d1 = torch.randn(B, h, w, 128, generator=g)
    d1 += 0.5 * torch.arange(1, B + 1, dtype=torch.float32)[:, None, None, None]
    d1[:, h // 2] = 0.0                       # a whole source row of exact zeros
    d1[..., 16:32] = 0.0                      # and a channel block
    d1[:, : max(1, h // 4), : max(1, w // 4), 32:48] *= 300.0
    wt = torch.randn(32, 9 * 128, generator=g, dtype=torch.float64) / math.sqrt(9 * 128)
    bias = torch.randn(32, generator=g, dtype=torch.float64).float().double()
    bias[:8] = -40.0
    bias[8:16] -= 1.0
    w4 = (0.15 + torch.randn(32, generator=g, dtype=torch.float64) / 4).float().double()
    d1 = d1.to(DT16[fmt]).float()             # float32 holding the exact 16-bit values (the model shapes are large)
    return d1, round16(wt, fmt), bias, w4, 1.5


def seg_inputs(B, H, W, fmt, Cin=256, N=256, seed=0):
    """Halo image [B][H+2][W+2][Cin] (distinct per batch row), conv weights [N][9 Cin], bias (BN shift, a third negative), classifier
    dot_w [3][N] with three different rows and bias [3]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=torch.float64) + 0.3 * torch.arange(B, dtype=torch.float64)[:, None, None, None]
    xh = F.pad(round16(x, fmt), (0, 0, 1, 1, 1, 1))
    wt = round16(torch.randn(N, 9 * Cin, generator=g, dtype=torch.float64) / math.sqrt(9 * Cin), fmt)
    bias = torch.randn(N, generator=g, dtype=torch.float64).float().double() - 0.3
    dot_w = (torch.randn(3, N, generator=g, dtype=torch.float64) / math.sqrt(N)).float().double()
    dot_w[1] += 0.05
    dot_w[2] -= 0.05
    sbias = torch.tensor([0.1, -0.2, 0.3], dtype=torch.float64)
    return xh, wt, bias, dot_w, sbias
