"""Float64 references of the forward attention kernels (csrc/attention.hip, attention_body.h, attention_qkv.hip, vit_attention.hip), each with an a-priori
per-element error bound, and the inputs the GPU tests and the CPU self-test share.

Conventions of tests/fused_refs.py: every reference starts from the exact 16-bit / f32 operand values the kernel reads and returns (expected, bound); |kernel -
expected| <= bound must hold for every element (an f32 output: check_bound; a 16-bit output: check_interval16; an x3 output: check_x3_interval).  Nothing is fitted
to a measured error.

The bound, per query row (softmax weights p_j, logits s_j, row maximum m, output o_d = sum_j p_j v_jd):

* Logits.  If every logit of the row is off by at most eps, the weights move by a factor within e^(+-2 eps), and since the perturbed weights still sum to one
      |o' - o| <= (e^(2 eps) - 1) D_d,     D_d = sum_j p_j |v_jd - o_d|
  (the mean absolute deviation itself, one output channel at a time: _mean_abs_dev).  eps is the maximum over the keys of the row of
      sum_i (Eq_i |k^_i| + |q^_i| Ek_i + Eq_i Ek_i)  +  gamma(34) (sum_i |q^_i k^_i| + |bias| + 100 [masked])  +  the exponent terms below,
  where q^ = scale q / max(|q|, 1e-12), k^ = k / max(|k|, 1e-12) and Eq, Ek bound the element errors of the operands the matrix cores read:
      Eq_i = |q^_i| (NORM + u16 (1 + NORM)) + a       NORM = gamma(24): 32 squares summed in f32 (half of gamma(33) after the root), sqrtf, the division, the product
      u16  = 2^-8 (bf16), 2^-11 (fp16), 0 (f32 kernels);  a = 2^-25 (fp16: a q^ / k^ element below 2^-14 lands on the subnormal grid), else 0.
  The products of 16-bit operands are exact, the accumulator starts from the bias (+ -100), and 32 products are added in f32: gamma(34) covers the two
  32x32x16 MFMA steps as well as the f32 kernels' 32 fmas + table add + mask add.
* Exponent.  Every kernel forms p~ = exp2(fma(s, log2e, -fl(mn log2e))) (or expf(s - mn)) against a running maximum mn and rescales earlier tiles by
  alpha = exp2(fma(m_old, log2e, -fl(mn log2e))).  The rounding of fl(mn log2e) is common to alpha and every p~ of the tile, so it cancels in o / l; what is left per
  factor is the fma's own rounding and the constant's, 2 u |argument|, plus EXP_ULPS = 4 ulps of v_exp_f32 / expf and one for the product.  Along the rescales the
  arguments telescope to m - s_j, so a weight carries at most 2 u (m - s_j) + u (EXP_ULPS + 5 R), R = the number of rescales the kernel can perform (key tiles + 2;
  the one-thread-per-query kernel rescales per key).  Relative perturbations of p: part of eps.
* 16-bit weights.  The 16-bit kernels round p~ to 16 bits for the P V product and take the row sum from the unrounded values, so the rounded weights no longer sum
  to one: that error is u16 sum_j p_j |v_jd| (NOT a multiple of D: with all v equal D is zero and the output still moves), plus for fp16 the subnormal grid
  2^-25 sum_j |v_jd| / rowsum, rowsum = sum_j e^(s_j - m) >= 1.
* f32 tail.  P V accumulation and the rescales, gamma(n_acc) sum_j p_j |v_jd| with n_acc = N + NT + 4 (2 N + 4 for the per-key kernel); the row sum l the same
  relative to |o|; reciprocal and final product gamma(3) |o|.  All multiplied by e^(2 eps) (the kernel's weights, not the exact ones).
* Fused qkv.  q, k, v come from f32 accumulators: |e| <= gamma(C + 2) (sum |x w| + |bias|) each.  For q and k the error passes through the normalisation,
  |d q^_i| <= scale (e_i + |q~_i| sum_k |q~_k| e_k) / (|q| - |e|)  (q~ the unit vector), and joins Eq / Ek; v is rounded once to 16 bits, Ev = e + u16 (|v| + e) + a,
  and the output moves by at most e^(2 eps) sum_j p_j Ev_jd.
* ViT attention: s = sum_i (q_i / 8) k_i, the scaling exact (fp16: an element of q / 8 below 2^-14 is rounded to the subnormal grid, a = 2^-25 per element);
  eps = gamma(66) sum_i |q_i k_i| / 8 + a sum_i |k_i| + the exponent terms; the two key halves of the 16-bit kernel meet with one more rescale.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from tests.fused_refs import U, check_bound, check_x3, gamma, round16  # noqa: F401  (re-exported for the tests)
from tests.fwd_aux_refs import check_interval16, check_x3_interval  # noqa: F401

U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 0.0}      # unit roundoff of round-to-nearest: 8 and 11 significant bits
SUBNORMAL = {"bf16": 0.0, "f16": 2.0 ** -25, "f32": 0.0}
NORM = gamma(24)
EXP_ULPS = 4
HEAD_SCALES = (1.0, 11.75, 100.0)      # cycled over the heads; 100 = exp(ln 100), the reference's clamp


def quantize(x: torch.Tensor, fmt: str) -> torch.Tensor:
    """float64 -> the nearest value of the operand format, as float64."""
    return x.float().double() if fmt == "f32" else round16(x, fmt)


# ---------------------------------------------------------------------------------------------------------------------------------
# window geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def window_rows(B, res, ws, shift, roll_sign=1, swap_windows=False):
    """[B * nw * nw][N] row indices into the [B * res * res] token list: window (b, wy, wx), token (r, c) reads row (wy ws + r + shift) mod res, column
    (wx ws + c + shift) mod res -- torch.roll by -shift, then the window partition.  The output goes back to the same rows (reverse, roll by +shift).
    roll_sign = -1 / swap_windows: the defects 'roll in the wrong direction' / 'window reverse with wx and wy swapped'."""
    nw = res // ws
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    wy = torch.arange(nw).view(1, nw, 1, 1, 1)
    wx = torch.arange(nw).view(1, 1, nw, 1, 1)
    if swap_windows:
        wy, wx = wx, wy
    r = torch.arange(ws).view(1, 1, 1, ws, 1)
    c = torch.arange(ws).view(1, 1, 1, 1, ws)
    sy = (wy * ws + r + roll_sign * shift) % res
    sx = (wx * ws + c + roll_sign * shift) % res
    return ((b * res + sy) * res + sx).reshape(B * nw * nw, ws * ws)


def window_masked(res, ws, shift, first=False):
    """[nw * nw][N][N] bool: the pairs that get -100.  In the rolled image the rows / columns >= res - shift came from the other side: within the last window row
    (column) a pair is masked when exactly one of its tokens lies there.  first: the defect 'mask on the first window row / column'."""
    if shift == 0:
        return None
    nw, N = res // ws, ws * ws
    r = torch.arange(N) // ws
    c = torch.arange(N) % ws
    rhi, chi = r >= ws - shift, c >= ws - shift
    rowdiff = rhi[:, None] != rhi[None, :]
    coldiff = chi[:, None] != chi[None, :]
    edge = 0 if first else nw - 1
    m = torch.zeros(nw, nw, N, N, dtype=torch.bool)
    m[edge, :] |= rowdiff
    m[:, edge] |= coldiff
    return m.reshape(nw * nw, N, N)


def bias_index(ws, transposed=False):
    """[N][N] index of (query, key) into the (2 ws - 1)^2 table: (rq - rk + ws - 1) (2 ws - 1) + (cq - ck + ws - 1).  transposed: the defect rk - rq."""
    N = ws * ws
    r = torch.arange(N) // ws
    c = torch.arange(N) % ws
    dr, dc = r[:, None] - r[None, :], c[:, None] - c[None, :]
    if transposed:
        dr, dc = -dr, -dc
    return (dr + ws - 1) * (2 * ws - 1) + (dc + ws - 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the softmax core: one chunk of (window, head) pairs
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Model:
    """What the bound needs to know about the kernel: operand format, the number of rescales a weight can go through, the length of the P V accumulation."""
    fmt: str
    rescales: int
    n_acc: int


def window_model(fmt, ws, per_key=False):
    N = ws * ws
    NT = (N + 31) // 32
    return Model(fmt, N if per_key else NT + 2, 2 * N + 4 if per_key else N + NT + 4)


def vit_model(fmt, N):
    NT = (N + 31) // 32
    return Model(fmt, NT + 3, N + NT + 8)


def _mean_abs_dev(p, v, o):
    """sum_j p_j |v_jd - o_d| for p [P][N][K], v [P][K][d], o [P][N][d], one output channel at a time through one [P][N][K] buffer.  Evaluated in f32 (the term
    is a factor of the bound, not a reference value): the caller allows 2^-12 relative for the K-long f32 sum of non-negative terms and 2^-22 (sum p |v| + |o|)
    for the f32 images of v and o."""
    p32, v32, o32 = p.float(), v.float(), o.float()
    buf = torch.empty_like(p32)
    D = torch.empty(o.shape, dtype=torch.float64)
    for c in range(v.shape[-1]):
        torch.sub(v32[:, None, :, c], o32[:, :, None, c], out=buf)
        buf.abs_().mul_(p32)
        D[..., c] = buf.sum(-1)
    return D


def _softmax_bound(s, eps_pair, v, model, Ev=None, defect=None):
    """s, eps_pair [P][N][K] (logits and their error, without the exponent terms), v [P][K][d] -> (o, bound) [P][N][d]."""
    m = s.amax(-1, keepdim=True)
    gap = m - s
    e = torch.exp(-gap)
    rowsum = e.sum(-1, keepdim=True)
    p = e / rowsum
    eps = (eps_pair + 2 * U * gap.clamp(max=1e4)).amax(-1, keepdim=True) + U * (EXP_ULPS + 5 * model.rescales)      # padded / -inf keys never reach here
    if defect is not None:
        return defect(s, p, v), None
    o = p @ v
    A = p @ v.abs()
    D = _mean_abs_dev(p, v, o) * (1 + 2.0 ** -12) + 2.0 ** -22 * (A + o.abs())
    grow = torch.exp(2 * eps)
    u16 = U16[model.fmt]
    bound = (grow - 1) * D + grow * ((u16 + gamma(model.n_acc)) * A + (gamma(model.n_acc) + gamma(3)) * o.abs())
    if SUBNORMAL[model.fmt]:
        bound = bound + SUBNORMAL[model.fmt] * v.abs().sum(-2, keepdim=True) / rowsum
    if Ev is not None:
        bound = bound + grow * (p @ Ev)
    return o, bound


def _cosine_logits(q, k, scale, bias, masked, fmt, Eq_extra=None, Ek_extra=None):
    """q, k [P][N][32], scale [P][1][1], bias [P][N][N], masked [P][N][N] bool or None -> (s, eps_pair)."""
    qn = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12) * scale
    kn = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    rel = NORM + U16[fmt] * (1 + NORM)
    Eq = qn.abs() * rel + SUBNORMAL[fmt]
    Ek = kn.abs() * rel + SUBNORMAL[fmt]
    if Eq_extra is not None:
        Eq = Eq + Eq_extra * (1 + U16[fmt])
        Ek = Ek + Ek_extra * (1 + U16[fmt])
    s = qn @ kn.transpose(-1, -2) + bias
    mag = qn.abs() @ kn.abs().transpose(-1, -2) + bias.abs()
    eps = Eq @ kn.abs().transpose(-1, -2) + qn.abs() @ Ek.transpose(-1, -2) + Eq @ Ek.transpose(-1, -2)
    if masked is not None:
        s = s - 100.0 * masked
        mag = mag + 100.0 * masked
    return s, eps + gamma(34) * mag


# ---------------------------------------------------------------------------------------------------------------------------------
# defects (tests/test_attention_refs.py: each must leave the bound)
# ---------------------------------------------------------------------------------------------------------------------------------
DEFECTS = ("bias_transposed", "roll_reversed", "mask_first", "drop_last_key", "pad_bias_zero", "next_head_scale", "reverse_swapped", "skip_rescale", "swap_v_keys")


def _defect_fn(name, N):
    """The defects that act inside the softmax: (s, p, v) -> the defective output."""
    if name == "drop_last_key":
        def f(s, p, v):
            return torch.softmax(s[..., : N - 1], -1) @ v[..., : N - 1, :]
    elif name == "pad_bias_zero":     # the keys that pad the last 32-key tile: k^ = 0, v = 0, bias 0 instead of -1e30 -> logit 0, weight e^(0 - m) in the row sum
        pad = (-N) % 32

        def f(s, p, v):
            m = s.amax(-1, keepdim=True).clamp(min=0.0) if pad else s.amax(-1, keepdim=True)
            e = torch.exp(s - m)
            return (e @ v) / (e.sum(-1, keepdim=True) + pad * torch.exp(-m))
    elif name == "skip_rescale":      # O is not multiplied by alpha at the tile that holds the row maximum (l is): the earlier tiles keep their old weight
        def f(s, p, v):
            t = s.argmax(-1, keepdim=True) // 32
            key_t = torch.arange(N).view(1, 1, N) // 32
            early = key_t < t
            m = s.amax(-1, keepdim=True)
            m_old = torch.where(early, s, torch.full_like(s, -1e300)).amax(-1, keepdim=True)
            boost = torch.where(early, torch.exp((m - m_old).clamp(max=700.0)), torch.ones_like(s))
            return (p * boost) @ v
    elif name == "swap_v_keys":       # V^T read with keys N - 1 and N - 5 (one 8-key group) exchanged
        def f(s, p, v):
            idx = torch.arange(N)
            if N >= 8:
                idx[N - 1], idx[N - 5] = N - 5, N - 1
            return p @ v[..., idx, :]
    else:
        raise ValueError(name)
    return f


# ---------------------------------------------------------------------------------------------------------------------------------
# windowed cosine attention
# ---------------------------------------------------------------------------------------------------------------------------------
def window_attention_ref(qkv, table, scale, B, res, ws, shift, heads, model, defect=None, err=None, pair_chunk=16):
    """qkv [B res res][3 C] (float64 holding the operand values), table [(2 ws - 1)^2][heads], scale [heads] -> (out [B res res][C], bound).
    err: [B res res][3 C] bound on the error of the q, k, v the kernel starts from (the fused qkv form), or None.  defect: one of DEFECTS -> (defective out, None)."""
    C, N, nw = heads * 32, ws * ws, res // ws
    M = B * res * res
    rows = window_rows(B, res, ws, shift, roll_sign=-1 if defect == "roll_reversed" else 1)
    out_rows = window_rows(B, res, ws, shift, swap_windows=True) if defect == "reverse_swapped" else rows
    masked = window_masked(res, ws, shift, first=defect == "mask_first")
    bidx = bias_index(ws, transposed=defect == "bias_transposed")
    inner = _defect_fn(defect, N) if defect in ("drop_last_key", "pad_bias_zero", "skip_rescale", "swap_v_keys") else None
    sc = scale.roll(-1) if defect == "next_head_scale" else scale
    out = torch.zeros(M, C, dtype=torch.float64)
    bound = None if defect else torch.zeros(M, C, dtype=torch.float64)
    nW = rows.shape[0]
    for w in range(nW):
        x = qkv[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)          # [3][heads][N][32]
        e = None if err is None else err[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        mk = None if masked is None else masked[w % (nw * nw)]
        for h0 in range(0, heads, pair_chunk):
            hs = slice(h0, min(heads, h0 + pair_chunk))
            q, k, v = x[0, hs], x[1, hs], x[2, hs]
            bias = table[:, hs][bidx].permute(2, 0, 1)
            P = q.shape[0]
            m_ = None if mk is None else mk[None].expand(P, N, N)
            Eq = Ek = Ev = None
            if e is not None:
                Eq = _through_normalize(q, e[0, hs]) * sc[hs].view(P, 1, 1)
                Ek = _through_normalize(k, e[1, hs])
                Ev = e[2, hs] + U16[model.fmt] * (v.abs() + e[2, hs]) + SUBNORMAL[model.fmt]
            s, eps = _cosine_logits(q, k, sc[hs].view(P, 1, 1), bias, m_, model.fmt, Eq, Ek)
            o, bd = _softmax_bound(s, eps, v, model, Ev, inner)
            out[out_rows[w], 32 * h0: 32 * (h0 + P)] = o.permute(1, 0, 2).reshape(N, 32 * P)
            if bound is not None:
                bound[out_rows[w], 32 * h0: 32 * (h0 + P)] = bd.permute(1, 0, 2).reshape(N, 32 * P)
    return out, bound


def _through_normalize(x, e):
    """|d (x / |x|)_i| for |dx_i| <= e_i: (e_i + |x~_i| sum_k |x~_k| e_k) / (|x| - |e|); an exactly zero vector with zero error stays zero."""
    n = x.norm(dim=-1, keepdim=True)
    en = e.norm(dim=-1, keepdim=True)
    xt = x.abs() / n.clamp(min=1e-300)
    d = (e + xt * (xt * e).sum(-1, keepdim=True)) / (n - en).clamp(min=1e-300)
    return torch.where((n == 0) & (en == 0), torch.zeros_like(d), d)


def qkv_projection_ref(x, w, bias):
    """x [M][C], w [3 C][C], bias [3 C] (float64 holding the operand values) -> (qkv [M][3 C] in float64, the bound on the kernel's f32 accumulators + bias)."""
    C = x.shape[1]
    qkv = x @ w.t() + bias
    return qkv, gamma(C + 2) * (x.abs() @ w.abs().t() + bias.abs())


def window_attention_qkv_ref(x, w, bias, table, scale, B, res, ws, shift, heads, fmt, defect=None):
    """The fused form: fmt = 'bf16' / 'f16' / 'x2w' (w then holds the decoded x3 pairs; the arithmetic after the projection is the fp16 kernel's)."""
    qkv, err = qkv_projection_ref(x, w, bias)
    return window_attention_ref(qkv, table, scale, B, res, ws, shift, heads, window_model("bf16" if fmt == "bf16" else "f16", ws), defect, err=err)


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT attention
# ---------------------------------------------------------------------------------------------------------------------------------
def vit_attention_ref(qkv, B, N, heads, model, defect=None):
    """qkv [B N][3 heads 64] -> (out [B N][heads 64], bound): softmax(q k^T / 8) v."""
    d = 64
    x = qkv.reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    out = torch.zeros(B, N, heads * d, dtype=torch.float64)
    bound = None if defect else torch.zeros_like(out)
    inner = _defect_fn(defect, N) if defect else None
    for b in range(B):
        q, k, v = x[0, b] * 0.125, x[1, b], x[2, b]
        s = q @ k.transpose(-1, -2)
        eps = gamma(66) * (q.abs() @ k.abs().transpose(-1, -2)) + SUBNORMAL[model.fmt] * k.abs().sum(-1)[:, None, :]
        o, bd = _softmax_bound(s, eps, v, model, None, inner)
        out[b] = o.permute(1, 0, 2).reshape(N, heads * d)
        if bound is not None:
            bound[b] = bd.permute(1, 0, 2).reshape(N, heads * d)
    return out.reshape(B * N, heads * d), None if bound is None else bound.reshape(B * N, heads * d)


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def plants(ws, shift, nw):
    """(window, query token, key token) triples: the key's k is the query's q (cosine exactly 1).  Window 0 (never masked): key N - 1; the first key of the last
    32-key tile (its last is N - 1); a key of a middle tile -- each lies in a later tile than everything the query has seen, so the running maximum jumps there.
    Shifted: a top-half query with a bottom-half key in a last-row window, a left-half query with a right-half key in a last-column window (masked pairs)."""
    N = ws * ws
    NT = (N + 31) // 32
    out = [(0, 3, N - 1)]
    if NT >= 2:
        out.append((0, 5, 32 * (NT - 1)))
    if NT >= 3:
        out.append((0, 7, 32 * (NT // 2) + 9))
    if shift:
        out.append(((nw - 1) * nw, 1 * ws + 2, (ws - 1) * ws + 3))        # window (wy = nw - 1, wx = 0)
        out.append((nw - 1, 2 * ws + 1, 3 * ws + ws - 1))                 # window (wy = 0, wx = nw - 1)
    return out


SPECIAL = {"q_big": 10, "q_small": 11, "k_big": 12, "k_small": 13, "v_big": 14, "v_small": 15, "q_zero": 16, "k_zero": 17}     # tokens of window 0


def head_scales(heads):
    return torch.tensor([HEAD_SCALES[h % 3] for h in range(heads)], dtype=torch.float64)


def cpb_table(ws, heads, g):
    """16 sigmoid(3 randn): values near both 0 and 16; f32 values.  Head 0 (logit scale 1) keeps to the low side, 16 sigmoid(randn - 8) < 0.2: all its logits are
    O(1), so a key that should have had zero weight (a padded key of a ragged tile with logit 0) is a visible share of its row sums."""
    z = 3 * torch.randn((2 * ws - 1) ** 2, heads, generator=g, dtype=torch.float64)
    z[:, 0] = z[:, 0] / 3 - 8.0
    return (16 * torch.sigmoid(z)).float().double()


def build_window(B, res, ws, shift, heads, fmt, seed=None):
    """-> dict(qkv [M][3 C], table, scale) of float64 tensors holding exact operand values of fmt ('bf16' / 'f16' / 'f32'): Gaussian q, k, v, the planted keys,
    and in window 0 the SPECIAL tokens (rows of q and k scaled by 2^+-10 -- q^ and k^ are invariant to that --, v rows by 2^3 and 2^-10, and one all-zero q row
    and k row)."""
    g = torch.Generator().manual_seed(1000 * res + 10 * heads + shift + ws if seed is None else seed)
    C, N, nw = heads * 32, ws * ws, res // ws
    qkv = torch.randn(B * res * res, 3, C, generator=g, dtype=torch.float64)
    qkv[:, 2, 31::32] += 4.0        # the last v channel of every head has a mean well above its spread: a weight share lost or gained anywhere in a row moves it
    rows = window_rows(B, res, ws, shift)
    for w, pq, pk in plants(ws, shift, nw):
        qkv[rows[w, pk], 1] = qkv[rows[w, pq], 0]
    r0 = rows[0]
    qkv[r0[SPECIAL["q_big"]], 0] *= 2.0 ** 10
    qkv[r0[SPECIAL["q_small"]], 0] *= 2.0 ** -10
    qkv[r0[SPECIAL["k_big"]], 1] *= 2.0 ** 10
    qkv[r0[SPECIAL["k_small"]], 1] *= 2.0 ** -10
    qkv[r0[SPECIAL["v_big"]], 2] *= 2.0 ** 3          # (v is not scale-free: a larger factor would only widen every allowance of the window by the spread it adds)
    qkv[r0[SPECIAL["v_small"]], 2] *= 2.0 ** -10
    qkv[r0[SPECIAL["q_zero"]], 0] = 0.0
    qkv[r0[SPECIAL["k_zero"]], 1] = 0.0
    return {"qkv": quantize(qkv.reshape(-1, 3 * C), fmt), "table": cpb_table(ws, heads, g), "scale": head_scales(heads)}


def build_window_qkv(B, res, ws, shift, heads, fmt, seed=None):
    """The fused form: x [M][C], w [3 C][C] (fmt 'x2w': f32 values, to be encoded as x3 pairs), bias [3 C] = cat(q_bias, 0, v_bias), table, scale.  Token
    SPECIAL['k_zero'] of window 0 has x = 0: its k is exactly zero (the k bias is), and with the q bias of head 0 zeroed so is that head's q.  Rows of x are scaled
    by 2^+-6 (q^ and k^ are invariant up to the bias)."""
    g = torch.Generator().manual_seed(2000 * res + 10 * heads + shift + ws if seed is None else seed)
    C = heads * 32
    act = "bf16" if fmt == "bf16" else "f16"
    x = torch.randn(B * res * res, C, generator=g, dtype=torch.float64) * 0.8
    w = torch.randn(3 * C, C, generator=g, dtype=torch.float64) / math.sqrt(C)
    qb, vb = torch.randn(C, generator=g, dtype=torch.float64) * 0.3, torch.randn(C, generator=g, dtype=torch.float64) * 0.3
    qb[:32] = 0.0
    r0 = window_rows(B, res, ws, shift)[0]
    x[r0[SPECIAL["q_big"]]] *= 2.0 ** 6
    x[r0[SPECIAL["q_small"]]] *= 2.0 ** -6
    x[r0[SPECIAL["k_zero"]]] = 0.0
    bias = torch.cat([qb, torch.zeros(C, dtype=torch.float64), vb]).float().double()
    return {"x": quantize(x, act), "w": quantize(w, "f32" if fmt == "x2w" else act), "bias": bias, "table": cpb_table(ws, heads, g), "scale": head_scales(heads)}


def build_vit(B, N, heads, fmt, seed=None):
    """Gaussian * 1.5 with the two large-match rows of tests/test_hybrid_gpu.py (query N // 2 and key N - 1 of head 0 set to 6: the running maximum jumps at the last
    key tile), and for N >= 8 one all-zero q row and one all-zero k row."""
    g = torch.Generator().manual_seed(B * 1000 + N + heads if seed is None else seed)
    d = 64
    qkv = torch.randn(B * N, 3 * heads * d, generator=g, dtype=torch.float64) * 1.5
    qkv[N // 2, :d] = 6.0
    qkv[N - 1, heads * d: heads * d + d] = 6.0
    if N >= 8:
        qkv[2, : heads * d] = 0.0
        qkv[3, heads * d: 2 * heads * d] = 0.0
    return {"qkv": quantize(qkv, fmt)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (B, res, ws, shift, heads) and what the launcher does with them (attention.hip launch_window_attention / _f32, vit_attention.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
WIN16_CASES = {
    "ws8": (2, 16, 8, 0, 3),                 # window_attention_kernel<8>
    "ws16": (1, 32, 16, 0, 3),               # window_attention_flash_kernel<16, *, 1>
    "ws16_shift": (1, 32, 16, 8, 3),         # the four windows: neither / last column / last row / both
    "ws12": (1, 12, 12, 0, 2),               # flash<12>: 144 keys, 16 padded keys in the fifth tile
    "ws12_shift": (1, 24, 12, 6, 4),
    "ws24_252": (1, 48, 24, 12, 63),         # 252 (window, head) pairs < 256: flash<24, *, 2>, the query split
    "ws24_256": (1, 48, 24, 12, 64),         # 256 pairs: flash<24, *, 1>
    "ws24_256_unshifted": (1, 48, 24, 0, 64),
}
WINF32_CASES = {                             # window_attention_f32_flash_kernel<8 / 16 / 12 / 24>
    "ws8": (2, 16, 8, 0, 3), "ws8_shift": (1, 16, 8, 4, 2), "ws16": (1, 32, 16, 0, 3), "ws16_shift": (1, 32, 16, 8, 3), "ws12": (1, 12, 12, 0, 2),
    "ws12_shift": (1, 24, 12, 6, 4), "ws24": (1, 24, 24, 0, 2), "ws24_shift": (1, 48, 24, 12, 3),
}
WINANY_CASES = {                             # window_attention_f32_any_kernel: 36 keys = one partial block of 64, 100 keys = two blocks
    "ws6": (1, 12, 6, 0, 2), "ws6_shift": (1, 12, 6, 3, 2), "ws10": (1, 20, 10, 0, 2), "ws10_shift": (1, 20, 10, 5, 2),
}
WINF32_WHOLE_CASES = {"ws16_shift": (1, 32, 16, 8, 3), "ws8": (2, 16, 8, 0, 3)}      # window_attention_f32_kernel<16> / <8>: SOCCDPT_ATTN_F32_FLASH16=0
QKV_CASES = {"ws16_shift": (1, 32, 16, 8, 3), "ws8": (2, 16, 8, 0, 6)}
VIT_CASES = [(B, N, heads) for B, N in ((1, 1), (1, 31), (1, 32), (1, 33), (1, 577), (1, 608), (22, 100)) for heads in (12, 16)]     # B, N, heads
VIT_X3_CASES = [(1, 33, 12), (1, 577, 12), (1, 577, 16), (1, 608, 16), (22, 100, 12)]      # the fp16 kernel's x3 store


def win16_split(B, res, ws, heads):
    """The query split launch_window_attention chooses."""
    return 2 if ws == 24 and B * (res // ws) ** 2 * heads < 256 else 1


_CACHE = {}


def cached(key, fn):
    """References are computed once per process and shared (never modified) by the tests that need them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def window_case(family, name, fmt):
    """(inputs, ref, bound) of a window case; family 'win16' / 'winf32' / 'winany' / 'whole'."""
    cases = {"win16": WIN16_CASES, "winf32": WINF32_CASES, "winany": WINANY_CASES, "whole": WINF32_WHOLE_CASES}[family]
    geom = cases[name]

    def make():
        inp = build_window(*geom, fmt)
        ref, bound = window_attention_ref(inp["qkv"], inp["table"], inp["scale"], *geom, window_model(fmt, geom[2], per_key=family == "winany"))
        return inp, ref, bound
    return cached((family if family == "winany" else "win", geom, fmt), make)


def qkv_case(name, fmt):
    geom = QKV_CASES[name]

    def make():
        inp = build_window_qkv(*geom, fmt)
        ref, bound = window_attention_qkv_ref(inp["x"], x3_value(inp["w"]) if fmt == "x2w" else inp["w"], inp["bias"], inp["table"], inp["scale"], *geom, fmt)
        return inp, ref, bound
    return cached(("qkv", geom, fmt), make)


def vit_case(B, N, heads, fmt):
    def make():
        inp = build_vit(B, N, heads, fmt)
        ref, bound = vit_attention_ref(inp["qkv"], B, N, heads, vit_model(fmt, N))
        return inp, ref, bound
    return cached(("vit", B, N, heads, fmt), make)


def x3_value(w):
    """What an x3 pair of w represents: hi + lo / 2048 with hi = RN16(w), lo = RN16((w - hi) 2048) (csrc/half16.h), as float64."""
    hi = round16(w.clamp(-65504.0, 65504.0), "f16")
    lo = round16(((w.float().double() - hi) * 2048.0).clamp(-65504.0, 65504.0), "f16")
    return hi + lo / 2048.0


def check_output(got, fmt_out, ref, bound, what):
    """got: the kernel's output tensor (16-bit, f32, or flat fp16 x3 storage with fmt_out = 'x3') -> the worst error as a fraction of its allowance.
    A 16-bit output is judged by check_interval16; the fraction that check returns is 1 whenever a value sits on the end of its interval (a grid point, often one of
    two), so the figure reported for a 16-bit output is |got - ref| over bound + the output's own rounding u16 (|ref| + bound) instead."""
    if fmt_out == "f32":
        return check_bound(got, ref, bound, what)
    if fmt_out == "x3":
        return check_x3_interval(got, tuple(ref.shape), ref, bound, what)
    check_interval16(got, ref, bound, fmt_out, what)
    return float(((got.double().cpu() - ref).abs() / (bound + U16[fmt_out] * (ref.abs() + bound) + SUBNORMAL[fmt_out])).max())
