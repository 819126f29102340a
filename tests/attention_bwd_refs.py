"""Float64 references of the attention backward of the training step (csrc/train_attn.hip attn_bwd_mfma_kernel / vit_attn_bwd_mfma_kernel, csrc/train.hip
tr_attn_param_grads / tr_qv_bias_grad), each with an a-priori per-element error bound, and the inputs the GPU tests and the CPU self-test share.  Geometry, mask
and bias-index helpers, check_bound, gamma, U16, SUBNORMAL, NORM, EXP_ULPS and HEAD_SCALES are tests/attention_refs.py's; so are the conventions: a reference
starts from the exact f32 values the kernel reads and returns (expected, bound), |kernel - expected| <= bound must hold for every element, nothing is fitted to a
measured error.

Expected values: the exact gradients of the function the kernel differentiates,
    q^ = scale q / max(|q|, 1e-12),  k^ = k / max(|k|, 1e-12),  S = q^ k^T + bias + mask(-100),  P = softmax(S),  O = P v,
    dP = dO v^T,  delta = rowsum(P o dP),  dS = P (dP - delta),  dq^ = dS k^,  dk^ = dS^T q^,  dv = P^T dO,
    dq = (scale / |q|) (dq^ - q~ (q~ . dq^)),  dk = (1 / |k|) (dk^ - k~ (k~ . dk^))   (x~ the unit vector),  dscale = sum dS (q^ . k^) / scale,
    rowstat = {m + ln l = logsumexp(S), delta};     ViT: S = (q / 8) k^T, head dimension 64, dq = (dS k) / 8, dk = dS^T (q / 8), no bias, mask or normalisation.
tests/test_attention_bwd_refs.py holds these closed forms against float64 autograd over the same forward.  attn_out, which the f32 kernels read for delta = dO . O,
is the f32 image of the exact O.

Bounds: first-order running-error analysis.  Beside every float64 quantity x a float64 magnitude E_x >= |kernel's x - x| is carried through the same formula
with absolute values (a product: E_a |b| + |a| E_b + E_a E_b + u |ab|; a sum: E_a + E_b + u |a + b|; an n-long accumulation: gamma(n) sum |terms|), so the
cancellations in dP - delta, in g - x~ (x~ . g) and in the dscale sum are bounded by the size of their terms, not of the result.  u = 2^-24.  The terms:
* q^, k^:  E = NORM |x^| (NORM = gamma(24): the forward's allowance for 32 squares, sqrtf, the division and the product).
* Scores (f32 MFMA in every form): E_raw = E_q |k^| + |q^| E_k + E_q E_k + gamma(32) |q^| |k^| (gamma(64) in the ViT form, q / 8 exact);
  E_S = E_raw + u |bias - 100 [masked]| + u |S|   (the table entry + -100, then the add to the raw score).
* m + ln l:  the kernel's weight of key j against the final maximum carries the relative error w_j = 3 u (m - s_j) + u ((EXP_ULPS + 2)(NT + 1) + 18): the
  argument (s - mn) LOG2E has the subtraction's, the product's and the constant's rounding (3 u |argument| in natural units, telescoping to m - s_j over the
  rescales), v_exp_f32 EXP_ULPS, every one of the NT rescales one more exp2, one product and one sum, and the 16 in-tile adds + the half-wave exchange.  Hence
  E_l / l = sum_j p_j w_j, the logits move logsumexp by at most sum_j p_j E_S_j, __logf (v_log_f32 times ln 2) is allowed max(2^-21, 4 u |ln l|) absolute and the
  final sum u |m + ln l|.
* P = exp2((S - (m + ln l)) LOG2E):  E_P = P (expm1(E_S + E_mln + 3 u |S - mln|) + EXP_ULPS u) + 2^-126 (f32 underflow: the weight of a masked pair may be
  flushed to zero; the same on dS).
* dP:  f32 form gamma(32) |dO| |v|^T (gamma(64) ViT).  16-bit forms: both operands are rounded, E_x16 = U16 |x| + SUBNORMAL (+ (1 + U16) E_x for an operand
  that already carries an error), products of 16-bit values are exact, 16 of them are added per MFMA step: gamma(5 steps), 5 roundings per step as in
  tests/fused_refs.py gemm_gamma.
* delta:  f32 form: 16 (32) fmas + the half-wave exchange + the rounding of attn_out, gamma(d / 2 + 2) sum |dO| |O|.  16-bit forms: the kernel's
  delta = rowsum(P o dP16) is accumulated online beside l: sum_j p_j (E_dP_j + (|dP_j| + E_dP_j) expm1(E_S_j + sum p E_S + w_j + E_l / l)) -- E_dP holds the U16
  terms, which is how the U16 distance to the exact delta enters -- + gamma(16 + NT + 4) sum_j p_j (|dP_j| + E_dP_j) + u |delta| for the division.
* dS = P (dP - delta):  the sum and product rules above.
* dq^, dk^, dv: accumulated over the walked axis, Npad = 32 NT products: f32 gamma(Npad + 2); 16-bit: dS, P, k^, q^, v, dO fragments rounded (E_x16), gamma(5 Npad / 16 + 2).
* Through the normalisation:  g = scale dq^ (u), x~ = x / nrm (NORM), dot = 16 fmas + exchange (gamma(18)), t = x~ dot (u), g - t (u), / nrm (NORM + u):
  E = (E_g + E_t + u |g - t|) (1 + NORM) / |x| + (NORM + u) |result|.   ViT: dq = dq^ / 8 exactly.
* dscale (the sum of the per-wave slots, added in float64 by the test):  (sum (E_dS (|raw| + E_raw) + |dS| E_raw) + gamma(Npad / 2 + 8) sum |dS raw|) / scale + u.
* Relational: every row of dS sums to zero.  The kernel's row is an f32 computation on ITS dP (whatever the operand format), whose exact row sum is zero, so
  |sum_j dS_ij| <= sum_j E'_dS_ij, E' the dS bound with the U16 terms of dP left out (only the accumulation rounding of dP stays) and magnitudes |dP| + E_dP.
  A delta taken from the exact dO . O in a 16-bit form breaks this by U16 sum p |dO| |v|: why those forms accumulate delta online.

Parameter-gradient chain (tr_attn_param_grads), expected = float64 autograd through table = 16 sigmoid(relu(coords W0^T + b0) W2^T) with timm's log-spaced
coordinates (divided by pws - 1 when a pretrained window is given):
* window sum: gamma(nwin) sum_w |dS|;  table gradient: gamma(ws^2) on sum |dS| (one lane adds at most ws entries, then six exchanges) -- together
  gamma(ws^2 + nwin) sum |dS| over the pairs of the entry.
* dt = dtable 16 s (1 - s), s = table / 16 from the f32 table:  E_s = u s, E_(1-s) = u s + u |1 - s|, three products.
* coordinates in f32 (division, log2f, product with 1 / log2f(8)): gamma(8) |c|;  pre-activation gamma(4) (|c0 w0| + |c1 w1| + |b0|) + the coordinates' share.
  Floating point must not decide the ReLU: build_params nudges b0 of any hidden unit whose float64 pre-activation is within 4 gamma(4 + 8) (|c0 w0| + |c1 w1| + |b0|)
  of zero at any table row and asserts that none is left within gamma(4) (...) + the coordinate term (an error, not a skip).
* cpb_reduce_kernel: a thread adds ceil(T2 / 64) + 1 products into each of four streams, three adds join them, sixteen partials follow: gamma(ceil(T2 / 64) + 21).
  dhid: gamma(heads + 1).
* dls = [ls <= float32(ln 100)] exp(ls) sum(partials): gamma(ceil(nwin slots / 256) + 9) for the block reduction, u (EXP_ULPS + 2 |ls| + 1) for __expf and the
  product.  torch.clamp passes the gradient at equality.
"""
from __future__ import annotations

import math

import torch

from tests import attention_refs as AR
from tests.attention_refs import EXP_ULPS, NORM, SUBNORMAL, U16, cached, check_bound, gamma  # noqa: F401  (re-exported for the tests)
from tests.fused_refs import U, round16

LN100_F32 = float(torch.tensor(4.605170185988092, dtype=torch.float32))
FMTS = ("f32", "bf16", "f16")
TINY = 2.0 ** -126        # f32 underflow: a weight or a dS below the normal range (a masked pair: e^-100 and less) may be flushed to zero

# (B, res, ws, shift, heads): the smallest shapes at which attn_bwd_mfma_kernel can still go wrong
WIN_CASES = {
    "ws8_shift": (1, 16, 8, 4, 2),        # N = 64: two walked tiles, one block whose waves 2 and 3 own nothing (their dscale slots are 0)
    "ws8": (1, 16, 8, 0, 2),
    "ws12_shift": (1, 24, 12, 6, 3),      # N = 144: four full tiles + 16 real keys; the second block has one live wave, half of whose lanes own no token; scale 100
    "ws12": (1, 24, 12, 0, 3),
    "ws12_b2": (2, 12, 12, 0, 1),
    "ws16_shift": (1, 32, 16, 8, 1),      # N = 256: every wave full
    "ws24_shift": (1, 48, 24, 12, 1),     # N = 576: 18 tiles, five blocks, the last with two live waves
    "ws24": (1, 24, 24, 0, 1),
}
VIT_CASES = [(2, 33, 2), (2, 64, 2), (2, 129, 2), (1, 577, 1)]        # B, N, heads: one token in the second tile / no padding / a second block with one live lane / the model's length
PARAM_CASES = [(8, 0, 1, 1), (8, 8, 4, 3), (12, 12, 4, 2), (24, 12, 2, 1)]      # ws, pws, nwin, heads


def slots(ws):
    """tr_attention_bwd_mfma_slots."""
    return ((ws * ws + 31) // 32 + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# running-error helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _op16(x, Ex, fmt):
    """Error of a product operand after the kernel rounds it to fmt (nothing for f32)."""
    if fmt == "f32":
        return Ex
    return Ex + U16[fmt] * (x.abs() + Ex) + SUBNORMAL[fmt]


def _mm(a, Ea, b, Eb, n):
    """a @ b with an n-rounding accumulation -> (value, bound)."""
    aa, ab = a.abs() + Ea, b.abs() + Eb
    return a @ b, Ea @ b.abs() + a.abs() @ Eb + Ea @ Eb + gamma(n) * (aa @ ab)


def _acc_len(fmt, k):
    """Roundings of a k-long dot product: the f32 MFMA adds one product at a time, a 16-bit MFMA step 16 (5 roundings)."""
    return k + 2 if fmt == "f32" else 5 * -(-k // 16) + 2


def _softmax_bwd(s, Es, a, Ea, b, Eb, v, dO, O32, fmt, d):
    """The part both kernels share.  s, Es [..][N][N] (logits and their bound); a, b [..][N][d] the operands of the scores (q^ / k^, or q / 8 and k) with their
    bounds; v, dO, O32 [..][N][d].  -> dict of (value, bound) pairs: ds, mln, delta, da (= dS b), db (= dS^T a), dv, and rowsum (the bound on |sum_j dS_ij|)."""
    N = s.shape[-1]
    NT = (N + 31) // 32
    Npad = 32 * NT
    m = s.amax(-1, keepdim=True)
    L = torch.logsumexp(s, -1, keepdim=True)
    P = torch.exp(s - L)
    gap = (m - s).clamp(max=1e4)
    w = 3 * U * gap + U * ((EXP_ULPS + 2) * (NT + 1) + 18)
    PEs = (P * Es).sum(-1, keepdim=True)
    El = (P * w).sum(-1, keepdim=True)
    lnl = L - m
    E_L = PEs + El + torch.clamp(4 * U * lnl.abs(), min=2.0 ** -21) + U * L.abs()
    E_P = P * (torch.expm1(Es + E_L + 3 * U * (s - L).abs().clamp(max=1e4)) + EXP_ULPS * U) + TINY
    vT = v.transpose(-1, -2)
    dP = dO @ vT
    EdO, EvT = _op16(dO, 0.0 * dO, fmt), _op16(vT, 0.0 * vT, fmt)
    mag_dP = (dO.abs() + EdO) @ (vT.abs() + EvT)
    E_dP_acc = gamma(_acc_len(fmt, d) - 2) * mag_dP                      # the accumulation alone: the kernel's dP as data
    E_dP = EdO @ vT.abs() + dO.abs() @ EvT + EdO @ EvT + E_dP_acc
    delta = (P * dP).sum(-1, keepdim=True)

    def ds_bound(E_dP_, extra):
        """E_dP_: the error of dP that counts; extra: what else the kernel's |dP - delta| may exceed the exact one by."""
        a_dP = dP.abs() + E_dP
        if fmt == "f32":
            E_delta = gamma(d // 2 + 2) * (dO.abs() * O32.abs()).sum(-1, keepdim=True)
        else:
            relp = torch.expm1(Es + PEs + w + El)
            E_delta = (P * (E_dP_ + a_dP * relp)).sum(-1, keepdim=True) + gamma(16 + NT + 4) * (P * a_dP).sum(-1, keepdim=True) + U * delta.abs()
        diff = dP - delta
        E_diff = E_dP_ + E_delta + U * diff.abs()
        dS = P * diff
        return dS, E_P * (diff.abs() + extra) + P * E_diff + E_P * E_diff + U * dS.abs() + TINY, E_delta

    dS, E_dS, E_delta = ds_bound(E_dP, 0.0)
    rowsum = E_dS.sum(-1) if fmt == "f32" else ds_bound(E_dP_acc, E_dP + E_delta)[1].sum(-1)
    n = _acc_len(fmt, Npad)
    da = _mm(dS, _op16(dS, E_dS, fmt), b, _op16(b, Eb, fmt), n)
    db = _mm(dS.transpose(-1, -2), _op16(dS, E_dS, fmt).transpose(-1, -2), a, _op16(a, Ea, fmt), n)
    dv = _mm(P.transpose(-1, -2), _op16(P, E_P, fmt).transpose(-1, -2), dO, EdO, n)
    return {"ds": (dS, E_dS), "mln": (L, E_L), "delta": (delta, E_delta), "da": da, "db": db, "dv": dv, "rowsum": rowsum, "P": P}


def _normalize_bwd(x, g, Eg, gs):
    """out = (gs / |x|) (g - x~ (x~ . g)) as the kernel forms it -> (value, bound).  x [..][N][32], g, Eg the gradient w.r.t. the normalised (and scaled) vector."""
    nrm = x.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    xt = x / nrm
    Ex = NORM * xt.abs()
    G = g * gs
    EG = Eg * gs + U * G.abs()
    dot = (xt * G).sum(-1, keepdim=True)
    Edot = (xt.abs() * EG + Ex * (G.abs() + EG)).sum(-1, keepdim=True) + gamma(18) * (xt * G).abs().sum(-1, keepdim=True)
    t = xt * dot
    Et = Ex * dot.abs() + xt.abs() * Edot + Ex * Edot + U * t.abs()
    diff = G - t
    out = diff / nrm
    return out, (EG + Et + U * diff.abs()) * (1 + NORM) / nrm + (NORM + U) * out.abs()


# ---------------------------------------------------------------------------------------------------------------------------------
# windowed cosine attention backward
# ---------------------------------------------------------------------------------------------------------------------------------
def window_forward(qkv, table, scale, B, res, ws, shift, heads):
    """The exact forward in float64 -> O [B res res][heads 32] (the tests hand its f32 image to the kernel as attn_out)."""
    C, N, nw = heads * 32, ws * ws, res // ws
    rows = AR.window_rows(B, res, ws, shift)
    masked = AR.window_masked(res, ws, shift)
    bias = table[AR.bias_index(ws)].permute(2, 0, 1)
    out = torch.zeros(B * res * res, C, dtype=torch.float64)
    for w in range(rows.shape[0]):
        x = qkv[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        qh = x[0] / x[0].norm(dim=-1, keepdim=True).clamp(min=1e-12) * scale.view(-1, 1, 1)
        kh = x[1] / x[1].norm(dim=-1, keepdim=True).clamp(min=1e-12)
        s = qh @ kh.transpose(-1, -2) + bias
        if masked is not None:
            s = s - 100.0 * masked[w % (nw * nw)]
        out[rows[w]] = (torch.softmax(s, -1) @ x[2]).permute(1, 0, 2).reshape(N, C)
    return out


def window_bwd_ref(inp, B, res, ws, shift, heads, fmt):
    """inp: qkv [M][3 C], dout [M][C], attn_out [M][C] (f32 image of the exact O), table, scale, all float64 holding f32 values ->
    dict name -> (expected, bound): dqkv [M][3 C], ds [nwin][heads][N][N], rowstat [nwin][heads][N][2], dscale [nwin][heads], and 'rowsum' -> the bound
    [nwin][heads][N] on |sum_j dS_ij|."""
    C, N, nw = heads * 32, ws * ws, res // ws
    M = B * res * res
    NT = (N + 31) // 32
    rows = AR.window_rows(B, res, ws, shift)
    masked = AR.window_masked(res, ws, shift)
    bias = inp["table"][AR.bias_index(ws)].permute(2, 0, 1)
    sc = inp["scale"].view(-1, 1, 1)
    nwin = rows.shape[0]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)      # noqa: E731
    dqkv, Edqkv = z(M, 3 * C), z(M, 3 * C)
    ds, Eds = z(nwin, heads, N, N), z(nwin, heads, N, N)
    rowstat, Erowstat = z(nwin, heads, N, 2), z(nwin, heads, N, 2)
    dscale, Edscale = z(nwin, heads), z(nwin, heads)
    rowsum = z(nwin, heads, N)
    for w in range(nwin):
        x = inp["qkv"][rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]
        dO = inp["dout"][rows[w]].reshape(N, heads, 32).permute(1, 0, 2)
        O32 = inp["attn_out"][rows[w]].reshape(N, heads, 32).permute(1, 0, 2)
        qh = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12) * sc
        kh = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        Eq, Ek = NORM * qh.abs(), NORM * kh.abs()
        raw, Eraw = _mm(qh, Eq, kh.transpose(-1, -2), Ek.transpose(-1, -2), 32)
        b = bias if masked is None else bias - 100.0 * masked[w % (nw * nw)]
        s = raw + b
        Es = Eraw + U * b.abs() + U * s.abs()
        r = _softmax_bwd(s, Es, qh, Eq, kh, Ek, v, dO, O32, fmt, 32)
        dS, EdS = r["ds"]
        dq, Edq = _normalize_bwd(q, *r["da"], sc)
        dk, Edk = _normalize_bwd(k, *r["db"], 1.0)
        for i, (val, err) in enumerate(((dq, Edq), (dk, Edk), r["dv"])):
            dqkv[rows[w], i * C:(i + 1) * C] = val.permute(1, 0, 2).reshape(N, C)
            Edqkv[rows[w], i * C:(i + 1) * C] = err.permute(1, 0, 2).reshape(N, C)
        ds[w], Eds[w] = dS, EdS
        rowstat[w] = torch.cat([r["mln"][0], r["delta"][0]], -1)
        Erowstat[w] = torch.cat([r["mln"][1], r["delta"][1]], -1)
        rowsum[w] = r["rowsum"]
        dscale[w] = (dS * raw).sum((-1, -2)) / sc.view(-1)
        Edscale[w] = ((EdS * (raw.abs() + Eraw) + dS.abs() * Eraw).sum((-1, -2)) + gamma(16 * NT + 8) * (dS * raw).abs().sum((-1, -2))) / sc.view(-1) + U * dscale[w].abs()
    return {"dqkv": (dqkv, Edqkv), "ds": (ds, Eds), "rowstat": (rowstat, Erowstat), "dscale": (dscale, Edscale), "rowsum": rowsum}


def vit_forward(qkv, B, N, heads):
    x = qkv.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return (torch.softmax((x[0] * 0.125) @ x[1].transpose(-1, -2), -1) @ x[2]).permute(0, 2, 1, 3).reshape(B * N, heads * 64)


def vit_bwd_ref(inp, B, N, heads, fmt):
    """inp: qkv [B N][3 E], dout, attn_out [B N][E] -> dqkv [B N][3 E], rowstat [B][heads][N][2] as (expected, bound)."""
    E = heads * 64
    x = inp["qkv"].reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    q8, k, v = x[0] * 0.125, x[1], x[2]
    dO = inp["dout"].reshape(B, N, heads, 64).permute(0, 2, 1, 3)
    O32 = inp["attn_out"].reshape(B, N, heads, 64).permute(0, 2, 1, 3)
    zero = 0.0 * q8
    s, Es = _mm(q8, zero, k.transpose(-1, -2), zero.transpose(-1, -2), 64)
    r = _softmax_bwd(s, Es, q8, zero, k, zero, v, dO, O32, fmt, 64)
    parts = ((r["da"][0] * 0.125, r["da"][1] * 0.125), r["db"], r["dv"])
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, E)      # noqa: E731
    dqkv = torch.cat([back(p[0]) for p in parts], -1)
    Edqkv = torch.cat([back(p[1]) for p in parts], -1)
    rowstat = torch.cat([r["mln"][0], r["delta"][0]], -1)
    Erowstat = torch.cat([r["mln"][1], r["delta"][1]], -1)
    return {"dqkv": (dqkv, Edqkv), "rowstat": (rowstat, Erowstat)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the parameter-gradient chain
# ---------------------------------------------------------------------------------------------------------------------------------
def cpb_coords(ws, pws):
    """timm's relative_coords_table, [(2 ws - 1)^2][2] in float64: sign(c) log2(|c| + 1) / log2(8), c = 8 (offset) / ((pws or ws) - 1)."""
    r = torch.arange(-(ws - 1), ws, dtype=torch.float64)
    c = torch.stack(torch.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2) / ((pws if pws > 0 else ws) - 1) * 8.0
    return torch.sign(c) * torch.log2(c.abs() + 1.0) / math.log2(8.0)


def cpb_table_of(w0, b0, w2, ws, pws):
    return 16.0 * torch.sigmoid(torch.relu(cpb_coords(ws, pws) @ w0.t() + b0) @ w2.t())


def _pre_margin(c, w0, b0, n):
    return gamma(n) * (c[:, :1].abs() * w0[:, 0].abs() + c[:, 1:].abs() * w0[:, 1].abs() + b0.abs())


def param_grads_ref(inp, ws, pws, nwin, heads, gate_strict=False):
    """inp: ds [nwin][heads][N][N], part [nwin][heads][slots], table (f32 image of the exact table), ls, w0, b0, w2 -> name -> (expected, bound) for
    dssum [heads][N][N], dls, dw0, db0, dw2.  gate_strict: the defect `ls < ln 100`."""
    T2 = (2 * ws - 1) ** 2
    ds = inp["ds"]
    dssum = ds.sum(0)
    a_dssum = ds.abs().sum(0)
    E_dssum = gamma(nwin) * a_dssum
    idx = AR.bias_index(ws).reshape(-1)
    N2 = idx.numel()
    dtable = torch.zeros(T2, heads, dtype=torch.float64).index_add_(0, idx, dssum.reshape(heads, N2).t())
    E_dtable = gamma(ws * ws + nwin) * torch.zeros(T2, heads, dtype=torch.float64).index_add_(0, idx, a_dssum.reshape(heads, N2).t())
    c = cpb_coords(ws, pws)
    Ec = gamma(8) * c.abs()
    w0, b0, w2 = inp["w0"], inp["b0"], inp["w2"]
    pre = c @ w0.t() + b0
    hid = torch.relu(pre)
    on = (pre > 0).double()
    E_hid = on * (_pre_margin(c, w0, b0, 4) + Ec @ w0.abs().t())
    t = hid @ w2.t()
    sg = torch.sigmoid(t)                               # the kernel: table / 16 from the f32 table
    dt = dtable * 16.0 * sg * (1 - sg)
    E_dt = E_dtable * 16.0 * sg * (1 - sg) + dtable.abs() * 16.0 * (U * sg * (1 - sg) + sg * (U * sg + U * (1 - sg))) + 4 * U * dt.abs()
    Lr = -(-T2 // 64) + 21
    dw2 = dt.t() @ hid
    E_dw2 = E_dt.t() @ hid + dt.abs().t() @ E_hid + E_dt.t() @ E_hid + gamma(Lr) * (dt.abs().t() @ hid)
    dhid = on * (dt @ w2)
    E_dhid = on * (E_dt @ w2.abs() + gamma(heads + 1) * (dt.abs() @ w2.abs()))
    dw0 = dhid.t() @ c
    E_dw0 = E_dhid.t() @ c.abs() + dhid.abs().t() @ Ec + E_dhid.t() @ Ec + gamma(Lr) * (dhid.abs().t() @ c.abs())
    db0 = dhid.sum(0)
    E_db0 = E_dhid.sum(0) + gamma(Lr) * dhid.abs().sum(0)
    part = inp["part"]
    ls = inp["ls"]
    passes = (ls < LN100_F32) if gate_strict else (ls <= LN100_F32)
    e = torch.exp(ls)
    dls = torch.where(passes, e * part.sum((0, 2)), torch.zeros_like(ls))
    E_dls = torch.where(passes, (gamma(-(-nwin * part.shape[-1] // 256) + 9) + U * (EXP_ULPS + 2 * ls.abs() + 1)) * e * part.abs().sum((0, 2)), torch.zeros_like(ls))
    return {"dssum": (dssum, E_dssum), "dtable": (dtable, E_dtable), "dls": (dls, E_dls), "dw0": (dw0, E_dw0), "db0": (db0, E_db0), "dw2": (dw2, E_dw2)}


def build_params(ws, pws, nwin, heads, seed=None):
    """Seeded inputs of the chain.  ls: below the clamp, above it and exactly at float32(ln 100), cycled over the heads (one head: at the boundary).  b0 of a
    hidden unit whose pre-activation comes close to zero at some table row is moved until it does not (see the module docstring); none may be left."""
    g = torch.Generator().manual_seed(7000 + 100 * ws + 10 * pws + nwin + heads if seed is None else seed)
    f32 = lambda t: t.float().double()      # noqa: E731
    N = ws * ws
    w0 = f32(torch.randn(512, 2, generator=g, dtype=torch.float64))
    b0 = f32(torch.randn(512, generator=g, dtype=torch.float64) * 0.5)
    w2 = f32(torch.randn(heads, 512, generator=g, dtype=torch.float64) * 0.08)
    c = cpb_coords(ws, pws)
    for _ in range(8):
        pre = c @ w0.t() + b0
        close = (pre.abs() <= 4 * _pre_margin(c, w0, b0, 12)).any(0)
        if not bool(close.any()):
            break
        b0 = torch.where(close, f32(b0 + 2.0 ** -10 * (1 + b0.abs())), b0)
    pre = c @ w0.t() + b0
    assert not bool((pre.abs() <= _pre_margin(c, w0, b0, 12)).any()), "a hidden unit of the CPB MLP sits on the ReLU kink: floating point would decide its gradient"
    ls_all = torch.tensor([LN100_F32, 2.0, 5.0], dtype=torch.float64)
    ls = ls_all[torch.arange(heads) % 3]
    ds = f32(torch.randn(nwin, heads, N, N, generator=g, dtype=torch.float64) * torch.rand(nwin, heads, N, 1, generator=g, dtype=torch.float64))
    part = f32(torch.randn(nwin, heads, slots(ws), generator=g, dtype=torch.float64))
    return {"ds": ds, "part": part, "table": f32(cpb_table_of(w0, b0, w2, ws, pws)), "ls": ls, "w0": w0, "b0": b0, "w2": w2}


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def build_window(B, res, ws, shift, heads, seed=None):
    """f32 values (as float64) shared by the three operand forms: Gaussian q, k, v, dO; in every window a few q / k rows scaled by 2^+-4, in window 0 one q row
    and one k row of tiny norm (2^-10: the normalisation backward divides by it); the planted keys of tests/attention_refs.py (cosine exactly 1, masked pairs
    included); table entries in (0, 16); HEAD_SCALES cycled over the heads."""
    g = torch.Generator().manual_seed(9000 + 1000 * ws + 10 * heads + shift + res + B if seed is None else seed)
    C, nw = heads * 32, res // ws
    M = B * res * res
    qkv = torch.randn(M, 3, C, generator=g, dtype=torch.float64)
    rows = AR.window_rows(B, res, ws, shift)
    for w, pq, pk in AR.plants(ws, shift, nw):
        qkv[rows[w, pk], 1] = qkv[rows[w, pq], 0]
    for w in range(rows.shape[0]):
        qkv[rows[w, 20], 0] *= 16.0
        qkv[rows[w, 21], 1] *= 16.0
        qkv[rows[w, 22], 0] *= 1.0 / 16
        qkv[rows[w, 23], 1] *= 1.0 / 16
    qkv[rows[0, 11], 0] *= 2.0 ** -10
    qkv[rows[0, 13], 1] *= 2.0 ** -10
    dout = torch.randn(M, C, generator=g, dtype=torch.float64)
    f32 = lambda t: t.float().double()      # noqa: E731
    inp = {"qkv": f32(qkv.reshape(M, 3 * C)), "dout": f32(dout), "table": AR.cpb_table(ws, heads, g), "scale": AR.head_scales(heads)}
    inp["attn_out"] = f32(window_forward(inp["qkv"], inp["table"], inp["scale"], B, res, ws, shift, heads))
    return inp


def build_vit(B, N, heads, seed=None):
    g = torch.Generator().manual_seed(11000 + 1000 * B + N + heads if seed is None else seed)
    E = heads * 64
    qkv = torch.randn(B * N, 3 * E, generator=g, dtype=torch.float64) * 1.5
    qkv[N // 2, :64] = 6.0                       # the two large-match rows of tests/attention_refs.py build_vit: the running maximum jumps at the last key tile
    qkv[N - 1, E:E + 64] = 6.0
    f32 = lambda t: t.float().double()      # noqa: E731
    inp = {"qkv": f32(qkv), "dout": f32(torch.randn(B * N, E, generator=g, dtype=torch.float64))}
    inp["attn_out"] = f32(vit_forward(inp["qkv"], B, N, heads))
    return inp


def window_case(name, fmt):
    """(inputs, reference dict) of a window case; the inputs are shared by the three operand forms."""
    geom = WIN_CASES[name]
    inp = cached(("bwd_in", geom), lambda: build_window(*geom))
    return inp, cached(("bwd_ref", geom, fmt), lambda: window_bwd_ref(inp, *geom, fmt))


def vit_case(B, N, heads, fmt):
    inp = cached(("vit_bwd_in", B, N, heads), lambda: build_vit(B, N, heads))
    return inp, cached(("vit_bwd_ref", B, N, heads, fmt), lambda: vit_bwd_ref(inp, B, N, heads, fmt))


def param_case(ws, pws, nwin, heads):
    inp = cached(("param_in", ws, pws, nwin, heads), lambda: build_params(ws, pws, nwin, heads))
    return inp, cached(("param_ref", ws, pws, nwin, heads), lambda: param_grads_ref(inp, ws, pws, nwin, heads))


def quant(x, fmt):
    """f32 tensor -> its values rounded to the operand format, as f32 (the emulation's fragment rounding; fp16 overflows to inf as f2h_ieee does)."""
    return x if fmt == "f32" else round16(x.double(), fmt).float()
