"""CPU: the references and bounds of tests/attention_bwd_refs.py, without a GPU.
1. The closed forms equal float64 autograd over the same forward (window, ViT, the parameter chain and the clamp at equality).
2. A torch emulation of the kernels' arithmetic -- f32 tensors, 32-token tiles of the walked axis with the online softmax (and, in the 16-bit forms, the online
   delta), 16-bit rounding of every fragment the kernel rounds -- stays within every bound, in every case and operand form; the worst fractions are printed.
3. Every named defect, injected into the emulation, leaves a bound in the case named beside it, in every operand form it exists in.
"""
import math

import pytest
import torch

from tests import attention_bwd_refs as R
from tests import attention_refs as AR

LOG2E = 1.4426950408889634
F = torch.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def _online(s, dp, fmt):
    """Sweep 1 over 32-key tiles: s [H][N][Kpad] f32 -> (m + ln l, delta or None) like the kernel (delta = dacc / l in the 16-bit forms)."""
    H, N, K = s.shape
    m = torch.full((H, N, 1), -3.0e38, dtype=F)
    l = torch.zeros(H, N, 1, dtype=F)
    dacc = torch.zeros(H, N, 1, dtype=F)
    for t in range(K // 32):
        st = s[..., 32 * t: 32 * t + 32]
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        pe = torch.exp2((st - mn) * LOG2E)
        alpha = torch.exp2((m - mn) * LOG2E)
        l = l * alpha + pe.sum(-1, keepdim=True)
        if fmt != "f32":
            dacc = dacc * alpha + (pe * dp[..., 32 * t: 32 * t + 32]).sum(-1, keepdim=True)
        m = mn
    return m, l, (dacc / l if fmt != "f32" else None)


def _tiles_mm(a, b, fmt):
    """a [H][X][Kpad] @ b [H][Kpad][d] accumulated tile by tile over the walked axis, fragments rounded to fmt."""
    out = torch.zeros(a.shape[0], a.shape[1], b.shape[-1], dtype=F)
    for t in range(a.shape[-1] // 32):
        out = out + R.quant(a[..., 32 * t: 32 * t + 32], fmt) @ R.quant(b[:, 32 * t: 32 * t + 32], fmt)
    return out


def _pad(x, dim, n, value=0.0):
    shape = list(x.shape)
    shape[dim] = n - x.shape[dim]
    return torch.cat([x, torch.full(shape, value, dtype=x.dtype)], dim)


def _core(s, a, b, v, dO, O, fmt, defect):
    """s [H][N][N] f32 logits, a / b the score operands -> dS, rowstat, da, db, dv as the kernels compute them (padded keys: logit -1e30, zero operands)."""
    H, N, _ = s.shape
    Kp = -(-N // 32) * 32
    sp = _pad(s, -1, Kp, -1.0e30)
    if defect == "tail32" and Kp != N:          # the padded keys of the last tile take part: logit = 0 + the bias of the clamped key N - 1
        sp[..., N:] = (s[..., N - 1:N] - (a @ b.transpose(-1, -2))[..., N - 1:N]).expand(H, N, Kp - N)
    bp, vp, = _pad(b, 1, Kp), _pad(v, 1, Kp)
    dp = R.quant(dO, fmt) @ R.quant(vp, fmt).transpose(-1, -2)
    m, l, delta = _online(sp, dp, fmt)
    mln = m + torch.log(l)
    if defect == "rowstat_no_lnl":
        mln = m
    if fmt == "f32" or defect == "delta_exact":
        delta = (dO * O).sum(-1, keepdim=True)
    P = torch.exp2((sp - mln) * LOG2E)
    dS = P * (dp - delta)
    da = _tiles_mm(dS, bp, fmt)
    # pass 1: the walked axis is the queries; P and dS are recomputed from the same operands and statistics
    Pq, dSq = _pad(P[..., :N], 1, Kp).transpose(-1, -2), _pad(dS[..., :N], 1, Kp).transpose(-1, -2)
    db = _tiles_mm(dSq, _pad(a, 1, Kp), fmt)
    dv = _tiles_mm(dSq if defect == "dv_with_ds" else Pq, _pad(dO, 1, Kp), fmt)
    return dS[..., :N], torch.cat([mln, delta], -1), da, db, dv


def _norm_bwd(x, g, gs, defect=None):
    nrm = torch.sqrt((x * x).sum(-1, keepdim=True)).clamp(min=1e-12)
    xt = x / nrm
    G = g * gs
    dot = (xt * G).sum(-1, keepdim=True)
    return G / nrm if defect == "dk_no_projection" else (G - xt * dot) / nrm


def emulate_window(inp, B, res, ws, shift, heads, fmt, defect=None):
    C, N, nw = heads * 32, ws * ws, res // ws
    M = B * res * res
    rows = AR.window_rows(B, res, ws, shift, roll_sign=-1 if defect == "roll_reversed" else 1)
    masked = AR.window_masked(res, ws, shift, first=defect == "mask_first")
    bias = inp["table"].float()[AR.bias_index(ws, transposed=defect == "bias_transposed")].permute(2, 0, 1)
    sc = inp["scale"].float().view(-1, 1, 1)
    qkv, dout, attn = inp["qkv"].float(), inp["dout"].float(), inp["attn_out"].float()
    nwin = rows.shape[0]
    dqkv = torch.zeros(M, 3 * C, dtype=F)
    ds = torch.zeros(nwin, heads, N, N, dtype=F)
    rowstat = torch.zeros(nwin, heads, N, 2, dtype=F)
    dscale = torch.zeros(nwin, heads, dtype=torch.float64)
    for w in range(nwin):
        x = qkv[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]
        dO = dout[rows[w]].reshape(N, heads, 32).permute(1, 0, 2)
        O = attn[rows[w]].reshape(N, heads, 32).permute(1, 0, 2)
        qh = q * (sc / torch.sqrt((q * q).sum(-1, keepdim=True)).clamp(min=1e-12))
        kh = k * (1.0 / torch.sqrt((k * k).sum(-1, keepdim=True)).clamp(min=1e-12))
        raw = qh @ kh.transpose(-1, -2)
        b = bias if masked is None else bias + (-100.0 * masked[w % (nw * nw)].float())
        dS, rs, da, db, dv = _core(raw + b, qh, kh, v, dO, O, fmt, defect)
        dq = _norm_bwd(q, da, 1.0 if defect == "dq_no_scale" else sc)
        dk = _norm_bwd(k, db, 1.0, defect)
        for i, val in enumerate((dq, dk, dv)):
            dqkv[rows[w], i * C:(i + 1) * C] = val.permute(1, 0, 2).reshape(N, C)
        ds[w], rowstat[w] = dS, rs
        dsc = (dS * raw).sum((-1, -2))
        dscale[w] = (dsc if defect == "dscale_not_divided" else dsc / sc.view(-1)).double()
    return {"dqkv": dqkv, "ds": ds, "rowstat": rowstat, "dscale": dscale}


def emulate_vit(inp, B, N, heads, fmt):
    E = heads * 64
    x = inp["qkv"].float().reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4).reshape(3, B * heads, N, 64)
    q8, k, v = x[0] * 0.125, x[1], x[2]
    dO = inp["dout"].float().reshape(B, N, heads, 64).permute(0, 2, 1, 3).reshape(B * heads, N, 64)
    O = inp["attn_out"].float().reshape(B, N, heads, 64).permute(0, 2, 1, 3).reshape(B * heads, N, 64)
    _, rs, da, db, dv = _core(q8 @ k.transpose(-1, -2), q8, k, v, dO, O, fmt, None)
    back = lambda t: t.reshape(B, heads, N, 64).permute(0, 2, 1, 3).reshape(B * N, E)      # noqa: E731
    return {"dqkv": torch.cat([back(da * 0.125), back(db), back(dv)], -1), "rowstat": rs.reshape(B, heads, N, 2)}


def emulate_params(inp, ws, pws, nwin, heads, defect=None):
    T2, N = (2 * ws - 1) ** 2, ws * ws
    ds = inp["ds"].float()
    dssum = ds[: nwin - 1 if defect == "window_sum_skips_last" else nwin].sum(0)
    idx = AR.bias_index(ws, transposed=defect == "table_grad_negated").reshape(-1)
    dtable = torch.zeros(T2, heads, dtype=F).index_add_(0, idx, dssum.reshape(heads, N * N).t())
    s = inp["table"].float() * (1.0 / 16.0)
    dt = dtable * 16.0 * s * (1.0 - s)
    c = R.cpb_coords(ws, pws).float()
    w0, b0, w2 = inp["w0"].float(), inp["b0"].float(), inp["w2"].float()
    pre = c[:, :1] * w0[:, 0] + c[:, 1:] * w0[:, 1] + b0
    hid = pre.clamp(min=0)
    dhid = (pre > 0).float() * (dt @ w2)
    ls = inp["ls"].float()
    passes = (ls < R.LN100_F32) if defect == "gate_at_equality" else (ls <= R.LN100_F32)
    dls = torch.where(passes, inp["part"].float().sum((0, 2)) * torch.exp(ls), torch.zeros_like(ls))
    return {"dssum": dssum, "dtable": dtable, "dls": dls, "dw0": dhid.t() @ c, "db0": dhid.sum(0), "dw2": dt.t() @ hid}


# ---------------------------------------------------------------------------------------------------------------------------------
# checks shared with the GPU module's logic
# ---------------------------------------------------------------------------------------------------------------------------------
def window_fractions(got, ref):
    """name -> worst |error| / bound over the outputs of one window launch (no assertion: the caller decides)."""
    out = {}
    for name in ("dqkv", "ds", "rowstat", "dscale"):
        val, bound = ref[name]
        out[name] = float(((got[name].double() - val).abs() / bound.clamp(min=1e-300)).max())
    out["rowsum"] = float((got["ds"].double().sum(-1).abs() / ref["rowsum"].clamp(min=1e-300)).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. closed forms = autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol=1e-9):
    err = float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))
    assert err < tol, (what, err)


@pytest.mark.parametrize("name", ["ws8_shift", "ws12_shift"])
def test_window_closed_forms_equal_float64_autograd(name):
    geom = R.WIN_CASES[name]
    B, res, ws, shift, heads = geom
    inp, ref = R.window_case(name, "f32")
    N, nw, C = ws * ws, res // ws, heads * 32
    qkv = inp["qkv"].clone().requires_grad_(True)
    scale = inp["scale"].clone().requires_grad_(True)
    rows = AR.window_rows(B, res, ws, shift)
    masked = AR.window_masked(res, ws, shift)
    bias = inp["table"][AR.bias_index(ws)].permute(2, 0, 1)
    loss = 0.0
    S = []
    for w in range(rows.shape[0]):
        x = qkv[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        qh = torch.nn.functional.normalize(x[0], dim=-1) * scale.view(-1, 1, 1)
        kh = torch.nn.functional.normalize(x[1], dim=-1)
        s = qh @ kh.transpose(-1, -2) + bias
        if masked is not None:
            s = s - 100.0 * masked[w % (nw * nw)]
        s.retain_grad()
        S.append(s)
        o = (torch.softmax(s, -1) @ x[2]).permute(1, 0, 2).reshape(N, C)
        loss = loss + (o * inp["dout"][rows[w]]).sum()
    loss.backward()
    _close(ref["dqkv"][0], qkv.grad, "dqkv")
    _close(ref["ds"][0], torch.stack([s.grad for s in S]), "dS")
    _close(ref["dscale"][0].sum(0), scale.grad, "dscale")
    _close(ref["rowstat"][0][..., 0], torch.stack([torch.logsumexp(s.detach(), -1) for s in S]), "m + ln l")
    assert float(ref["ds"][0].sum(-1).abs().max()) < 1e-12


def test_vit_closed_forms_equal_float64_autograd():
    B, N, heads = 2, 33, 2
    inp, ref = R.vit_case(B, N, heads, "f32")
    qkv = inp["qkv"].clone().requires_grad_(True)
    (R.vit_forward(qkv, B, N, heads) * inp["dout"]).sum().backward()
    _close(ref["dqkv"][0], qkv.grad, "dqkv")


@pytest.mark.parametrize("ws,pws,nwin,heads", R.PARAM_CASES)
def test_param_chain_equals_float64_autograd(ws, pws, nwin, heads):
    inp, ref = R.param_case(ws, pws, nwin, heads)
    w0, b0, w2 = (inp[k].clone().requires_grad_(True) for k in ("w0", "b0", "w2"))
    table = R.cpb_table_of(w0, b0, w2, ws, pws)
    bias = table[AR.bias_index(ws)].permute(2, 0, 1)                 # [heads][N][N], the same for every window
    (bias[None] * inp["ds"]).sum().backward()
    _close(ref["dw0"][0], w0.grad, "dw0")
    _close(ref["db0"][0], b0.grad, "db0")
    _close(ref["dw2"][0], w2.grad, "dw2")
    ls = inp["ls"].clone().requires_grad_(True)
    dscale = inp["part"].sum((0, 2))
    (torch.clamp(ls, max=R.LN100_F32).exp() * dscale).sum().backward()
    _close(ref["dls"][0], ls.grad, "dls")
    assert bool((inp["ls"] == R.LN100_F32).any())


def test_torch_passes_the_clamp_gradient_at_equality():
    """The reference's torch.clamp(logit_scale, max=log(100)).exp() at logit_scale == float32(log 100), in f32 as the model runs it."""
    ls = torch.tensor([R.LN100_F32], dtype=torch.float32, requires_grad=True)
    torch.clamp(ls, max=math.log(1.0 / 0.01)).exp().sum().backward()
    assert abs(float(ls.grad) - 100.0) < 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the emulation stays within the bounds
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.WIN_CASES))
def test_window_emulation_within_bounds(name, fmt):
    geom = R.WIN_CASES[name]
    inp, ref = R.window_case(name, fmt)
    fr = window_fractions(emulate_window(inp, *geom, fmt), ref)
    print(f"window bwd emulation {fmt} {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("B,N,heads", R.VIT_CASES)
def test_vit_emulation_within_bounds(B, N, heads, fmt):
    inp, ref = R.vit_case(B, N, heads, fmt)
    got = emulate_vit(inp, B, N, heads, fmt)
    for name in ("dqkv", "rowstat"):
        print(f"ViT bwd emulation {fmt} N{N} {name}: {R.check_bound(got[name], *ref[name], name):.3f}")


@pytest.mark.parametrize("ws,pws,nwin,heads", R.PARAM_CASES)
def test_param_emulation_within_bounds(ws, pws, nwin, heads):
    inp, ref = R.param_case(ws, pws, nwin, heads)
    got = emulate_params(inp, ws, pws, nwin, heads)
    for name, (val, bound) in ref.items():
        print(f"param chain emulation ws{ws} {name}: {R.check_bound(got[name], val, bound, name):.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every defect leaves a bound
# ---------------------------------------------------------------------------------------------------------------------------------
WINDOW_DEFECTS = {        # defect -> (the case that refuses it, the outputs of which at least one must leave its bound)
    "roll_reversed": "ws8_shift",
    "mask_first": "ws8_shift",
    "bias_transposed": "ws8",
    "delta_exact": "ws8",                 # 16-bit forms only: refused by the row sums of dS
    "tail32": "ws12_b2",
    "dq_no_scale": "ws12",                # the heads with scale 11.75 and 100
    "dk_no_projection": "ws8",
    "dv_with_ds": "ws8",
    "rowstat_no_lnl": "ws8",
    "dscale_not_divided": "ws12",
}


@pytest.mark.parametrize("defect,fmt", [(d, f) for d in WINDOW_DEFECTS for f in R.FMTS if not (d == "delta_exact" and f == "f32")])      # the f32 form's delta IS dO . O
def test_window_bounds_refuse_the_defect(defect, fmt):
    name = WINDOW_DEFECTS[defect]
    geom = R.WIN_CASES[name]
    inp, ref = R.window_case(name, fmt)
    fr = window_fractions(emulate_window(inp, *geom, fmt, defect), ref)
    print(f"{defect} {fmt} {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in fr.items()))
    assert max(fr.values()) > 1.0, f"{defect} passes every bound of {name} in {fmt}: {fr}"
    if defect == "delta_exact":
        assert fr["rowsum"] > 1.0


@pytest.mark.parametrize("defect,case,output", [("table_grad_negated", (8, 8, 4, 3), "dw2"), ("gate_at_equality", (8, 0, 1, 1), "dls"),
                                                ("window_sum_skips_last", (12, 12, 4, 2), "dssum")])
def test_param_bounds_refuse_the_defect(defect, case, output):
    inp, ref = R.param_case(*case)
    got = emulate_params(inp, *case, defect)
    val, bound = ref[output]
    worst = float(((got[output].double() - val).abs() / bound.clamp(min=1e-300)).max())
    print(f"{defect} {case}: {output} at {worst:.3g} of its allowance")
    assert worst > 1.0
