"""GPU: every attention backward launch of the training step against float64 with an a-priori bound on every element (tests/attention_bwd_refs.py: the references,
the bound model and the inputs; tests/test_attention_bwd_refs.py shows on the CPU that the bounds admit the kernels' roundings and refuse thirteen kinds of defect).
One launch per test through soccdpt_amd.lib's op_attention_bwd / op_vit_attention_bwd / op_attn_param_grads / op_qv_bias_grad, compared on the CPU.  Every output
lives between two guard zones and is preset to NaN: an element the kernel does not write fails its bound, a write outside the tensor breaks a sentinel.

What a case reaches (csrc/train_attn.hip): attn_bwd_mfma_kernel<ws, pass 0 / 1, OP 0 / 1 / 2> for ws 8, 12, 16, 24 and the f32 / bf16 / fp16 operand forms;
vit_attn_bwd_mfma_kernel<pass, OP>; csrc/train.hip rowsum_kernel, attn_table_grad_kernel, cpb_dt_kernel, cpb_hidden_kernel, cpb_reduce_kernel (mode 0 and 1),
attn_scale_reduce_kernel, qv_bias_grad_kernel.
"""
import pytest
import torch

from tests import attention_bwd_refs as R
from tests import attention_refs as AR

pytestmark = pytest.mark.gpu

PREC = {"bf16": 0, "f32": 1, "f16": 2, "f16x3": 3}
GUARD = 64            # floats on either side: the body stays 256-byte aligned
SENTINEL = 12345.0


class Guarded:
    """A f32 device tensor preset to NaN between two guard zones."""

    def __init__(self, shape, dev, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        self.whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.t = self.whole[GUARD:GUARD + n].view(*shape)
        self.t.fill_(fill)

    def host(self, what):
        w = self.whole.cpu()
        assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()), f"{what}: a guard zone was written"
        return w[GUARD:-GUARD].view(*self.t.shape)


def _report(what, frac):
    print(f"{what}: worst element at {frac:.3f} of its allowance")
    assert frac <= 1.0


def _f(t, dev):
    return t.float().contiguous().to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# windowed cosine attention backward
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_window(inp, geom, fmt, dev):
    from soccdpt_amd.lib import op_attention_bwd, op_attention_bwd_slots
    B, res, ws, shift, heads = geom
    N, nwin, C = ws * ws, B * (res // ws) ** 2, heads * 32
    nslots = op_attention_bwd_slots(ws)
    assert nslots == R.slots(ws)
    out = {"ds": Guarded((nwin, heads, N, N), dev), "rowstat": Guarded((nwin, heads, N, 2), dev), "part": Guarded((nwin, heads, nslots), dev),
           "dqkv": Guarded((B * res * res, 3 * C), dev)}
    op_attention_bwd(_f(inp["qkv"], dev), _f(inp["attn_out"], dev), _f(inp["dout"], dev), _f(inp["table"], dev), _f(inp["scale"], dev), out["ds"].t, out["rowstat"].t,
                     out["part"].t, out["dqkv"].t, B, res, ws, shift, heads, precision=PREC[fmt])
    torch.cuda.synchronize()
    return {k: v.host(f"{k} {fmt} {geom}") for k, v in out.items()}


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", list(R.WIN_CASES))
def test_window_attention_bwd(gpu_device, name, fmt):
    geom = R.WIN_CASES[name]
    ws = geom[2]
    inp, ref = R.window_case(name, fmt)
    got = launch_window(inp, geom, fmt, gpu_device)
    what = f"window attention bwd {fmt} {name} {geom}"
    NT = (ws * ws + 31) // 32
    assert bool((got["part"][..., NT:] == 0).all()), "the dscale slot of a wave that owns no query is exactly 0"
    fr = {k: R.check_bound(got[k], *ref[k], f"{what} {k}") for k in ("dqkv", "ds", "rowstat")}
    fr["dscale"] = R.check_bound(got["part"].double().sum(-1), *ref["dscale"], f"{what} dscale (the sum of the slots)")
    fr["rowsum"] = R.check_bound(got["ds"].double().sum(-1), torch.zeros_like(ref["rowsum"]), ref["rowsum"], f"{what} row sums of dS")
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    _report(what, max(fr.values()))


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("name", ["ws8_shift", "ws12_shift", "ws24_shift"])
def test_window_attention_bwd_second_launch_is_bit_identical(gpu_device, name, fmt):
    geom = R.WIN_CASES[name]
    inp = R.window_case(name, fmt)[0]
    a, b = (launch_window(inp, geom, fmt, gpu_device) for _ in range(2))
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_fp16_overflow_reaches_the_gradients_as_non_finite_values(gpu_device):
    """csrc/half16.h f2h_ieee: 'an overflow must reach GradScaler as inf'.  One dO element of 1e5 in window 1: its fp16 fragment is inf, that window's dk and dv
    hold non-finite values, and every other window stays within its bound."""
    name, fmt = "ws8_shift", "f16"
    geom = R.WIN_CASES[name]
    B, res, ws, shift, heads = geom
    C = heads * 32
    inp, ref = R.window_case(name, fmt)
    rows = AR.window_rows(B, res, ws, shift)
    dout = inp["dout"].clone()
    dout[rows[1, 5], 3] = 1.0e5
    got = launch_window(dict(inp, dout=dout), geom, fmt, gpu_device)
    hit = got["dqkv"][rows[1]]
    assert not bool(torch.isfinite(hit[:, C:2 * C]).all()) and not bool(torch.isfinite(hit[:, 2 * C:]).all()), "the overflow did not reach dk / dv"
    others = torch.cat([rows[w] for w in range(rows.shape[0]) if w != 1])
    wins = [w for w in range(rows.shape[0]) if w != 1]
    fr = [R.check_bound(got["dqkv"][others], ref["dqkv"][0][others], ref["dqkv"][1][others], "dqkv of the other windows"),
          R.check_bound(got["ds"][wins], ref["ds"][0][wins], ref["ds"][1][wins], "dS of the other windows"),
          R.check_bound(got["rowstat"][wins], ref["rowstat"][0][wins], ref["rowstat"][1][wins], "rowstat of the other windows")]
    _report("window attention bwd f16 with one overflowing dO element, the other windows", max(fr))


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT attention backward
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_vit(inp, B, N, heads, fmt, dev):
    from soccdpt_amd.lib import op_vit_attention_bwd
    out = {"rowstat": Guarded((B, heads, N, 2), dev), "dqkv": Guarded((B * N, 3 * heads * 64), dev)}
    op_vit_attention_bwd(_f(inp["qkv"], dev), _f(inp["attn_out"], dev), _f(inp["dout"], dev), out["rowstat"].t, out["dqkv"].t, B, N, heads, precision=PREC[fmt])
    torch.cuda.synchronize()
    return {k: v.host(f"ViT {k} {fmt} {(B, N, heads)}") for k, v in out.items()}


@pytest.mark.parametrize("fmt", R.FMTS)
@pytest.mark.parametrize("B,N,heads", R.VIT_CASES)
def test_vit_attention_bwd(gpu_device, B, N, heads, fmt):
    inp, ref = R.vit_case(B, N, heads, fmt)
    got = launch_vit(inp, B, N, heads, fmt, gpu_device)
    what = f"ViT attention bwd {fmt} B{B} N{N} heads{heads}"
    fr = {k: R.check_bound(got[k], *ref[k], f"{what} {k}") for k in ("dqkv", "rowstat")}
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    _report(what, max(fr.values()))


# ---------------------------------------------------------------------------------------------------------------------------------
# parameter gradients
# ---------------------------------------------------------------------------------------------------------------------------------
def launch_params(inp, ws, pws, nwin, heads, dev, want=("dls", "dw0", "db0", "dw2")):
    """-> (outputs asked for, dS after the call, the untouched-ness of what was not asked for is asserted here)."""
    from soccdpt_amd.lib import op_attn_param_grads
    T2 = (2 * ws - 1) ** 2
    N = ws * ws
    ds = Guarded((nwin, heads, N, N), dev)
    ds.t.copy_(_f(inp["ds"], dev))
    outs = {"dls": Guarded((heads,), dev), "dw0": Guarded((512, 2), dev), "db0": Guarded((512,), dev), "dw2": Guarded((heads, 512), dev)}
    scratch = {"dtable": Guarded((T2, heads), dev), "dt": Guarded((T2, heads), dev), "hid": Guarded((2 * T2 * 512,), dev)}
    arg = {k: (v.t if k in want else None) for k, v in outs.items()}
    op_attn_param_grads(ds.t, _f(inp["part"], dev), _f(inp["table"], dev), _f(inp["ls"], dev), _f(inp["w0"], dev), _f(inp["b0"], dev), _f(inp["w2"], dev),
                        scratch["dtable"].t, scratch["dt"].t, scratch["hid"].t, arg["dls"], arg["dw0"], arg["db0"], arg["dw2"], nwin, ws, pws, heads)
    torch.cuda.synchronize()
    host = {k: v.host(k) for k, v in outs.items()}
    for k, v in host.items():
        if k not in want:
            assert bool(torch.isnan(v).all()), f"{k} was not asked for and was written"
    sc = {k: v.host(k) for k, v in scratch.items()}
    return {k: host[k] for k in want}, ds.host("dS"), sc


@pytest.mark.parametrize("ws,pws,nwin,heads", R.PARAM_CASES)
def test_attn_param_grads(gpu_device, ws, pws, nwin, heads):
    """ls holds float32(ln 100) exactly on head 0 (and 2.0, 5.0 on the next two): torch.clamp passes the gradient at equality, and so must the kernel."""
    inp, ref = R.param_case(ws, pws, nwin, heads)
    assert float(inp["ls"][0]) == R.LN100_F32
    got, ds, sc = launch_params(inp, ws, pws, nwin, heads, gpu_device)
    what = f"attn_param_grads ws{ws} pws{pws} nwin{nwin} heads{heads}"
    fr = {k: R.check_bound(got[k], *ref[k], f"{what} {k}") for k in ("dls", "dw0", "db0", "dw2")}
    fr["dssum"] = R.check_bound(ds[0], *ref["dssum"], f"{what} dS slab 0 = the window sum")
    fr["dtable"] = R.check_bound(sc["dtable"], *ref["dtable"], f"{what} dtable")
    assert torch.equal(_bits(ds[1:]), _bits(inp["ds"][1:].float())), "the other slabs of dS are only read"
    print(f"{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in fr.items()))
    _report(what, max(fr.values()))


@pytest.mark.parametrize("want", [("dls",), ("dw2",), ("dw0",)], ids=lambda w: "+".join(w))
def test_attn_param_grads_writes_only_what_was_asked(gpu_device, want):
    case = (8, 8, 4, 3)
    inp, ref = R.param_case(*case)
    got, ds, sc = launch_params(inp, *case, gpu_device, want=want)
    for k in want:
        _report(f"attn_param_grads {case} {k} alone", R.check_bound(got[k], *ref[k], k))
    if want == ("dls",):          # no table gradient: dS and the scratch are not touched
        assert torch.equal(_bits(ds), _bits(inp["ds"].float()))
        assert all(bool(torch.isnan(v).all()) for v in sc.values())


@pytest.mark.parametrize("C", [96, 1536])
@pytest.mark.parametrize("want", [("dq", "dv"), ("dq",), ("dv",)], ids=lambda w: "+".join(w))
def test_qv_bias_grad_is_an_exact_copy(gpu_device, C, want):
    from soccdpt_amd.lib import op_qv_bias_grad
    g = torch.Generator().manual_seed(C)
    src = torch.randn(3 * C, generator=g)
    outs = {"dq": Guarded((C,), gpu_device), "dv": Guarded((C,), gpu_device)}
    op_qv_bias_grad(src.to(gpu_device), outs["dq"].t if "dq" in want else None, outs["dv"].t if "dv" in want else None, C)
    torch.cuda.synchronize()
    host = {k: v.host(k) for k, v in outs.items()}
    for k, lo in (("dq", 0), ("dv", 2 * C)):
        if k in want:
            assert torch.equal(_bits(host[k]), _bits(src[lo:lo + C])), k
        else:
            assert bool(torch.isnan(host[k]).all()), k


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: an error before anything is launched, every output keeps its sentinel
# ---------------------------------------------------------------------------------------------------------------------------------
WINDOW_PTRS = ("qkv", "attn_out", "dout", "table", "scale", "ds", "rowstat", "part", "dqkv")
BAD_WINDOW = [(p, None, "null argument") for p in WINDOW_PTRS] + [
    ("B", 0, "must be positive"), ("B", -1, "must be positive"), ("res", 0, "must be positive"), ("res", -16, "must be positive"), ("heads", 0, "must be positive"),
    ("heads", -2, "must be positive"), ("ws", 0, "must be positive"), ("res", 20, "res % ws"), ("shift", 3, "shift must be 0 or ws / 2"), ("shift", -1, "shift outside"),
    ("shift", 8, "shift outside"), ("ws,shift", (4, 2), "no instantiation for this window size"), ("prec", PREC["f16x3"], "products are f32, bf16 or fp16"),
    ("prec", 7, "unknown precision")]


@pytest.mark.parametrize("field,value,message", BAD_WINDOW, ids=lambda v: str(v))
def test_window_attention_bwd_refuses_bad_arguments(gpu_device, field, value, message):
    """Correctly sized buffers for the good geometry (1, 16, 8, 4, 2); one argument wrong."""
    from soccdpt_amd.lib import _call, _ptr
    B, res, ws, shift, heads = 1, 16, 8, 4, 2
    N, nwin, C, M = ws * ws, 4, heads * 32, res * res
    dev = gpu_device
    outs = {"ds": Guarded((nwin, heads, N, N), dev, 3.0), "rowstat": Guarded((nwin, heads, N, 2), dev, 3.0), "part": Guarded((nwin, heads, 4), dev, 3.0),
            "dqkv": Guarded((M, 3 * C), dev, 3.0)}
    a = dict(qkv=torch.zeros(M, 3 * C, device=dev), attn_out=torch.zeros(M, C, device=dev), dout=torch.zeros(M, C, device=dev),
             table=torch.zeros((2 * ws - 1) ** 2, heads, device=dev), scale=torch.ones(heads, device=dev), **{k: v.t for k, v in outs.items()},
             B=B, res=res, ws=ws, shift=shift, heads=heads, prec=PREC["f32"])
    a.update(zip(field.split(","), value) if "," in field else [(field, value)])
    with pytest.raises(RuntimeError, match="soccdpt_op_attention_bwd.*" + message):
        _call("soccdpt_op_attention_bwd", *(_ptr(a[p]) for p in WINDOW_PTRS), a["B"], a["res"], a["ws"], a["shift"], a["heads"], a["prec"], device=dev, guard=False)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v.host(k) == 3.0).all()), k


VIT_PTRS = ("qkv", "attn_out", "dout", "rowstat", "dqkv")
BAD_VIT = [(p, None, "null argument") for p in VIT_PTRS] + [("B", 0, "must be positive"), ("N", 0, "must be positive"), ("N", -33, "must be positive"),
                                                              ("heads", 0, "must be positive"), ("prec", PREC["f16x3"], "products are f32, bf16 or fp16"),
                                                              ("prec", -1, "unknown precision")]


@pytest.mark.parametrize("field,value,message", BAD_VIT, ids=lambda v: str(v))
def test_vit_attention_bwd_refuses_bad_arguments(gpu_device, field, value, message):
    from soccdpt_amd.lib import _call, _ptr
    B, N, heads = 1, 33, 2
    E = heads * 64
    dev = gpu_device
    outs = {"rowstat": Guarded((B, heads, N, 2), dev, 3.0), "dqkv": Guarded((N, 3 * E), dev, 3.0)}
    a = dict(qkv=torch.zeros(N, 3 * E, device=dev), attn_out=torch.zeros(N, E, device=dev), dout=torch.zeros(N, E, device=dev), **{k: v.t for k, v in outs.items()},
             B=B, N=N, heads=heads, prec=PREC["f32"])
    a[field] = value
    with pytest.raises(RuntimeError, match="soccdpt_op_vit_attention_bwd.*" + message):
        _call("soccdpt_op_vit_attention_bwd", *(_ptr(a[p]) for p in VIT_PTRS), a["B"], a["N"], a["heads"], a["prec"], device=dev, guard=False)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v.host(k) == 3.0).all()), k


BAD_PARAMS = [("nwin", 0, "must be positive"), ("ws", 10, "no attention backward is instantiated"), ("heads", 0, "must be positive"), ("pws", -1, "pws >= 0"),
              ("pws", 1, "window size - 1"), ("dls+dw0+db0+dw2", None, "no output requested"), ("part", None, "dls needs"), ("ls", None, "dls needs"),
              ("ds", None, "table gradients need"), ("hid", None, "table gradients need"), ("w2", None, "table gradients need")]


@pytest.mark.parametrize("field,value,message", BAD_PARAMS, ids=lambda v: str(v))
def test_attn_param_grads_refuses_bad_arguments(gpu_device, field, value, message):
    from soccdpt_amd.lib import _call, _ptr
    ws, pws, nwin, heads = 8, 8, 2, 2
    T2, N, dev = (2 * ws - 1) ** 2, ws * ws, gpu_device
    outs = {"ds": Guarded((nwin, heads, N, N), dev, 3.0), "dtable": Guarded((T2, heads), dev, 3.0), "dt": Guarded((T2, heads), dev, 3.0),
            "hid": Guarded((2 * T2 * 512,), dev, 3.0), "dls": Guarded((heads,), dev, 3.0), "dw0": Guarded((512, 2), dev, 3.0), "db0": Guarded((512,), dev, 3.0),
            "dw2": Guarded((heads, 512), dev, 3.0)}
    a = dict(part=torch.zeros(nwin, heads, R.slots(ws), device=dev), table=torch.ones(T2, heads, device=dev), ls=torch.zeros(heads, device=dev),
             w0=torch.zeros(512, 2, device=dev), b0=torch.zeros(512, device=dev), w2=torch.zeros(heads, 512, device=dev), **{k: v.t for k, v in outs.items()},
             nwin=nwin, ws=ws, pws=pws, heads=heads)
    a.update((f, value) for f in field.split("+"))
    with pytest.raises(RuntimeError, match="soccdpt_op_attn_param_grads.*" + message):
        _call("soccdpt_op_attn_param_grads", *(_ptr(a[p]) for p in ("ds", "part", "table", "ls", "w0", "b0", "w2", "dtable", "dt", "hid", "dls", "dw0", "db0", "dw2")),
              a["nwin"], a["ws"], a["pws"], a["heads"], device=dev, guard=False)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v.host(k) == 3.0).all()), k


@pytest.mark.parametrize("field,value,message", [("src", None, "null argument"), ("dq+dv", None, "null argument"), ("C", 0, "C must be positive")], ids=lambda v: str(v))
def test_qv_bias_grad_refuses_bad_arguments(gpu_device, field, value, message):
    from soccdpt_amd.lib import _call, _ptr
    C, dev = 96, gpu_device
    outs = {"dq": Guarded((C,), dev, 3.0), "dv": Guarded((C,), dev, 3.0)}
    a = dict(src=torch.zeros(3 * C, device=dev), dq=outs["dq"].t, dv=outs["dv"].t, C=C)
    a.update((f, value) for f in field.split("+"))
    with pytest.raises(RuntimeError, match="soccdpt_op_qv_bias_grad.*" + message):
        _call("soccdpt_op_qv_bias_grad", _ptr(a["src"]), _ptr(a["dq"]), _ptr(a["dv"]), a["C"], device=dev, guard=False)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v.host(k) == 3.0).all()), k
