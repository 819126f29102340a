"""GPU: the three kernels of the Swin-V1 block (csrc/swin1.hip) through include/soccdpt_swin1.h, one launch per test, against float64 with an a-priori bound
on every element (tests/swin1_large_refs.py: references, bounds and inputs; tests/test_swin1_large_cpu.py shows on the CPU that the bounds admit the kernels'
roundings and refuse six kinds of defect).  The smallest shapes that can still go wrong:

  attention   B = 1, res = 24, heads = 2, shift 6 and 0: 2 x 2 windows, so the last-row, last-column and corner masks all occur; B = 2, res = 12, heads = 1:
              one window per sample.  144 keys = four full 32-key tiles + one of 16 real and 16 padded keys.  bf16 / fp16 -> window_attention_sdp_kernel<12, *>
              (also with the fp16 kernel's x3 store), f32 / f16x3 -> window_attention_sdp_f32_kernel<12>.
  pre-norm LN 5 rows (two workgroups of 4 waves, the second with one live wave) at every width the model has: ln_prenorm_kernel<1 / 2 / 3 / 6>.
  merge-LN    (B, R, C) = (1, 4, 192), (2, 6, 384), (1, 2, 768): merge_ln_kernel<192 / 384 / 768>, 4 / 18 / 1 output rows.
"""
import pytest
import torch

from tests import attention_refs as AR
from tests import swin1_large_refs as L

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": 0, "f32": 1, "f16": 2, "x3": 3}


def _out(shape, kind, dev, fill=float("nan")):
    """An output buffer of `kind` ('bf16' / 'f16' / 'f32', or 'x3' = two fp16 words per element) preset with `fill`."""
    n = 1
    for d in shape:
        n *= d
    if kind == "x3":
        return torch.full((n * 2,), fill, dtype=torch.float16, device=dev)
    return torch.full(tuple(shape), fill, dtype=DT[kind], device=dev)


def _report(what, frac):
    print(f"{what}: worst element at {frac:.3f} of its allowance")
    assert frac <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# scaled dot-product window attention
# ---------------------------------------------------------------------------------------------------------------------------------
#          operand format, output kind, SOCCDPT_PREC_*, out_x3
ATTN_MODES = {"bf16": ("bf16", "bf16", 0, False), "f16": ("f16", "f16", 2, False), "f32": ("f32", "f32", 1, False), "f16_x3store": ("f16", "x3", 2, True),
              "f16x3": ("f32", "x3", 3, False)}


@pytest.mark.parametrize("mode", list(ATTN_MODES))
@pytest.mark.parametrize("case", list(L.ATTN_CASES))
def test_window_attention(gpu_device, case, mode):
    from soccdpt_amd.lib import op_swin1_window_attention
    fmt, kind, prec, x3 = ATTN_MODES[mode]
    B, res, ws, shift, heads = L.ATTN_CASES[case]
    inp, ref, bound = L.attention_case(case, fmt)
    out = _out((B * res * res, heads * 32), kind, gpu_device)
    op_swin1_window_attention(inp["qkv"].to(DT[fmt]).to(gpu_device), inp["table"].float().to(gpu_device), out, B, res, ws, shift, heads, precision=prec, out_x3=x3)
    torch.cuda.synchronize()
    _report(f"swin1 attention {case} {mode}", AR.check_output(out.cpu(), kind, ref, bound, f"swin1 attention {case} {mode}"))


# ---------------------------------------------------------------------------------------------------------------------------------
# pre-norm LayerNorm rows, merge-LN
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", L.OUT_FORMATS)
@pytest.mark.parametrize("C", L.LN_WIDTHS)
def test_prenorm_rows(gpu_device, C, kind):
    from soccdpt_amd.lib import op_swin1_ln_rows
    inp, ref, bound = L.prenorm_case(C)
    xf = inp["xf"].float().to(gpu_device)
    before = xf.clone()
    out = _out((L.LN_ROWS, C), kind, gpu_device)
    op_swin1_ln_rows(xf, inp["g"].float().to(gpu_device), inp["beta"].float().to(gpu_device), out, L.LN_ROWS, C, precision=PREC[kind], eps=L.EPS)
    torch.cuda.synchronize()
    assert torch.equal(xf.view(torch.int32), before.view(torch.int32)), "xf is read and not written"
    _report(f"swin1 pre-norm LN C = {C} {kind}", AR.check_output(out.cpu(), kind, ref, bound, f"swin1 pre-norm LN C = {C} {kind}"))


@pytest.mark.parametrize("kind", L.OUT_FORMATS)
@pytest.mark.parametrize("shape", L.MERGE_CASES)
def test_merge_ln(gpu_device, shape, kind):
    from soccdpt_amd.lib import op_swin1_merge_ln
    B, Rr, C = shape
    inp, ref, bound = L.merge_case(*shape)
    xf = inp["xf"].float().to(gpu_device)
    before = xf.clone()
    rows = B * (Rr // 2) ** 2
    out = _out((rows, 4 * C), kind, gpu_device)
    op_swin1_merge_ln(xf, inp["g"].float().to(gpu_device), inp["beta"].float().to(gpu_device), out, B, Rr, C, precision=PREC[kind], eps=L.EPS)
    torch.cuda.synchronize()
    assert torch.equal(xf.view(torch.int32), before.view(torch.int32))
    _report(f"swin1 merge-LN {shape} {kind}", AR.check_output(out.cpu(), kind, ref, bound, f"swin1 merge-LN {shape} {kind}"))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: a refused call has launched nothing
# ---------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def test_refusals_launch_nothing(gpu_device):
    """Every refusal is decided before the first launch (the attention entry's bias arrangement included): the output and the bias scratch keep their sentinel."""
    from soccdpt_amd.lib import load_library
    lib = load_library()
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    dev = gpu_device
    qkv = torch.zeros((576, 192), dtype=torch.float16, device=dev)
    table = torch.zeros((529, 2), dtype=torch.float32, device=dev)
    out = torch.full((576, 64), SENTINEL, dtype=torch.float16, device=dev)
    scratch = torch.full((2 * 25 * 1024,), SENTINEL, dtype=torch.float32, device=dev)
    xf = torch.ones((16, 768), dtype=torch.float32, device=dev)
    g = torch.ones((3072,), dtype=torch.float32, device=dev)
    ln_out = torch.full((16, 3072), SENTINEL, dtype=torch.float32, device=dev)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    # (qkv, table, out, scratch, B, res, ws, shift, heads, precision, out_x3)
    attn = [
        ((None, table, out, scratch, 1, 24, 12, 0, 2, 2, 0), "null"),
        ((qkv, None, out, scratch, 1, 24, 12, 0, 2, 2, 0), "null"),
        ((qkv, table, out, scratch, 0, 24, 12, 0, 2, 2, 0), "positive"),
        ((qkv, table, out, scratch, 1, 0, 12, 0, 2, 2, 0), "positive"),
        ((qkv, table, out, scratch, 1, 24, 12, 0, 0, 2, 0), "positive"),
        ((qkv, table, out, scratch, 1, 24, 24, 0, 2, 2, 0), "window size not instantiated"),
        ((qkv, table, out, scratch, 1, 24, 8, 0, 2, 2, 0), "window size not instantiated"),
        ((qkv, table, out, scratch, 1, 24, 12, 3, 2, 2, 0), "shift must be 0 or ws / 2"),
        ((qkv, table, out, scratch, 1, 24, 12, -6, 2, 2, 0), "shift outside"),
        ((qkv, table, out, scratch, 1, 24, 12, 0, 2, 1, 1), "x3 output form"),
    ]
    for args, word in attn:
        rc = lib.soccdpt_swin1_window_attention(*[P(a) if isinstance(a, torch.Tensor) or a is None else a for a in args], stream)
        msg = lib.soccdpt_last_error(None).decode()
        assert rc != 0 and word in msg, (args[4:], rc, msg)
    # (xf, g, beta, out, format, rows, C, eps) / (xf, g, beta, out, format, B, R, C, eps)
    for rc_args, word in [((P(xf), None, P(g), P(ln_out), 1, 5, 768, 1e-5), "null"), ((P(xf), P(g), P(g), P(ln_out), 1, 0, 768, 1e-5), "rows"),
                          ((P(xf), P(g), P(g), P(ln_out), 1, 5, 1024, 1e-5), "C not instantiated"), ((P(xf), P(g), P(g), P(xf), 1, 5, 768, 1e-5), "alias")]:
        rc = lib.soccdpt_swin1_ln_rows(*rc_args, stream)
        msg = lib.soccdpt_last_error(None).decode()
        assert rc != 0 and word in msg, (rc_args[4:], rc, msg)
    for rc_args, word in [((P(xf), P(g), None, P(ln_out), 1, 1, 4, 768, 1e-5), "null"), ((P(xf), P(g), P(g), P(ln_out), 1, 1, 3, 768, 1e-5), "R must be even"),
                          ((P(xf), P(g), P(g), P(ln_out), 1, 0, 4, 768, 1e-5), "positive"), ((P(xf), P(g), P(g), P(ln_out), 1, 1, -2, 768, 1e-5), "positive"),
                          ((P(xf), P(g), P(g), P(ln_out), 1, 1, 4, 1536, 1e-5), "C not instantiated"), ((P(xf), P(g), P(g), P(ln_out), 1, 1, 4, 96, 1e-5), "C not instantiated")]:
        rc = lib.soccdpt_swin1_merge_ln(*rc_args, stream)
        msg = lib.soccdpt_last_error(None).decode()
        assert rc != 0 and word in msg, (rc_args[4:], rc, msg)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((scratch == SENTINEL).all()) and bool((ln_out == SENTINEL).all())
    assert bool((xf == 1.0).all())
