"""GPU: every forward attention launch (csrc/attention.hip, attention_body.h, attention_qkv.hip, vit_attention.hip) against float64 with an a-priori bound on every
element (tests/attention_refs.py: the references, the bound model and the inputs; tests/test_attention_refs.py shows on the CPU that the bound admits the
kernels' roundings and refuses nine kinds of defect).  One launch per test through soccdpt_amd.lib's op_window_attention / op_window_attention_qkv /
op_vit_attention, compared on the CPU.

Which kernel a case reaches (launch_window_attention, launch_window_attention_f32, launch_vit_attention):
  16-bit windows   ws 8 -> window_attention_kernel<8>; ws 16 -> window_attention_flash_kernel<16, *, 1>; ws 12 -> flash<12, *, 1>; ws 24 -> flash<24, *, 2> below
                   256 (window, head) pairs (ws24_252) and flash<24, *, 1> from 256 on (ws24_256, ws24_256_unshifted).
  f32 / f16x3      ws 8, 12, 16, 24 -> window_attention_f32_flash_kernel<ws>; any other ws (6, 10) -> window_attention_f32_any_kernel;
                   window_attention_f32_kernel<16> / <8> only in a process started with SOCCDPT_ATTN_F32_FLASH16=0 (one child process below).
  fused qkv        window_attention_qkv_kernel<16 / 8> + window_attention_flash_core; the x3 output of the fp16 window kernels is reachable through this entry only
                   (soccdpt_op_window_attention carries no out_x3 argument; the fp16 ViT kernel's x3 store goes through soccdpt_op_vit_attention_out).
  ViT              vit_attention_kernel<bf16 / fp16> (K / V^T resident in LDS, two key halves per query block, query split by B x heads) and
                   vit_attention_f32_kernel<2 / 3>.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_refs as AR

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
PREC = {"bf16": 0, "f32": 1, "f16": 2, "f16x3": 3, "x2w": 5}


def _dev(t, fmt, dev):
    return t.to(DT[fmt]).to(dev)


def _out(M, C, kind, dev):
    """An output buffer of `kind` ('bf16' / 'f16' / 'f32', or 'x3' = two fp16 words per element) preset with NaN."""
    if kind == "x3":
        return torch.full((M * C * 2,), float("nan"), dtype=torch.float16, device=dev)
    return torch.full((M, C), float("nan"), dtype=DT[kind], device=dev)


def launch_window(inp, geom, fmt, dev, x3=False):
    """fmt 'bf16' / 'f16' / 'f32'; x3: the F16X3 mode of the f32 kernels (f32 qkv in, x3 operand out)."""
    from soccdpt_amd.lib import op_window_attention
    B, res, ws, shift, heads = geom
    out = _out(B * res * res, heads * 32, "x3" if x3 else fmt, dev)
    op_window_attention(_dev(inp["qkv"], fmt, dev), inp["table"].float().to(dev), inp["scale"].float().to(dev), out, B, res, ws, shift, heads,
                        precision=PREC["f16x3"] if x3 else PREC[fmt])
    torch.cuda.synchronize()
    return out.cpu()


def launch_qkv(inp, geom, fmt, dev, x3=False):
    from soccdpt_amd.lib import op_window_attention_qkv, x3_encode
    B, res, ws, shift, heads = geom
    act = "bf16" if fmt == "bf16" else "f16"
    w = x3_encode(inp["w"].float().to(dev)) if fmt == "x2w" else _dev(inp["w"], act, dev)
    out = _out(B * res * res, heads * 32, "x3" if x3 else act, dev)
    op_window_attention_qkv(_dev(inp["x"], act, dev), w, inp["bias"].float().to(dev), inp["table"].float().to(dev), inp["scale"].float().to(dev), out, B, res, ws, shift,
                            heads, PREC[fmt], out_x3=x3)
    torch.cuda.synchronize()
    return out.cpu()


def launch_vit(inp, B, N, heads, fmt, dev, x3=False):
    """x3 with fmt 'f32': the F16X3 mode of the f32 kernel; x3 with fmt 'f16': the fp16 kernel's out_x3 store (soccdpt_op_vit_attention_out)."""
    from soccdpt_amd.lib import op_vit_attention
    out = _out(B * N, heads * 64, "x3" if x3 else fmt, dev)
    if x3 and fmt == "f16":
        op_vit_attention(_dev(inp["qkv"], fmt, dev), out, B, N, heads, PREC["f16"], out_x3=True)
        torch.cuda.synchronize()
        return out.cpu()
    op_vit_attention(_dev(inp["qkv"], fmt, dev), out, B, N, heads, PREC["f16x3"] if x3 else PREC[fmt])
    torch.cuda.synchronize()
    return out.cpu()


def _report(what, frac):
    print(f"{what}: worst element at {frac:.3f} of its allowance")
    assert frac <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# windowed cosine attention
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(AR.WIN16_CASES))
def test_window_attention_16bit(gpu_device, name, fmt):
    geom = AR.WIN16_CASES[name]
    B, res, ws, shift, heads = geom
    assert AR.win16_split(B, res, ws, heads) == (2 if name == "ws24_252" else 1)
    inp, ref, bound = AR.window_case("win16", name, fmt)
    _report(f"window attention {fmt} {name} {geom}", AR.check_output(launch_window(inp, geom, fmt, gpu_device), fmt, ref, bound, f"window attention {fmt} {geom}"))


@pytest.mark.parametrize("out", ["f32", "x3"])
@pytest.mark.parametrize("name", list(AR.WINF32_CASES))
def test_window_attention_f32_flash(gpu_device, name, out):
    geom = AR.WINF32_CASES[name]
    inp, ref, bound = AR.window_case("winf32", name, "f32")
    got = launch_window(inp, geom, "f32", gpu_device, x3=out == "x3")
    _report(f"window attention f32 flash -> {out} {name} {geom}", AR.check_output(got, out, ref, bound, f"f32 flash window attention {geom} -> {out}"))


@pytest.mark.parametrize("out", ["f32", "x3"])
@pytest.mark.parametrize("name", list(AR.WINANY_CASES))
def test_window_attention_f32_any_window_size(gpu_device, name, out):
    """window_attention_f32_any_kernel: one thread per query, keys staged 64 at a time (36 keys: one partial block; 100 keys: a full and a partial one)."""
    geom = AR.WINANY_CASES[name]
    inp, ref, bound = AR.window_case("winany", name, "f32")
    got = launch_window(inp, geom, "f32", gpu_device, x3=out == "x3")
    _report(f"window attention f32 any-size -> {out} {name} {geom}", AR.check_output(got, out, ref, bound, f"f32 any-size window attention {geom} -> {out}"))


def test_window_attention_f32_whole_matrix_kernels_in_a_child_process(gpu_device, tmp_path):
    """window_attention_f32_kernel<16> (shifted: the -100 mask of its 16 x 16 form) and <8>: one fresh process with SOCCDPT_ATTN_F32_FLASH16=0 runs both and hands
    the outputs back; a child that fails fails the test."""
    path = str(tmp_path / "whole.npz")
    env = dict(os.environ, SOCCDPT_ATTN_F32_FLASH16="0")
    env.pop("SOCCDPT_ATTN_F32_ANY", None)
    worker = os.path.join(os.path.dirname(__file__), "attention_f32_whole_worker_gpu.py")
    r = subprocess.run([sys.executable, worker, path], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(path)
    for name, geom in AR.WINF32_WHOLE_CASES.items():
        inp, ref, bound = AR.window_case("whole", name, "f32")
        _report(f"window attention f32 whole-matrix kernel {name} {geom}", AR.check_output(torch.from_numpy(got[name]), "f32", ref, bound, f"f32 whole-matrix kernel {geom}"))


@pytest.mark.parametrize("fmt", ["f16", "x2w", "bf16"])
@pytest.mark.parametrize("name", list(AR.QKV_CASES))
def test_window_attention_with_qkv_inside(gpu_device, name, fmt):
    geom = AR.QKV_CASES[name]
    inp, ref, bound = AR.qkv_case(name, fmt)
    act = "bf16" if fmt == "bf16" else "f16"
    _report(f"fused qkv + window attention {fmt} {name} {geom}", AR.check_output(launch_qkv(inp, geom, fmt, gpu_device), act, ref, bound, f"fused qkv attention {fmt} {geom}"))


@pytest.mark.parametrize("name,fmt", [("ws16_shift", "f16"), ("ws8", "x2w")])
def test_window_attention_x3_output_of_the_fp16_kernels(gpu_device, name, fmt):
    """out_x3 of window_attention_flash_core (the store the fp16 window kernels share): the f32 accumulators go out as x3 pairs."""
    geom = AR.QKV_CASES[name]
    inp, ref, bound = AR.qkv_case(name, fmt)
    _report(f"fused qkv + window attention {fmt} -> x3 {name} {geom}", AR.check_output(launch_qkv(inp, geom, fmt, gpu_device, x3=True), "x3", ref, bound, f"fused qkv attention {fmt} {geom} -> x3"))


# ---------------------------------------------------------------------------------------------------------------------------------
# ViT attention
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32", "f16x3"])
@pytest.mark.parametrize("B,N,heads", AR.VIT_CASES)
def test_vit_attention(gpu_device, B, N, heads, fmt):
    """N = 1, 31, 32, 33: one or two key tiles (the second key half of the 16-bit kernel empty or one tile); 577 = 18 tiles + 1 with the largest query split at B = 1;
    608: the LDS-resident form's maximum; B = 22, N = 100: B x heads >= 256, no query split, and the exchange region larger than K / V^T."""
    src = "f32" if fmt == "f16x3" else fmt
    inp, ref, bound = AR.vit_case(B, N, heads, src)
    got = launch_vit(inp, B, N, heads, src, gpu_device, x3=fmt == "f16x3")
    _report(f"ViT attention {fmt} B{B} N{N} heads{heads}", AR.check_output(got, "x3" if fmt == "f16x3" else fmt, ref, bound, f"ViT attention {fmt} {(B, N, heads)}"))


@pytest.mark.parametrize("B,N,heads", AR.VIT_X3_CASES)
def test_vit_attention_x3_output_of_the_fp16_kernel(gpu_device, B, N, heads):
    """vit_attention_kernel<fp16> with out_x3: the f32 accumulators times 1 / l go out as x3 pairs (the proj GEMM operand of a mixed-precision block) -- the
    fp16 kernel's arithmetic and bound, the output held by check_x3_interval instead of the fp16 interval."""
    inp, ref, bound = AR.vit_case(B, N, heads, "f16")
    got = launch_vit(inp, B, N, heads, "f16", gpu_device, x3=True)
    _report(f"ViT attention f16 -> x3 B{B} N{N} heads{heads}", AR.check_output(got, "x3", ref, bound, f"ViT attention f16 -> x3 {(B, N, heads)}"))


def test_vit_attention_x3_output_is_refused_outside_fp16(gpu_device):
    from soccdpt_amd.lib import op_vit_attention
    N, heads = 33, 12
    qkv = torch.zeros(N, 3 * heads * 64, dtype=torch.bfloat16, device=gpu_device)
    out = torch.full((N * heads * 64 * 2,), 3.0, dtype=torch.float16, device=gpu_device)
    with pytest.raises(RuntimeError, match="x3 output form belongs to the fp16 kernel"):
        op_vit_attention(qkv, out, 1, N, heads, PREC["bf16"], out_x3=True)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


def test_vit_attention_refuses_a_sequence_beyond_its_lds(gpu_device):
    from soccdpt_amd.lib import op_vit_attention
    N, heads = 609, 12
    qkv = torch.zeros(N, 3 * heads * 64, dtype=torch.bfloat16, device=gpu_device)
    out = torch.full((N, heads * 64), 3.0, dtype=torch.bfloat16, device=gpu_device)
    with pytest.raises(RuntimeError, match="sequence too long"):
        op_vit_attention(qkv, out, 1, N, heads, PREC["bf16"])
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# bitwise facts
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("what", ["win16_split", "win16_unsplit", "winf32", "winany", "qkv", "vit16", "vitf32"])
def test_a_repeated_launch_gives_identical_bits(gpu_device, what):
    if what.startswith("win"):
        family, name, fmt = {"win16_split": ("win16", "ws24_252", "f16"), "win16_unsplit": ("win16", "ws24_256", "bf16"), "winf32": ("winf32", "ws12_shift", "f32"),
                             "winany": ("winany", "ws10_shift", "f32")}[what]
        geom = {"win16": AR.WIN16_CASES, "winf32": AR.WINF32_CASES, "winany": AR.WINANY_CASES}[family][name]
        inp = AR.window_case(family, name, fmt)[0]
        a, b = (launch_window(inp, geom, fmt, gpu_device) for _ in range(2))
    elif what == "qkv":
        inp = AR.qkv_case("ws16_shift", "x2w")[0]
        a, b = (launch_qkv(inp, AR.QKV_CASES["ws16_shift"], "x2w", gpu_device) for _ in range(2))
    else:
        fmt = "f16" if what == "vit16" else "f32"
        inp = AR.vit_case(1, 577, 12, fmt)[0]
        a, b = (launch_vit(inp, 1, 577, 12, fmt, gpu_device) for _ in range(2))
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_a_batch_of_two_equals_two_batches_of_one(gpu_device, fmt):
    """No sample's result depends on its neighbours or on the grid size: window (2, 16, 8, 0, 3) and ViT B = 2, N = 33."""
    geom = AR.WIN16_CASES["ws8"]
    B, res, ws, shift, heads = geom
    inp = AR.window_case("win16" if fmt != "f32" else "winf32", "ws8", fmt)[0]
    both = launch_window(inp, geom, fmt, gpu_device)
    M = res * res
    for b in range(B):
        one = launch_window(dict(inp, qkv=inp["qkv"][b * M:(b + 1) * M]), (1, res, ws, shift, heads), fmt, gpu_device)
        assert torch.equal(_bits(one), _bits(both[b * M:(b + 1) * M])), f"window sample {b}"
    N, vh = 33, 12
    vin = AR.build_vit(2, N, vh, fmt)
    vboth = launch_vit(vin, 2, N, vh, fmt, gpu_device)
    for b in range(2):
        one = launch_vit({"qkv": vin["qkv"][b * N:(b + 1) * N]}, 1, N, vh, fmt, gpu_device)
        assert torch.equal(_bits(one), _bits(vboth[b * N:(b + 1) * N])), f"ViT sample {b}"


@pytest.mark.parametrize("family,name", [("winf32", "ws16_shift"), ("winf32", "ws12"), ("winany", "ws6_shift")])
def test_f32_kernels_ignore_a_power_of_two_on_a_q_or_k_row(gpu_device, family, name):
    """q^ = q (scale / max(sqrt(sum q^2), 1e-12)) in f32: a factor 2^10 on a row multiplies the sum of squares by 2^20 (exact), its correctly rounded root by 2^10
    (exact), divides the quotient by 2^10 (exact) and cancels in the product -- bit for bit, as long as nothing overflows or reaches the 1e-12 floor.  Both the
    streaming kernel and the one-thread-per-query kernel compute q^ and k^ this way, so the output keeps every bit."""
    geom = {"winf32": AR.WINF32_CASES, "winany": AR.WINANY_CASES}[family][name]
    B, res, ws, shift, heads = geom
    C = heads * 32
    inp = AR.window_case(family, name, "f32")[0]
    rows = AR.window_rows(B, res, ws, shift)
    scaled = inp["qkv"].clone()
    scaled[rows[0, 20], :C] *= 2.0 ** 10
    scaled[rows[0, 21], C:2 * C] *= 2.0 ** 10
    scaled[rows[-1, 22], :C] *= 2.0 ** -10
    a = launch_window(inp, geom, "f32", gpu_device)
    b = launch_window(dict(inp, qkv=scaled), geom, "f32", gpu_device)
    assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: an error before anything is launched, the output untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def _raw_window(dev, prec, qkv, table, scale, out, scratch, B, res, ws, shift, heads):
    from soccdpt_amd.lib import _call, _ptr
    _call("soccdpt_op_window_attention", _ptr(qkv), _ptr(table), _ptr(scale), _ptr(out), _ptr(scratch), B, res, ws, shift, heads, prec, device=dev, guard=False)


BAD_WINDOW = [("shift", -1, "shift outside"), ("shift", 16, "shift outside"), ("shift", 3, "shift must be 0 or ws / 2"), ("B", 0, "must be positive"),
              ("B", -1, "must be positive"), ("res", 0, "must be positive"), ("heads", 0, "must be positive"), ("ws", 0, "must be positive"), ("res", 40, "res % ws"),
              ("qkv", None, "null argument"), ("table", None, "null argument"), ("scale", None, "null argument"), ("out", None, "null argument"),
              ("scratch", None, "null argument")]


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
@pytest.mark.parametrize("field,value,message", BAD_WINDOW, ids=lambda v: str(v))
def test_window_attention_refuses_bad_arguments(gpu_device, fmt, field, value, message):
    """Correctly sized, allocated buffers for the good geometry (1, 32, 16, 8, 3); one argument wrong.  The entry returns non-zero with the message, and neither
    the output nor the bias scratch changes (the refusal comes before launch_attn_bias)."""
    B, res, ws, shift, heads = 1, 32, 16, 8, 3
    M, C = res * res, heads * 32
    a = dict(qkv=torch.zeros(M, 3 * C, dtype=DT[fmt], device=gpu_device), table=torch.zeros((2 * ws - 1) ** 2, heads, device=gpu_device),
             scale=torch.ones(heads, device=gpu_device), out=torch.full((M, C), 3.0, dtype=DT[fmt], device=gpu_device),
             scratch=torch.full((heads * 8 * 8 * 1024,), 5.0, device=gpu_device), B=B, res=res, ws=ws, shift=shift, heads=heads)
    keep_out, keep_scratch = a["out"], a["scratch"]
    a[field] = value
    with pytest.raises(RuntimeError, match=message):
        _raw_window(gpu_device, PREC[fmt], **a)
    torch.cuda.synchronize()
    assert bool((keep_out == 3.0).all()) and bool((keep_scratch == 5.0).all())


@pytest.mark.parametrize("ws,shift,message", [(8, 4, "shifted 8x8 windows are not instantiated"), (4, 0, "window size not instantiated"), (32, 16, "window size not instantiated")])
def test_window_attention_16bit_refuses_what_is_not_instantiated_before_the_bias_launch(gpu_device, ws, shift, message):
    res, heads = 32, 3
    M, C = res * res, heads * 32
    nt = (ws * ws + 31) // 32
    qkv = torch.zeros(M, 3 * C, dtype=torch.float16, device=gpu_device)
    table, scale = torch.zeros((2 * ws - 1) ** 2, heads, device=gpu_device), torch.ones(heads, device=gpu_device)
    out = torch.full((M, C), 3.0, dtype=torch.float16, device=gpu_device)
    scratch = torch.full((heads * nt * nt * 1024,), 5.0, device=gpu_device)
    with pytest.raises(RuntimeError, match=message):
        _raw_window(gpu_device, PREC["f16"], qkv, table, scale, out, scratch, 1, res, ws, shift, heads)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and bool((scratch == 5.0).all())


@pytest.mark.parametrize("field,value,message", [("shift", -1, "shift outside"), ("shift", 16, "shift outside"), ("shift", 4, "shift must be 0 or ws / 2"),
                                                 ("B", 0, "must be positive"), ("res", -32, "must be positive"), ("heads", -3, "must be positive"),
                                                 ("x", None, "null argument"), ("out", None, "null argument")], ids=lambda v: str(v))
def test_window_attention_qkv_refuses_bad_arguments(gpu_device, field, value, message):
    from soccdpt_amd.lib import _call, _ptr
    B, res, ws, shift, heads = 1, 32, 16, 8, 3
    M, C = res * res, heads * 32
    a = dict(x=torch.zeros(M, C, dtype=torch.float16, device=gpu_device), w=torch.zeros(3 * C, C, dtype=torch.float16, device=gpu_device),
             bias=torch.zeros(3 * C, device=gpu_device), table=torch.zeros((2 * ws - 1) ** 2, heads, device=gpu_device), scale=torch.ones(heads, device=gpu_device),
             out=torch.full((M, C), 3.0, dtype=torch.float16, device=gpu_device), scratch=torch.full((heads * 8 * 8 * 1024,), 5.0, device=gpu_device),
             B=B, res=res, ws=ws, shift=shift, heads=heads)
    keep_out, keep_scratch = a["out"], a["scratch"]
    a[field] = value
    with pytest.raises(RuntimeError, match=message):
        _call("soccdpt_op_window_attention_qkv", _ptr(a["x"]), _ptr(a["w"]), _ptr(a["bias"]), _ptr(a["table"]), _ptr(a["scale"]), _ptr(a["out"]), _ptr(a["scratch"]),
              a["B"], a["res"], a["ws"], a["shift"], a["heads"], PREC["f16"], 0, None, device=gpu_device, guard=False)
    torch.cuda.synchronize()
    assert bool((keep_out == 3.0).all()) and bool((keep_scratch == 5.0).all())


@pytest.mark.parametrize("field,value,message", [("qkv", None, "null argument"), ("out", None, "null argument"), ("B", 0, "bad geometry"), ("N", -5, "bad geometry"),
                                                 ("heads", 0, "bad geometry")], ids=lambda v: str(v))
def test_vit_attention_refuses_bad_arguments(gpu_device, field, value, message):
    from soccdpt_amd.lib import _call, _ptr
    N, heads = 33, 12
    a = dict(qkv=torch.zeros(N, 3 * heads * 64, dtype=torch.float16, device=gpu_device), out=torch.full((N, heads * 64), 3.0, dtype=torch.float16, device=gpu_device),
             B=1, N=N, heads=heads)
    keep = a["out"]
    a[field] = value
    with pytest.raises(RuntimeError, match=message):
        _call("soccdpt_op_vit_attention", _ptr(a["qkv"]), _ptr(a["out"]), PREC["f16"], a["B"], a["N"], a["heads"], device=gpu_device, guard=False)
    torch.cuda.synchronize()
    assert bool((keep == 3.0).all())
