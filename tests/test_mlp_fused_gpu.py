"""GPU: the fused MLP half-block (csrc/mlp_fused.hip, mlp_ln_kernel) through soccdpt_op_mlp_ln, one launch per call, against the float64 reference and a-priori
per-element bound of tests/mlp_fused_refs.py (derivation there; tests/test_mlp_fused_refs.py holds the same reference against an f32 emulation of the kernel and
shows on the CPU which planted defects it refuses).

tests/test_kernels_gpu.py::test_mlp_ln_fused compares with a torch f32 chain at rtol = atol = 2e-2 / 3e-3, which accepts a tanh-GELU, eps = 1e-6 or an unbiased
variance, and never runs the PatchMerging layout (`merge`), which the network uses on the last block of stage 0.  Here every case of the table (C = 96 / 128 /
192 / 256; bf16 and fp16; M = 1, 63, 64, 65, 130 and the token grids 1 x 2 x 2, 3 x 6 x 4, 2 x 8 x 8; f32 only, separate operand copy, in place, halo, merged copy,
merged copy + halo) runs in both input families, and the special rows (variance exactly 0: xres + beta bit for bit; fp16 hidden units beyond 65504; an fc2
output with mean 50; an all-zero row of x) as cases of their own.  EVERY element of the f32 output is held to its bound; every 16-bit copy must be RN16 of the
launch's own f32 output bit for bit, in the plain, merged and zero-halo layouts.

Per call: x_f32 holds the residual, every other output is 0xFF bytes beforehand -- the halo image too, whose ring must come back 0xFF bit for bit -- and a 4 KB
0xFF guard sits directly behind every operand and every output; afterwards every guard is intact, x_op (unless the call is in place), w1, w2 and every f32
parameter are unchanged, a second call on freshly preset buffers gives the same bits, and an in-place call gives the bits of the call with a separate output.
A HIP error ends the session.  The refusal table (unsupported C, M = 0, f32 / x3 precision, a halo or merged output without a fitting token grid, a merged output
that is NULL or x_op, each required pointer NULL in turn): the call returns an error with a non-empty text and not one byte of an output, halo or guard changes.

Measured on MI355X: over the cases of each (C, format), the largest error / bound of the f32 output and the range of the undecided share (hidden elements whose
16-bit rounding the bound on gelu_fast leaves open; the bound pays for each -- most are elements of the negative tail pre < -3, where h is 1e-4 and smaller and
the absolute error of the erf approximation is a visible fraction of it, and cost next to nothing).  test_report prints the table with -s.

    family   C    format  cases  worst error / bound   undecided share
    dyadic   96   bf16        4                0.032   0.0078 - 0.0415
    dyadic   96   f16         4                0.054   0.0892 - 0.1007
    dyadic   128  bf16        4                0.021   0.0470 - 0.0501
    dyadic   128  f16         3                0.036   0.1045 - 0.1085
    dyadic   192  bf16        3                0.011   0.0563 - 0.0620
    dyadic   192  f16         4                0.041   0.0807 - 0.1200
    dyadic   256  bf16        4                0.007   0.0098 - 0.0726
    dyadic   256  f16         4                0.014   0.1277 - 0.1302
    random   96   bf16        4                0.495   0.0052 - 0.0375
    random   96   f16         4                0.195   0.1662 - 0.1719
    random   128  bf16        4                0.386   0.0492 - 0.0511
    random   128  f16         3                0.083   0.2182 - 0.2227
    random   192  bf16        3                0.004   0.0742 - 0.0773
    random   192  f16         4                0.184   0.0365 - 0.3311
    random   256  bf16        4                0.025   0.0098 - 0.1041
    random   256  f16         4                0.113   0.4084 - 0.4144
    special  96   bf16        2                0.004   0.0366 - 0.0371
    special  96   f16         1                0.028   0.1620 - 0.1620
    special  128  f16         3                0.115   0.2146 - 0.2270
    special  192  bf16        1                0.014   0.0778 - 0.0778
    special  192  f16         1                0.009   0.3249 - 0.3249
"""
import ctypes

import pytest
import torch

from tests import mlp_fused_refs as R
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu

MEASURED = {}          # (family, C, fmt) -> [largest error / bound, smallest undecided share, largest, cases]


@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


_cache = {}


def prepared(name, family):
    """(case, inputs, reference) of a case, computed once and left unchanged."""
    if (name, family) not in _cache:
        case = R.find(name)
        inp = R.build(case, family)
        _cache[name, family] = (case, inp, R.case_reference(case, family, inp))
    return _cache[name, family]


def bits(t):
    return t.contiguous().view(-1).view(torch.uint8).cpu()


def make_buffers(case, inp, dev, out=None):
    """Operands and outputs of one call, each with its guard.  out: the output variant (default the case's)."""
    out = out or case.out
    dt = R.DT[case.fmt]
    M, C = case.rows, case.C
    B, H, W = case.bhw
    b = {k: Buf(inp[k].shape, dt, dev, inp[k]) for k in ("x", "w1", "w2")}
    b.update({k: Buf(inp[k].shape, torch.float32, dev, inp[k]) for k in ("b1", "b2", "g", "beta")})
    b["xf"] = Buf((M, C), torch.float32, dev, inp["xres"])
    b["xop"] = Buf((M // 4, 4 * C) if out in ("merge", "merge_halo") else (M, C), dt, dev) if out in ("copy", "merge", "merge_halo") else None
    b["halo"] = Buf((B, H + 2, W + 2, C), dt, dev) if out in ("halo", "merge_halo") else None
    return b


def sync_or_stop(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_op_mlp_ln ({what}): {e}", returncode=3)


def run(case, inp, dev, out=None):
    """One soccdpt_op_mlp_ln with canaries -> {"xf", "xop", "halo"} on the host."""
    from soccdpt_amd.lib import PREC_BF16, PREC_F16, op_mlp_ln
    out = out or case.out
    b = make_buffers(case, inp, dev, out)
    before = {k: bits(b[k].t) for k in ("x", "w1", "w2", "b1", "b2", "g", "beta")}
    B, H, W = case.bhw
    grid = out in ("halo", "merge", "merge_halo")
    xop_out = b["x"].t if out == "inplace" else (b["xop"].t if b["xop"] is not None else None)
    op_mlp_ln(b["x"].t, b["xf"].t, b["w1"].t, b["b1"].t, b["w2"].t, b["b2"].t, b["g"].t, b["beta"].t, x_op_out=xop_out, halo=b["halo"].t if b["halo"] is not None else None,
              precision=PREC_F16 if case.fmt == "f16" else PREC_BF16, H=H if grid else 0, W=W if grid else 0, merge=out in ("merge", "merge_halo"))
    sync_or_stop(f"{case.name} {out}")
    for k, buf in b.items():
        if buf is not None:
            assert buf.guard_untouched(), f"{case.name}: the guard behind {k} was written"
    for k, v in before.items():
        if not (k == "x" and out == "inplace"):
            assert torch.equal(bits(b[k].t), v), f"{case.name}: operand {k} was written"
    return {"xf": b["xf"].t.cpu(), "xop": b["x"].t.cpu() if out == "inplace" else (b["xop"].t.cpu() if b["xop"] is not None else None),
            "halo": b["halo"].t.cpu() if b["halo"] is not None else None}


def same(a, b, what):
    for k in a:
        assert (a[k] is None) == (b[k] is None)
        if a[k] is not None:
            assert torch.equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


def record(family, case, ratio, undecided):
    m = MEASURED.setdefault((family, case.C, case.fmt), [0.0, 1.0, 0.0, 0])
    m[0], m[1], m[2], m[3] = max(m[0], ratio), min(m[1], undecided), max(m[2], undecided), m[3] + 1


def hold(name, family, dev):
    case, inp, ref = prepared(name, family)
    got = run(case, inp, dev)
    ratio = R.check_outputs(case, inp, ref, got, f"{name} {family}")
    print(f"  {name} {family}: worst error / bound {ratio:.3f}, undecided share {ref['undecided']:.4f}")
    record("special" if case.special else family, case, ratio, ref["undecided"])
    same(got, run(case, inp, dev), f"{name} {family}: a second call on fresh buffers")
    if case.out == "inplace":
        same(got, run(case, inp, dev, out="copy"), f"{name} {family}: in place against a separate output")
    return case, inp, got


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("name", list(R.CASES))
def test_case(dev, name, family):
    case, inp, got = hold(name, family, dev)
    if case.merge:         # the check tells the PatchMerging layout from its neighbour
        with pytest.raises(AssertionError):
            B, H, W = case.bhw
            R.check_copy16(got["xop"], R.merged(got["xf"], B, H, W, swapped=True), case.fmt, "swapped")


@pytest.mark.parametrize("name", list(R.SPECIAL_CASES))
def test_special_rows(dev, name):
    hold(name, "random", dev)


# ---------------- refusals ----------------
POINTERS = ("x", "xf", "w1", "b1", "w2", "b2", "g", "beta")
#           label -> the one thing it changes about raw_call's valid call: C, M, precision, H, W, merge, halo, xop ("buf", None or "x"), null (a pointer's name)
REFUSALS = {
    "C=64": dict(C=64), "C=160": dict(C=160), "C=288": dict(C=288), "M=0": dict(M=0), "precision f32": dict(precision=1), "precision f16x3": dict(precision=3),
    "halo, M % (H W) != 0": dict(H=3, W=2, merge=0), "halo, H = 0": dict(H=0, merge=0), "merge, H odd": dict(M=12, H=3, W=4, halo=False),
    "merge, W odd": dict(M=12, H=4, W=3, halo=False), "merge, x_op_out NULL": dict(xop=None), "merge, x_op_out == x_op": dict(xop="x"),
    **{f"{p} NULL": dict(null=p) for p in POINTERS}}


def raw_call(dev, changes):
    """The valid call here is C = 96, bf16, the 2 x 2 grid (M = 4), merged copy + halo; `changes` alters one thing about it.  -> (rc, error text, buffers, their bytes before)."""
    from soccdpt_amd.lib import load_library
    L = load_library()
    r = dict(C=96, M=4, precision=0, H=2, W=2, merge=1, halo=True, xop="buf", null=None)
    r.update(changes)
    C, M = r["C"], r["M"]
    rows = max(M, 4)                                   # the buffers never shrink below the valid call's
    dt = torch.bfloat16
    b = {"x": Buf((rows, C), dt, dev, R.rnd((rows, C), 1)), "w1": Buf((4 * C, C), dt, dev, R.rnd((4 * C, C), 2, 0.1)), "w2": Buf((C, 4 * C), dt, dev, R.rnd((C, 4 * C), 3, 0.05)),
         "b1": Buf((4 * C,), torch.float32, dev, R.rnd((4 * C,), 4)), "b2": Buf((C,), torch.float32, dev, R.rnd((C,), 5)), "g": Buf((C,), torch.float32, dev, R.rnd((C,), 6)),
         "beta": Buf((C,), torch.float32, dev, R.rnd((C,), 7)), "xf": Buf((rows, C), torch.float32, dev, R.rnd((rows, C), 8)),
         "xop": Buf((rows, C), dt, dev), "halo": Buf((rows, 4, 4, C), dt, dev)}
    before = {k: bits(v.raw) for k, v in b.items()}
    ptr = {k: (None if r["null"] == k else v.ptr()) for k, v in b.items()}
    xop = {"buf": ptr["xop"], None: None, "x": ptr["x"]}[r["xop"]]
    rc = L.soccdpt_op_mlp_ln(ptr["x"], ptr["xf"], ptr["w1"], ptr["b1"], ptr["w2"], ptr["b2"], ptr["g"], ptr["beta"], xop, ptr["halo"] if r["halo"] else None, r["precision"], M, C,
                             r["H"], r["W"], r["merge"], ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    sync_or_stop(str(changes))
    return rc, (L.soccdpt_last_error(None).decode() if rc else ""), b, before


@pytest.mark.parametrize("label", list(REFUSALS))
def test_refusal_writes_nothing(dev, label):
    rc, text, b, before = raw_call(dev, REFUSALS[label])
    print(f"  {label}: rc {rc}, {text!r}")
    assert rc != 0 and text.strip(), f"{label}: accepted (rc {rc}, text {text!r})"
    for k, v in b.items():
        assert torch.equal(bits(v.raw), before[k]), f"{label}: {k} or its guard changed after a refused call"


def test_the_valid_call_of_the_refusal_table_is_accepted(dev):
    """... so that every refusal above is owed to the one thing its row changes: the unchanged call succeeds and writes x_f32, the merged copy and the halo's interior."""
    rc, text, b, before = raw_call(dev, {})
    assert rc == 0, text
    for k, v in b.items():
        assert v.guard_untouched(), k
        assert torch.equal(bits(v.raw), before[k]) == (k not in ("xf", "xop", "halo")), k
    xf = b["xf"].t[:4].cpu()
    assert bool(torch.isfinite(xf).all())
    R.check_copy16(b["xop"].t.cpu().view(-1)[: 4 * 96].view(1, 384), R.merged(xf, 1, 2, 2), "bf16", "merged copy")
    R.check_copy16(R.interior(b["halo"].t[:1].cpu()).contiguous(), xf.reshape(1, 2, 2, 96), "bf16", "halo interior")


def test_report(dev):
    """Prints what the module measured (largest error / bound of the f32 output and the undecided share per family, C and format)."""
    print("\n    family   C    format  cases  worst error / bound   undecided share")
    for (family, C, fmt), (ratio, lo, hi, n) in sorted(MEASURED.items()):
        print(f"    {family:<8} {C:<4} {fmt:<6}  {n:>5}  {ratio:>19.3f}   {lo:.4f} - {hi:.4f}")
