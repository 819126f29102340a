"""GPU: the forward path's non-GEMM launchers (csrc/elementwise.hip, csrc/hybrid.hip), one launcher -- or the forward's composition of two -- at a time
through soccdpt_op_fwd_aux, against the float64 references and a-priori bounds of tests/fwd_aux_refs.py (derivations there).

The whole-network tests reach these kernels at one or two geometries per model and hold them to a network-level relative tolerance sized for bf16 GEMMs; a
bilinear weight off by 1e-3 on the last row, a LayerNorm lane mask wrong at C = 100, merge blocks (1,0) / (0,1) exchanged, a grid-stride loop that drops
its tail or a CPB table built with the wrong window disappear under it.  Here every kernel runs at the smallest shapes at which its edges exist (every
instantiation of the post-norm LayerNorm, all three bilinear kernels, both classifiers, every output format, partial last blocks, one case past every
grid cap) and EVERY element is held to its bound; permutations, selections and single roundings are compared bitwise, operand copies against the launch's
own f32 output (RN16 exactly; fused_refs' x3 rule).

Per call: every output is 0xFF bytes (NaN) beforehand, a 4 KB 0xFF guard sits directly behind every operand and every output; afterwards every guard and
every operand is untouched, the ring of a zero-halo output is still 0xFF (the kernels write the interior only), every written element is finite (except
where the case feeds an overflow on purpose: CVT), and a second call gives the same bits.  A HIP error ends the session.  The kernel a launcher chose comes
back through path_out; test_every_route_was_reached closes the module over them.

Measured on MI355X, per case the element with the largest error / allowance over every output and variant (operand format or out_mode, activation; the count
of variants in parentheses).  For an f32 output the allowance is the bound; for an x3 output the decoded pair against bound + 2^-23 |ref| + 2^-36; for a
16-bit output with no f32 twin the error is the distance from RN16(ref) and the allowance the width of [RN16(ref - bound), RN16(ref + bound)] (equal where the
value is the interval's other end).  Copies beside an f32 output are exact by construction of the check and do not appear.  The LayerNorm allowances are
dominated by the cancellation term of the rows with a spread of 0.01 (and of the shifted rows); the kernels use a fraction of it.  No kernel was found to
be numerically wrong.  Every test prints each figure with -s.

    case (variants)                          worst element (variant)                        error  allowance
    bilinear generic big                     rows 0[0, 286, 520, 2]                       9.5e-05    1.7e-04
    bilinear generic h1                      f32[0, 0, 3, 9]                              1.8e-07    3.9e-06
    bilinear generic identity                f32[0, 0, 0, 0]                              0.0e+00    3.6e-07
    bilinear generic nonint                  bf16 -> halo[0, 2, 5, 7]                     2.0e-03    2.0e-03
    bilinear generic one                     f32[0, 0, 0, 0]                              0.0e+00    3.6e-07
    bilinear generic w1                      f32[0, 1, 0, 10]                             1.8e-07    2.6e-06
    bilinear generic x2                      bf16 -> halo[0, 0, 4, 10]                    3.9e-03    3.9e-03
    bilinear halo8 h1 (3)                    x3 halo[0, 0, 0, 9] (fmt 3)                  6.0e-08    6.0e-07
    bilinear halo8 identity (3)              x3 halo[0, 0, 0, 9] (fmt 3)                  6.0e-08    6.0e-07
    bilinear halo8 nonint (3)                x3 halo[1, 0, 7, 1] (fmt 3)                  9.0e-07    4.2e-06
    bilinear halo8 one (3)                   x3 halo[0, 0, 0, 9] (fmt 3)                  6.0e-08    6.0e-07
    bilinear halo8 w1 (3)                    x3 halo[0, 2, 0, 5] (fmt 3)                  1.5e-07    1.2e-06
    bilinear halo8 x2 (3)                    halo[0, 2, 6, 3] (fmt 1)                     1.2e-04    1.2e-04
    bn_fold 1                                shift[0]                                     6.5e-06    6.7e-05
    bn_fold 100                              scale[8]                                     1.1e-07    4.8e-07
    bn_fold 300                              scale[8]                                     1.1e-07    4.8e-07
    conv_w 1x1 scaled 0 (3)                  bitwise                                            -          -
    conv_w 1x1 scaled 1 (3)                  out[0, 0, 1, 0] (f32)                        2.0e-07    2.5e-07
    conv_w 2x16 scaled 0                     bitwise                                            -          -
    conv_w 2x16 scaled 1                     out[1, 0, 0, 13]                             1.8e-07    2.0e-07
    conv_w 3x5 scaled 0 (3)                  bitwise                                            -          -
    conv_w 3x5 scaled 1 (3)                  out[1, 2, 2, 2] (f32)                        1.1e-07    1.2e-07
    conv_w 64x912 scaled 0 (4)               bitwise                                            -          -
    conv_w 64x912 scaled 1 (4)               out[32, 2, 2, 98] (f32)                      1.2e-07    1.2e-07
    cpb_table (12, 0, 6)                     table[79, 4]                                 3.2e-06    9.9e-04
    cpb_table (12, 16, 3)                    table[218, 0]                                1.6e-06    6.8e-04
    cpb_table (16, 8, 24)                    table[509, 11]                               3.1e-06    8.8e-04
    cpb_table (24, 12, 32)                   table[1006, 26]                              4.4e-06    8.7e-04
    cpb_table (8, 0, 3)                      table[210, 2]                                3.9e-06    1.5e-03
    cpb_table (8, 8, 6)                      table[83, 3]                                 2.9e-06    9.1e-04
    cvt n 1 (3)                              bitwise                                            -          -
    cvt n 1000 (3)                           bitwise                                            -          -
    cvt n 1008                               bitwise                                            -          -
    cvt n 16                                 bitwise                                            -          -
    cvt n 600000 (4)                         bitwise                                            -          -
    gn_relu_maxpool (1, 6, 64, 2) (4)        out[0, 1, 2, 38] (mode 3)                    2.1e-08    7.2e-08
    gn_relu_maxpool (2, 16, 16, 4) (4)       out[0, 5, 1, 4] (mode 3)                     1.2e-07    2.2e-07
    gn_relu_maxpool (2, 2, 16, 2) (4)        out[1, 0, 0, 9] (mode 2)                     1.5e-08    1.2e-07
    gn_relu_maxpool (2, 6, 32, 8) (4)        out[0, 1, 2, 17] (mode 3)                    2.5e-08    6.4e-08
    ln_residual c1000_m7                     xf[4, 157]                                   4.7e-06    3.2e-03
    ln_residual c100_m5                      xf[4, 3]                                     3.0e-06    2.9e-04
    ln_residual c100_shifted                 xf[3, 31]                                    1.0e-05    6.7e-04
    ln_residual c1024_m7                     xf[3, 390]                                   3.8e-08    4.1e-05
    ln_residual c192_m23                     xf[22, 93]                                   3.4e-07    5.7e-05
    ln_residual c256_m1                      xf[0, 14]                                    3.3e-06    1.0e-03
    ln_residual c384_m7                      xf[0, 165]                                   2.2e-06    7.0e-04
    ln_residual c512_m5                      xf[3, 501]                                   4.9e-07    3.7e-04
    ln_residual c576_m5                      xf[4, 233]                                   2.6e-06    1.2e-03
    ln_residual c768_m23                     xf[13, 390]                                  8.2e-08    2.0e-05
    ln_residual c768_shifted                 xf[4, 716]                                   1.6e-06    1.2e-03
    ln_residual c96_m1                       xf[0, 53]                                    3.1e-06    3.3e-04
    ln_residual halo16_c192                  xf[2, 41]                                    4.2e-07    1.1e-04
    ln_residual halo16_c256                  xf[4, 242]                                   4.2e-06    1.1e-03
    ln_residual halof32_c100                 xf[10, 89]                                   1.0e-07    8.6e-06
    ln_residual halof32_c256                 xf[4, 242]                                   4.2e-06    1.1e-03
    ln_residual merge_r2_c96                 xf[4, 63]                                    2.6e-06    1.9e-04
    ln_residual merge_r6_c192_x3             xf[22, 93]                                   3.4e-07    5.7e-05
    ln_residual merge_r6_c256                xf[4, 159]                                   2.3e-06    5.8e-04
    ln_residual rowscale_c512                xf[8, 394]                                   9.3e-07    5.3e-04
    ln_residual rowscale_c96                 xf[4, 47]                                    5.3e-06    4.0e-04
    ln_residual x3halo_f16_c256              xf[4, 242]                                   4.2e-06    1.1e-03
    ln_residual x3halo_f16_c96               xf[4, 63]                                    2.6e-06    1.9e-04
    ln_rows 1 (4)                            xb[0, 93] (mode)                             6.1e-05    6.0e-03
    ln_rows 7 (4)                            xb[4, 672] (mode 0)                          9.8e-04    4.9e-03
    ln_rows 7_shifted (4)                    xb[4, 672] (mode 0)                          9.8e-04    4.9e-03
    logit_scale 1                            out[0]                                       9.2e-07    2.4e-05
    logit_scale 100                          out[32]                                      1.1e-06    4.9e-06
    logit_scale 24                           out[23]                                      1.6e-06    9.1e-06
    logit_scale 3                            out[1]                                       1.2e-06    2.4e-05
    logit_scale 64                           out[32]                                      1.1e-06    4.9e-06
    merge_gather (1, 6, 4, 4)                bitwise                                            -          -
    merge_gather (2, 2, 8, 2)                bitwise                                            -          -
    merge_gather (2, 32, 1056, 4)            bitwise                                            -          -
    merge_gather (2, 6, 24, 2)               bitwise                                            -          -
    patch_embed 1x32x40 (2)                  xf[10, 20] (fmt 0)                           4.3e-07    5.9e-05
    patch_embed 1x32x96 (4)                  xf[1, 77] (fmt 0)                            9.1e-07    1.6e-04
    patch_embed 1x32x96_shifted              xf[62, 28]                                   5.3e-06    1.9e-04
    patch_embed 3x64x128 (2)                 xf[716, 5] (fmt 1)                           7.3e-07    9.0e-05
    patch_embed 8x384x40                     xf[42399, 9]                                 9.2e-07    5.9e-05
    pos_embed_resize (24, 16, 16)            out[145, 15]                                 4.6e-06    4.0e-05
    pos_embed_resize (24, 30, 16)            out[29, 10]                                  2.5e-06    6.5e-06
    pos_embed_resize (4, 4, 8)               out[0, 0]                                    0.0e+00    0.0e+00
    pos_embed_resize (4, 5, 8)               out[2, 0]                                    7.2e-08    7.5e-07
    qkv_bias 1                               bitwise                                            -          -
    qkv_bias 100                             bitwise                                            -          -
    qkv_bias 300                             bitwise                                            -          -
    seg_tail (1, 1, 1) (6)                   seg[0, 0, 0, 0] (fmt 2 sigmoid 1)            3.4e-08    2.7e-07
    seg_tail (1, 1, 3) (6)                   seg[0, 0, 0, 1] (fmt 2 sigmoid 1)            3.8e-08    2.6e-07
    seg_tail (1, 192, 192) (6)               seg[0, 2, 0, 337] (fmt 0 sigmoid 0)          1.1e-05    1.9e-05
    seg_tail (1, 3, 6) (6)                   seg[0, 0, 3, 0] (fmt 2 sigmoid 1)            5.3e-08    3.9e-07
    stem_im2col 16 (4)                       bitwise                                            -          -
    stem_im2col 34 (4)                       bitwise                                            -          -
    vit_tokens_ln (2, 2) (4)                 xb[9, 71] (mode 1)                           9.8e-04    9.8e-04
    vit_tokens_ln (3, 3) (4)                 xb[6, 503] (mode 1)                          2.4e-04    7.3e-04
    ws_conv_w 1x1 (4)                        out[2, 16] (mode 3)                          4.1e-07    7.1e-07
    ws_conv_w 3x3_144 (4)                    out[0, 9] (mode 2)                           1.7e-07    2.5e-07
    ws_conv_w 3x3_288 (4)                    out[1, 199] (mode 3)                         3.0e-07    4.3e-07
    ws_conv_w stem (4)                       out[5, 46] (mode 1)                          7.6e-06    7.6e-06
"""
import pytest
import torch

from tests import fused_refs as FR
from tests import fwd_aux_refs as R
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu

MEASURED = {}          # label -> (error / allowance, where, error, allowance) of the worst element
ROUTES = {"bilinear": set(), "seg_tail": set(), "ln_residual": set()}


# ---------------- harness ----------------
@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


def _out_buf(spec, preset, dev):
    name, shape, fmt = spec
    if isinstance(fmt, torch.dtype):
        dtype, shape_ = fmt, shape
    else:
        dtype, per = R.op_dtype(fmt)
        n = 1
        for s in shape:
            n *= s
        shape_ = (n * per,) if fmt == 3 else shape
    return Buf(shape_, dtype, dev, preset.get(name))


def make_args(call, in_ptrs, out_ptrs):
    from soccdpt_amd.lib import FWD, FwdAuxArgs
    a = FwdAuxArgs(kind=FWD[call.kind] if isinstance(call.kind, str) else call.kind, flags=call.flags)
    for i, v in enumerate(call.dim):
        a.dim[i] = v
    for i, v in enumerate(call.f):
        a.f[i] = v
    for i, p in enumerate(in_ptrs):
        a.inp[i] = p
    for i, p in enumerate(out_ptrs):
        a.out[i] = p
    return a


def _ring_untouched(name, spec, host):
    _, shape, fmt = spec
    if fmt == 3:
        hi, lo = R.x3_words(host, shape)
        words = torch.stack([hi, lo], -1)
    else:
        words = host.view(torch.int16 if host.element_size() == 2 else torch.int32)
    ring = torch.ones(shape[:3], dtype=torch.bool)
    ring[:, 1:-1, 1:-1] = False
    assert bool((words[ring] == -1).all()), f"the ring of the zero-halo output {name} was written"


def _written(spec, host, is_halo):
    """The float values a call wrote (the interior of a halo image), for the finiteness check."""
    _, shape, fmt = spec
    if fmt == 3:
        hi, lo = FR.x3_parts(host, shape)
        v = torch.stack([hi, lo], -1)
    else:
        v = host
    return v[:, 1:-1, 1:-1] if is_halo else v


def run(call, dev):
    """One soccdpt_op_fwd_aux with canaries -> ({output name: host tensor}, path)."""
    from soccdpt_amd.lib import op_fwd_aux
    ins = [None if t is None else Buf(t.shape, t.dtype, dev, t) for t in call.ins]
    outs = [None if o is None else _out_buf(o, call.preset, dev) for o in call.outs]
    a = make_args(call, [b and b.ptr() for b in ins], [b and b.ptr() for b in outs])
    path = op_fwd_aux(a, dev)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_op_fwd_aux ({call.kind} {call.dim} flags {call.flags:#x}): {e}", returncode=3)
    for i, (b, t) in enumerate(zip(ins, call.ins)):
        if b is not None:
            assert b.guard_untouched(), f"the guard behind operand {i} was written"
            assert torch.equal(b.raw[: b.nbytes].cpu(), t.contiguous().view(-1).view(torch.uint8)), f"operand {i} was written"
    got = {}
    for b, o in zip(outs, call.outs):
        if b is None:
            continue
        name = o[0]
        assert b.guard_untouched(), f"the guard behind {name} was written"
        got[name] = b.t.cpu()
        is_halo = name in call.halo
        if is_halo:
            _ring_untouched(name, o, got[name])
        if call.finite and got[name].is_floating_point():
            w = _written(o, got[name], is_halo)
            assert bool(torch.isfinite(w).all()), f"{name} is not finite everywhere it was written: {int((~torch.isfinite(w)).sum())} of {w.numel()} elements"
    return got, path


def run_twice(call, dev):
    got, path = run(call, dev)
    again, path2 = run(call, dev)
    assert path == path2
    for k in got:
        assert torch.equal(got[k].view(-1).view(torch.uint8), again[k].view(-1).view(torch.uint8)), f"{call.kind} {call.dim}: {k} differs between two calls"
    return got, path


def measure(label, what, got64, ref, allow):
    """Record and print the element with the largest error / allowance (the assertion itself is the caller's check)."""
    err = (got64 - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), (err / allow.clamp(min=1e-300)).nan_to_num(float("inf")))
    if ratio.numel():
        i = int(ratio.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        rec = (float(ratio.view(-1)[i]), f"{what}{list(idx)}", float(err.view(-1)[i]), float(allow.expand_as(err).reshape(-1)[i]))
        print(f"  {label} {what}: worst element {list(idx)} error {rec[2]:.2e} allowance {rec[3]:.2e} ({rec[0]:.3f})")
        if label not in MEASURED or rec[0] > MEASURED[label][0]:
            MEASURED[label] = rec
            print(f"MEASURED {label}: {rec[1]} error {rec[2]:.1e} allowance {rec[3]:.1e}")


def exact(label):
    MEASURED[label] = (0.0, "bitwise", 0.0, 0.0)
    print(f"MEASURED {label}: bitwise")


def check_f32(label, what, got, ref, bound):
    measure(label, what, got.double(), ref, bound)
    FR.check_bound(got, ref, bound, f"{label} {what}")


def check_op(label, what, got, fmt, shape, ref, bound):
    """An operand output with no f32 twin against (ref, bound) in its format."""
    if fmt == 2:
        return check_f32(label, what, got, ref, bound)
    if fmt == 3:
        hi, lo = FR.x3_parts(got, shape)
        measure(label, what, hi + lo / 2048.0, ref, bound + 2.0 ** -23 * ref.abs() + 2.0 ** -36)
    else:
        f = R.FMT16[fmt]      # recorded: the distance from RN16(ref) against the width of [RN16(ref - bound), RN16(ref + bound)] (0 of 0 where the interval is one value)
        measure(label, what, got.double(), R.round16(ref, f), R.round16(ref + bound, f) - R.round16(ref - bound, f))
    R.check_op(got, fmt, shape, ref, bound, f"{label} {what}")


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8)), f"{what}: not the same bits"


# ---------------- elementwise.hip ----------------
@pytest.mark.parametrize("case,fmt", R.PATCH_RUNS, ids=lambda v: str(v))
def test_patch_embed(dev, case, fmt):
    inp = R.build_patch(case)
    ref = R.ref_patch(inp)
    call = R.call_patch(case, fmt, inp)
    got, _ = run_twice(call, dev)
    label = f"patch_embed {case} fmt {fmt}"
    same_bits(got["wT"], ref["wT"].float(), "the prepared weight [48][128]")
    check_f32(label, "xf", got["xf"], *ref["xf"])
    if fmt is not None:
        R.check_op(got["xb"], fmt, got["xf"].shape, None, None, f"{label} xb", twin=got["xf"])


@pytest.mark.parametrize("case", list(R.LN_CASES))
def test_ln_residual(dev, case):
    c = R.LN_CASES[case]
    inp = R.build_ln(case)
    call = R.call_ln(case, inp)
    got, path = run_twice(call, dev)
    assert path == c.path, f"{case}: kernel {path:#x}, expected {c.path:#x}"
    ROUTES["ln_residual"].add(path)
    label = f"ln_residual {case}"
    check_f32(label, "xf", got["xf"], *R.ref_ln(case, inp))
    B = c.M // (c.res * c.res) if c.res else 0
    if c.xb:     # the operand copy: RN16 / x3 of the kernel's own xf, for merge in the PatchMerging layout (a permutation: bitwise)
        twin = R.merge_layout(got["xf"], B, c.res) if c.merge else got["xf"]
        R.check_op(got["xb"], c.fmt, twin.shape, None, None, f"{label} xb", twin=twin)
        if c.merge and c.fmt != 3:
            with pytest.raises(AssertionError):
                R.check_op(got["xb"], c.fmt, twin.shape, None, None, "swapped", twin=R.merge_layout_swapped(got["xf"], B, c.res))
    img = got["xf"].reshape(B, c.res, c.res, c.C) if c.halo else None
    if c.halo == "op":
        hfmt = c.fmt if c.halo_fmt is None else c.halo_fmt
        hshape = (B, c.res + 2, c.res + 2, c.C)
        if hfmt == 3:
            hi, lo = FR.x3_parts(got["halo"], hshape)
            FR.check_x3_parts(R.interior(hi), R.interior(lo), img, f"{label} halo")
        else:
            FR.check_copy16(R.interior(got["halo"]).contiguous(), img, R.FMT16[hfmt], f"{label} halo")
    if c.halo == "f32":
        same_bits(R.interior(got["halo_f32"]).contiguous(), img, f"{label} halo_f32")


@pytest.mark.parametrize("shape", R.MERGE_SHAPES, ids=str)
def test_merge_gather(dev, shape):
    inp = R.build_merge(shape)
    got, _ = run_twice(R.call_merge(shape, inp), dev)
    same_bits(got["out"], R.merge_layout(inp["in"], shape[0], shape[1]), f"merge_gather {shape}")
    assert not torch.equal(got["out"], R.merge_layout_swapped(inp["in"], shape[0], shape[1]))
    exact(f"merge_gather {shape}")


@pytest.mark.parametrize("name", list(R.BILINEAR_SHAPES))
def test_bilinear_generic(dev, name):
    shape = R.BILINEAR_SHAPES[name]
    B, h, w, H, W = shape
    label = f"bilinear generic {name}"
    # f32 in -> f32 plain, bf16 plain, f32 halo in one launch
    inp = R.build_bilinear(shape, 12)
    ref, bound = R.ref_bilinear(inp, shape)
    got, path = run_twice(R.call_bilinear(shape, 12, inp, fmt=0, f32_plain=True, op="plain", f32_halo=True), dev)
    ROUTES["bilinear"].add(path)
    assert path == 1
    check_f32(label, "f32", got["out_f32"], ref, bound)
    FR.check_copy16(got["out_op"], got["out_f32"], "bf16", f"{label} bf16 copy")
    same_bits(R.interior(got["out_f32_halo"]).contiguous(), got["out_f32"], f"{label} f32 halo")
    # 16-bit in -> a 16-bit halo alone (C % 8 != 0 keeps it on the generic kernel): no f32 twin
    for f in (0, 1):
        inp16 = R.build_bilinear(shape, 12, in_fmt=f)
        ref16, bound16 = R.ref_bilinear(inp16, shape)
        got, path = run_twice(R.call_bilinear(shape, 12, inp16, in_fmt=f, fmt=f, op="halo"), dev)
        assert path == 1
        check_op(label, f"{R.FMT16[f]} -> halo", R.interior(got["out_op"]).contiguous(), f, ref16.shape, ref16, bound16)
    # 16-bit in -> f32 plain beside a 16-bit plain copy
    got, path = run_twice(R.call_bilinear(shape, 12, inp16, in_fmt=1, fmt=1, f32_plain=True, op="plain"), dev)
    check_f32(label, "f16 -> f32", got["out_f32"], ref16, bound16)
    FR.check_copy16(got["out_op"], got["out_f32"], "f16", f"{label} f16 copy")
    # f32 in -> x3 plain beside f32 plain
    inp = R.build_bilinear(shape, 16)
    ref, bound = R.ref_bilinear(inp, shape)
    got, path = run_twice(R.call_bilinear(shape, 16, inp, fmt=3, f32_plain=True, op="plain"), dev)
    assert path == 1
    check_f32(label, "f32 (C 16)", got["out_f32"], ref, bound)
    FR.check_x3(got["out_op"], ref.shape, got["out_f32"], f"{label} x3 copy")


@pytest.mark.parametrize("fmt", [0, 1, 3])
@pytest.mark.parametrize("name", list(R.BILINEAR_SHAPES))
def test_bilinear_halo8(dev, name, fmt):
    """The 8-channel halo kernels claim "same expression as bilinear_kernel: identical results": their output is the rounding of the generic kernel's f32
    output on the same input, bitwise -- and inside the reference's interval on its own."""
    shape = R.BILINEAR_SHAPES[name]
    C = 16 if fmt == 3 else 8
    label = f"bilinear halo8 {name} fmt {fmt}"
    inp = R.build_bilinear(shape, C)
    ref, bound = R.ref_bilinear(inp, shape)
    got, path = run_twice(R.call_bilinear(shape, C, inp, fmt=fmt, op="halo"), dev)
    ROUTES["bilinear"].add(path)
    assert path == (3 if fmt == 3 else 2)
    gen, gpath = run(R.call_bilinear(shape, C, inp, fmt=fmt, f32_plain=True, op="plain"), dev)
    assert gpath == 1
    hshape = (shape[0], shape[3] + 2, shape[4] + 2, C)
    if fmt == 3:
        hi, lo = (R.interior(t).contiguous() for t in R.x3_words(got["out_op"], hshape))
        ghi, glo = R.x3_words(gen["out_op"], ref.shape)
        same_bits(hi, ghi, f"{label}: hi words against the generic kernel's")
        same_bits(lo, glo, f"{label}: lo words against the generic kernel's")
        vhi, vlo = (R.interior(t) for t in FR.x3_parts(got["out_op"], hshape))
        FR.check_x3_parts(vhi, vlo, gen["out_f32"], f"{label} against the generic f32 output")
        measure(label, "x3 halo", vhi + vlo / 2048.0, ref, bound + 2.0 ** -23 * ref.abs() + 2.0 ** -36)
        R.check_interval16(vhi, ref, bound, "f16", f"{label} hi")
        FR.check_bound(vhi + vlo / 2048.0, ref, bound + 2.0 ** -23 * ref.abs() + 2.0 ** -36, f"{label} decode")
    else:
        inner = R.interior(got["out_op"]).contiguous()
        FR.check_copy16(inner, gen["out_f32"], R.FMT16[fmt], f"{label} against the generic f32 output")
        same_bits(inner, gen["out_op"], f"{label} against the generic 16-bit output")
        check_op(label, "halo", inner, fmt, ref.shape, ref, bound)


def test_bilinear_beyond_the_grid_cap(dev):
    """2,102,500 threads of work for a grid capped at 8192 x 256: the grid-stride loop's second trip."""
    shape = R.BILINEAR_BIG
    B, h, w, H, W, C = shape
    assert B * H * W * (C // 4) > 8192 * 256
    inp = R.build_bilinear(shape, C)
    got, path = run_twice(R.call_bilinear(shape, C, inp, f32_plain=True), dev)
    assert path == 1
    for r0 in range(0, H, 290):
        rows = slice(r0, min(r0 + 290, H))
        ref, bound = R.ref_bilinear(inp, shape, rows=rows)
        check_f32("bilinear generic big", f"rows {r0}", got["out_f32"][:, rows], ref, bound)


@pytest.mark.parametrize("sigmoid", [0, 1])
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("shape", R.SEG_SHAPES, ids=str)
def test_seg_tail(dev, shape, fmt, sigmoid):
    B, h, w = shape
    inp = R.build_seg(shape, fmt)
    got, path = run_twice(R.call_seg(shape, fmt, sigmoid, inp), dev)
    ROUTES["seg_tail"].add(path)
    assert path == (1 if fmt == 2 else 2)
    label = f"seg_tail {shape} fmt {fmt} sigmoid {sigmoid}"
    check_f32(label, "logits", got["tmp"], *R.ref_seg_logits(inp))
    check_f32(label, "seg", got["seg"], *FR.seg_up_act_ref(got["tmp"].double(), B, h, w, sigmoid))      # from the logits the second kernel read


@pytest.mark.parametrize("fmt,n", [(f, n) for f, ns in R.CVT_SIZES.items() for n in ns], ids=str)
def test_cvt(dev, fmt, n):
    inp = R.build_cvt(n, fmt)
    got, _ = run_twice(R.call_cvt(n, fmt, inp), dev)
    out = got["out"]
    if fmt == 3:
        FR.check_x3(out, (n,), inp["in"].float(), f"cvt x3 {n}")
        hi, lo = FR.x3_parts(out, (n,))
        assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all())
    else:
        exp = R.expect_cvt(inp["in"], fmt)
        same = (out.view(torch.int16) == exp.view(torch.int16)) | ((out == 0) & (exp == 0))
        assert bool(same.all()), f"cvt fmt {fmt}: {int((~same).sum())} of {n} words differ; first at {int((~same).nonzero()[0])}"
        x = inp["in"]
        if fmt == 1:
            assert bool(torch.isfinite(out).all()) and (n < 16 or float(out.double().abs().max()) == R.F16_MAX)      # saturates (half16.h f2h<true>)
        if fmt == 5 and n >= 16:
            assert bool((out[x >= 65520.0] == float("inf")).all()) and bool((out[x <= -65520.0] == float("-inf")).all()) and bool(torch.isinf(out).any())
    exact(f"cvt fmt {fmt} n {n}")


@pytest.mark.parametrize("shape,mode,scaled", R.CONV_W_RUNS, ids=str)
def test_conv_w(dev, shape, mode, scaled):
    inp = R.build_conv_w(shape)
    ref, bound = R.ref_conv_w(inp, scaled)
    got, _ = run_twice(R.call_conv_w(shape, mode, scaled, inp), dev)
    fmt = 2 if mode == "f32" else R.CONV_W_MODE[mode][1]
    label = f"conv_w {shape} {mode} scaled {int(scaled)}"
    if scaled:
        check_op(label, "out", got["out"], fmt, ref.shape, ref, bound)
    else:     # a re-layout and at most one rounding: bitwise
        R.check_op(got["out"], fmt, ref.shape, None, None, label, twin=ref.float())
        exact(label)


@pytest.mark.parametrize("C", R.SMALL_SIZES)
def test_bn_fold(dev, C):
    inp = R.build_bn_fold(C)
    ref = R.ref_bn_fold(inp)
    got, _ = run_twice(R.call_bn_fold(C, inp), dev)
    for k in ("scale", "shift"):
        check_f32(f"bn_fold {C}", k, got[k], *ref[k])


@pytest.mark.parametrize("C", R.SMALL_SIZES)
def test_qkv_bias(dev, C):
    inp = R.build_qkv_bias(C)
    got, _ = run_twice(R.call_qkv_bias(C, inp), dev)
    same_bits(got["out"], torch.cat([inp["q"], torch.zeros(C, dtype=torch.float64), inp["v"]]).float(), f"qkv_bias {C}")
    exact(f"qkv_bias {C}")


@pytest.mark.parametrize("H", R.LOGIT_HEADS)
def test_logit_scale(dev, H):
    inp = R.build_logit_scale(H)
    got, _ = run_twice(R.call_logit_scale(H, inp), dev)
    check_f32(f"logit_scale {H}", "out", got["out"], *R.ref_logit_scale(inp))


@pytest.mark.parametrize("case", R.CPB_CASES, ids=str)
def test_cpb_table(dev, case):
    inp = R.build_cpb(case)
    got, _ = run_twice(R.call_cpb(case, inp), dev)
    check_f32(f"cpb_table {case}", "table", got["table"], *R.ref_cpb(case, inp))


# ---------------- hybrid.hip ----------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("case", list(R.WS_CASES))
def test_ws_conv_w(dev, case, mode):
    Cout, Cin, k, Kpad = R.WS_CASES[case]
    fan = Cin * k * k
    inp = R.build_ws(case)
    ref, bound = R.ref_ws(case, inp)
    got, _ = run_twice(R.call_ws(case, mode, inp), dev)
    check_op(f"ws_conv_w {case} mode {mode}", "out", got["out"], mode, ref.shape, ref, bound)
    if mode == 3:
        hi, lo = R.x3_words(got["out"], ref.shape)
        assert bool((hi[:, fan:] == 0).all()) and bool((lo[:, fan:] == 0).all()), "padding columns are not exactly zero"
    else:
        words = got["out"].view(torch.int32 if mode == 2 else torch.int16)
        assert bool((words[:, fan:] == 0).all()), "padding columns are not exactly zero"


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("S", R.IM2COL_SIZES)
def test_stem_im2col(dev, S, mode):
    inp = R.build_im2col(S)
    A = R.ref_im2col(inp)
    got, _ = run_twice(R.call_im2col(S, mode, inp), dev)
    R.check_op(got["A"], mode, A.shape, None, None, f"stem_im2col {S} mode {mode}", twin=A.float())
    exact(f"stem_im2col {S} mode {mode}")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("shape", R.POOL_SHAPES, ids=str)
def test_gn_relu_maxpool(dev, shape, mode):
    inp = R.build_pool(shape)
    ref, bound = R.ref_pool(shape, inp)
    got, _ = run_twice(R.call_pool(shape, mode, inp), dev)
    check_op(f"gn_relu_maxpool {shape} mode {mode}", "out", got["out"], mode, ref.shape, ref, bound)
    if mode == 2:
        assert bool((got["out"][ref == 0] == 0).all()), "a window that is all <= 0 must give exactly 0"


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("case", R.VIT_CASES, ids=str)
def test_vit_tokens_ln(dev, case, mode):
    B, g = case
    ntok = 1 + g * g
    inp = R.build_vit(case)
    got, _ = run_twice(R.call_vit(case, mode, inp), dev)
    same_bits(got["xf"], R.vit_tokens(inp, B, ntok), f"vit_tokens_ln {case}: the token sums")
    ref, bound = R.ln_bound(got["xf"].double(), inp["g"], inp["be"], R.VIT_EPS)
    check_op(f"vit_tokens_ln {case} mode {mode}", "xb", got["xb"], mode, ref.shape, ref, bound)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("case", list(R.LN_ROWS_CASES))
def test_ln_rows(dev, case, mode):
    inp = R.build_ln_rows(case)
    got, _ = run_twice(R.call_ln_rows(case, mode, inp), dev)
    same_bits(got["xf"], inp["xf"].float(), f"ln_rows {case}: xf is read, not written")
    ref, bound = R.ln_bound(inp["xf"], inp["g"], inp["be"], R.VIT_EPS)
    check_op(f"ln_rows {case} mode {mode}", "xb", got["xb"], mode, ref.shape, ref, bound)


@pytest.mark.parametrize("case", R.POS_CASES, ids=str)
def test_pos_embed_resize(dev, case):
    inp = R.build_pos(case)
    got, _ = run_twice(R.call_pos(case, inp), dev)
    check_f32(f"pos_embed_resize {case}", "out", got["out"], *R.ref_pos(case, inp))
    if case[0] == case[1]:
        same_bits(got["out"], inp["pos"].float(), "the same grid: the input itself")


# ---------------- refusals, routes ----------------
def bad_calls():
    """(label, Call, {slot: byte offset}) the entry or the launcher must refuse.  ins / outs hold True for a pointer (a placeholder into real memory) and None
    for NULL; the third element moves a pointer off its 16-byte alignment ("in0" / "out1" -> bytes)."""
    C = R.Call
    T, N = True, None
    fl = R.flags_of
    yield "unknown kind", C(len(R.KINDS), [1]), {}
    yield "negative kind", C(-1, [1]), {}
    yield "patch_embed: C0 > 128", C("patch_embed", [1, 32, 129], ins=[T] * 5, outs=[T, N, T]), {}
    yield "patch_embed: S % 32", C("patch_embed", [1, 48, 96], ins=[T] * 5, outs=[T, N, T]), {}
    yield "patch_embed: null x", C("patch_embed", [1, 32, 96], ins=[N, T, T, T, T], outs=[T, N, T]), {}
    yield "patch_embed: no room for the prepared weight", C("patch_embed", [1, 32, 96], ins=[T] * 5, outs=[T, N, N]), {}
    yield "patch_embed: x3 with C0 % 16", C("patch_embed", [1, 32, 40], fl(0, 3), ins=[T] * 5, outs=[T, T, T]), {}
    yield "ln_residual: merge with odd res", C("ln_residual", [18, 96, 3, 0], fl(2, 0), ins=[T, T, T, N], outs=[T, T, N, N]), {}
    yield "ln_residual: x3 with C % 16", C("ln_residual", [5, 100, 0, 0], fl(1, 3), ins=[T, T, T, N], outs=[T, T, N, N]), {}
    yield "ln_residual: bf16 beside an fp16 halo", C("ln_residual", [8, 96, 2, 0], fl(1, 0, 1), ins=[T, T, T, N], outs=[T, T, T, N]), {}
    yield "ln_residual: bf16 beside an x3 halo", C("ln_residual", [8, 96, 2, 0], fl(1, 0, 3), ins=[T, T, T, N], outs=[T, T, T, N]), {}
    yield "ln_residual: C > 1024", C("ln_residual", [5, 1088, 0, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, T, N, N]), {}
    yield "ln_residual: float4 route, y off by 4 bytes", C("ln_residual", [5, 256, 0, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, T, N, N]), {"in0": 4}
    yield "ln_residual: float4 route, halo off by 8 bytes", C("ln_residual", [8, 512, 2, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, N, T, N]), {"out2": 8}
    yield "ln_residual: null gamma", C("ln_residual", [5, 96, 0, 0], fl(1, 0), ins=[T, N, T, N], outs=[T, T, N, N]), {}
    yield "ln_residual: a halo without the grid's side", C("ln_residual", [8, 96, 0, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, N, T, N]), {}
    yield "ln_residual: row_scale without rows_per_scale", C("ln_residual", [8, 96, 0, 0], fl(1, 0), ins=[T, T, T, T], outs=[T, N, N, N]), {}
    yield "merge_gather: rows of 12 bytes", C("merge_gather", [1, 2, 6, 2], ins=[T], outs=[T]), {}
    yield "merge_gather: rows of 24 bytes", C("merge_gather", [1, 2, 6, 4], ins=[T], outs=[T]), {}
    yield "merge_gather: odd R", C("merge_gather", [1, 3, 8, 2], ins=[T], outs=[T]), {}
    yield "merge_gather: in off by 8 bytes", C("merge_gather", [1, 2, 8, 2], ins=[T], outs=[T]), {"in0": 8}
    yield "merge_gather: out off by 4 bytes", C("merge_gather", [1, 2, 8, 2], ins=[T], outs=[T]), {"out0": 4}
    yield "bilinear: C % 4", C("bilinear", [1, 2, 2, 4, 4, 6], ins=[T], outs=[T, N, N]), {}
    yield "bilinear: x3 from a 16-bit input", C("bilinear", [1, 2, 2, 4, 4, 16], fl(1, 3), ins=[T], outs=[N, T, N]), {}
    yield "bilinear: x3 with C % 16", C("bilinear", [1, 2, 2, 4, 4, 12], fl(0, 3), ins=[T], outs=[N, T, N]), {}
    yield "bilinear: in off by 4 bytes", C("bilinear", [1, 2, 2, 4, 4, 8], ins=[T], outs=[T, N, N]), {"in0": 4}
    yield "bilinear: out_f32 off by 8 bytes", C("bilinear", [1, 2, 2, 4, 4, 8], ins=[T], outs=[T, N, N]), {"out0": 8}
    yield "bilinear: halo off by 8 bytes", C("bilinear", [1, 2, 2, 4, 4, 8], fl(2, 1), ins=[T], outs=[N, T, N]), {"out1": 8}
    yield "bilinear: no output", C("bilinear", [1, 2, 2, 4, 4, 8], ins=[T], outs=[N, N, N]), {}
    yield "seg_tail: features off by 8 bytes", C("seg_tail", [1, 2, 2], fl(0, 1), ins=[T, T, T], outs=[T, T]), {"in0": 8}
    yield "seg_tail: f32 features off by 4 bytes", C("seg_tail", [1, 2, 2], fl(2, 0), ins=[T, T, T], outs=[T, T]), {"in0": 4}
    yield "seg_tail: weights off by 4 bytes beside 16-bit features", C("seg_tail", [1, 2, 2], fl(0, 0), ins=[T, T, T], outs=[T, T]), {"in1": 4}
    yield "cvt: x3 with n % 16", C("cvt", [1000], fl(0, 3), ins=[T], outs=[T]), {}
    yield "cvt: unknown format", C("cvt", [16], fl(0, 2), ins=[T], outs=[T]), {}
    yield "conv_w: x3 with Cin % 16", C("conv_w", [3, 5], fl(0, 3), ins=[T, N], outs=[T]), {}
    yield "logit_scale: no heads", C("logit_scale", [0], ins=[T], outs=[T]), {}
    yield "cpb_table: too many heads for the LDS-resident MLP", C("cpb_table", [8, 0, R.CPB_TOO_MANY_HEADS], ins=[T, T, T], outs=[T]), {}
    yield "ws_conv_w: Kpad below the fan-in", C("ws_conv_w", [4, 3, 7, 144], fl(0, 2), f=(1e-8, 0, 0), ins=[T], outs=[T]), {}
    yield "stem_im2col: odd S", C("stem_im2col", [1, 17], fl(0, 2), ins=[T], outs=[T]), {}
    pool = lambda d: C("gn_relu_maxpool", d, fl(0, 2), ins=[T] * 4, outs=[T])
    yield "gn_relu_maxpool: odd Hi", pool([1, 5, 16, 4]), {}
    yield "gn_relu_maxpool: C % 4", pool([1, 4, 6, 2]), {}
    yield "gn_relu_maxpool: cpg 1", pool([1, 4, 16, 1]), {}
    yield "gn_relu_maxpool: cpg 6", pool([1, 4, 24, 6]), {}
    yield "gn_relu_maxpool: C % cpg", pool([1, 4, 20, 8]), {}
    yield "gn_relu_maxpool: raw off by 4 bytes", pool([1, 4, 16, 4]), {"in0": 4}
    yield "vit_tokens_ln: C != 768", C("vit_tokens_ln", [1, 5, 512], fl(0, 2), f=(1e-6, 0, 0), ins=[T] * 5, outs=[T, T]), {}
    yield "vit_tokens_ln: pos off by 4 bytes", C("vit_tokens_ln", [1, 5, 768], fl(0, 2), f=(1e-6, 0, 0), ins=[T] * 5, outs=[T, T]), {"in2": 4}
    yield "ln_rows: C != 768", C("ln_rows", [3, 1024], fl(0, 2), f=(1e-6, 0, 0), ins=[T, T], outs=[T, T]), {}
    yield "ln_rows: xf off by 8 bytes", C("ln_rows", [3, 768], fl(0, 2), f=(1e-6, 0, 0), ins=[T, T], outs=[T, T]), {"out0": 8}


def test_bad_arguments_launch_nothing(dev):
    """Every refusal, from the entry's plan or from the launcher itself: an error that names the entry, no kernel launched, and the memory every pointer of
    the call points into still 0xFF."""
    from soccdpt_amd.lib import load_library, op_fwd_aux
    L = load_library()
    SLOT = 1 << 16
    arena = Buf((16 * SLOT,), torch.uint8, dev)                    # 0xFF; every pointer of the refused calls points into it
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    n = 0
    for label, call, off in bad_calls():
        ins = [None if t is None else arena.ptr() + SLOT * i + off.get(f"in{i}", 0) for i, t in enumerate(call.ins)]
        outs = [None if t is None else arena.ptr() + SLOT * (8 + i) + off.get(f"out{i}", 0) for i, t in enumerate(call.outs)]
        with pytest.raises(RuntimeError, match="soccdpt_op_fwd_aux"):
            op_fwd_aux(make_args(call, ins, outs), dev)
            pytest.fail(f"accepted: {label}")
        torch.cuda.synchronize()
        assert int(L.soccdpt_launch_counter()) == before, f"{label}: a refused call launched a kernel"
        assert bool((arena.raw == 0xFF).all()), f"{label}: a refused call wrote"
        n += 1
    assert n >= 45
    assert L.soccdpt_op_fwd_aux(None, None, None) == 1
    assert int(L.soccdpt_launch_counter()) == before
    # and good ones launch: one kernel, and the composition's two
    inp = R.build_qkv_bias(100)
    run(R.call_qkv_bias(100, inp), dev)
    assert int(L.soccdpt_launch_counter()) == before + 1
    inp = R.build_patch("1x32x40")
    run(R.call_patch("1x32x40", None, inp), dev)
    assert int(L.soccdpt_launch_counter()) == before + 3


def test_every_route_was_reached():
    """Over the path_out values the tests above recorded: all three bilinear kernels, both classifiers, all nine LayerNorm instantiations."""
    assert ROUTES["bilinear"] == {1, 2, 3}, ROUTES["bilinear"]
    assert ROUTES["seg_tail"] == {1, 2}, ROUTES["seg_tail"]
    want = {R.PATH_LN_SCALAR | v for v in (2, 4, 8, 12, 16)} | {R.PATH_LN_V4 | v for v in (1, 2, 3, 4)}
    assert ROUTES["ln_residual"] == want, sorted(hex(p) for p in want - ROUTES["ln_residual"])
    print()
    for label, rec in sorted(MEASURED.items()):
        print(f"TABLE {label:<48} {rec[1]:<28} {rec[2]:.1e}  {rec[3]:.1e}")
