"""GPU: the training step's non-GEMM backward kernels (csrc/train.hip, csrc/train_hybrid.hip), one launcher -- or the step's composition of a few -- at a
time through soccdpt_op_train_aux, against the float64 references of tests/train_aux_refs.py.

The whole-step tests reach these kernels at one batch size and one geometry per model and hold them to a per-parameter relative L2 with a median; a wrong
border row of one resampling level or one mis-summed chunk disappears under it.  Here every kernel runs at the smallest shapes at which its edges exist
(partial last blocks, more chunks than rows, chunk counts clamped to 1, the grid-stride loop, both channel-vector widths, every optional argument on and
off, in-place forms) and is measured by relative L2 on the whole tensor AND on the slices of train_aux_refs.slices: first / last row, the last partial
4-row block (LayerNorm), every 64-column block of a reduction, border ring / interior per image (bilinear, max-pool), every sample (GroupNorm) or row
block (BatchNorm).  Bound: max(3 x the error of torch's own CPU f32 evaluation of the same operation on the same inputs, 2e-6), the yardstick computed
here, per slice.  No element is excluded: the input builders keep every recomputed ReLU / clamp decision 1e-3 away from zero (checked on the CPU by
tests/test_train_aux_refs.py).  Max-pool is checked by its returned argmax bytes: the byte is the float64 argmax where the window's two best values
are more than 1e-4 apart (or the window is all zero: first position), elsewhere the value at the byte is within 1e-5 of the maximum; dA equals the
scatter of dpool by THOSE bytes up to the rounding of at most four additions.  Permutations and scalings (merge_scatter, scale_rows, drop_path_fill)
are compared bitwise.

Per call: the scratch is 0xFF bytes and every output 0xFF (NaN) beforehand, a 4 KB 0xFF guard sits directly behind the scratch, every operand and every
output; afterwards every output is finite, every guard and every operand is untouched, and a second call gives the same bits.  A HIP error ends the
session.

The compositions are the step's: LayerNorm = tr_ln_bwd + tr_colsum2; BatchNorm forward = tr_bn_stats + tr_bn_relu_dropout_fwd, backward =
tr_bn_relu_dropout_bwd_pre + tr_bn_xhat + tr_colsum (dbeta) + tr_colsum (dgamma) + tr_bn_bwd (train_step.cpp uses two single column sums there, not
colsum2); depth tail = forward + backward.  LayerNorm's `dy = dout` form runs without parameter gradients: their column sums read dout after dy is
written, so the entry refuses the combination (no call site of the step uses it).

Measured on MI355X: per case the slice with the largest error / bound over every output, variant (b, accumulate, add, activation) and slice, with
torch's CPU f32 error on that slice and the bound it gives.  3 x torch stays under the 2e-6 floor except where the inputs themselves cancel
(LayerNorm rows of mean 50 / spread 0.5, BatchNorm over x = 30 + 0.1 randn or over two rows): there the kernels stay within 1.3 x torch's own error.
No case needs the factor 3 above the floor.  Every test prints each figure with -s.

    case                                  worst slice          kernel  torch f32    bound
    ln_bwd 1x96                           dy.whole             7.0e-08    6.8e-08  2.0e-06
    ln_bwd 5x96                           dy.row.last          9.5e-08    1.0e-07  2.0e-06
    ln_bwd 259x192                        dgamma.cols.0        1.0e-07    1.4e-07  2.0e-06
    ln_bwd 64x100                         dgamma.cols.64       9.4e-08    1.3e-07  2.0e-06
    ln_bwd 33x24                          dbeta.whole          8.3e-08    8.1e-08  2.0e-06
    ln_bwd 130x768                        dgamma.cols.64       1.1e-07    1.4e-07  2.0e-06
    ln_bwd 7x1024                         dgamma.cols.128      9.5e-08    6.2e-08  2.0e-06
    ln_bwd 130x768_shifted                dgamma.cols.704      5.6e-06    4.3e-06  1.3e-05
    ln_bwd 259x192_alias                  dy.whole             5.9e-08    6.9e-08  2.0e-06
    ln_bwd 33x24_bare                     dy.row.first         7.7e-08    1.4e-07  2.0e-06
    colsum (1, 64)                        out.whole            3.4e-08    3.4e-08  2.0e-06
    colsum (15, 1)                        out.whole            7.9e-08    7.9e-08  2.0e-06
    colsum (16, 63)                       out.whole            6.5e-08    8.3e-08  2.0e-06
    colsum (17, 65)                       out.cols.64          8.4e-07    3.4e-07  2.0e-06
    colsum (1000, 96)                     out.cols.64          1.0e-07    1.2e-07  2.0e-06
    colsum (4099, 288)                    out.cols.64          1.2e-07    1.3e-07  2.0e-06
    colsum (2063, 2304)                   out.cols.256         1.4e-07    1.5e-07  2.0e-06
    colsum2 (1, 64)                       out_ab.whole         2.7e-08    2.7e-08  2.0e-06
    colsum2 (15, 1)                       out_ab.whole         8.5e-08    6.8e-08  2.0e-06
    colsum2 (16, 63)                      out_ab.whole         6.6e-08    6.5e-08  2.0e-06
    colsum2 (17, 65)                      out_ab.cols.64       3.2e-07    5.7e-08  2.0e-06
    colsum2 (1000, 96)                    out_a.cols.64        9.7e-08    1.4e-07  2.0e-06
    colsum2 (4099, 288)                   out_a.cols.128       1.2e-07    1.6e-07  2.0e-06
    colsum2 (2063, 2304)                  out_ab.cols.1408     1.3e-07    1.4e-07  2.0e-06
    bn_fwd 2x5                            y.row.last           4.0e-07    8.3e-07  2.5e-06
    bn_bwd 2x5                            dx.row.last          1.1e-05    1.2e-05  3.7e-05
    bn_fwd 100x128                        y.row.first          7.0e-08    5.7e-08  2.0e-06
    bn_bwd 100x128                        dgamma.cols.64       9.6e-08    6.0e-08  2.0e-06
    bn_fwd 128x64                         y.row.first          5.9e-08    6.8e-08  2.0e-06
    bn_bwd 128x64                         dgamma.whole         9.5e-08    7.0e-08  2.0e-06
    bn_fwd 129x128                        y.rows.part1         5.2e-08    5.1e-08  2.0e-06
    bn_bwd 129x128                        dgamma.cols.0        9.1e-08    7.7e-08  2.0e-06
    bn_fwd 4099x128                       rmean.cols.0         5.9e-08    5.9e-08  2.0e-06
    bn_bwd 4099x128                       dgamma.cols.64       1.3e-07    2.4e-07  2.0e-06
    bn_fwd 3072x200                       rmean.cols.64        5.8e-08    5.8e-08  2.0e-06
    bn_bwd 3072x200                       dgamma.cols.128      1.3e-07    2.0e-07  2.0e-06
    bn_fwd 129x128_shifted                y.row.last           5.4e-06    7.8e-06  2.3e-05
    bn_bwd 129x128_shifted                dgamma.cols.64       5.3e-06    5.4e-06  1.6e-05
    bn_fwd 8209x130                       rmean.cols.128       7.0e-08    7.0e-08  2.0e-06
    bn_bwd 8209x130                       dbeta.cols.64        1.1e-07    2.9e-07  2.0e-06
    bn_fwd dropout                        y.row.first          7.3e-08    8.8e-08  2.0e-06
    bn_bwd dropout                        dgamma.cols.64       1.5e-07    1.8e-07  2.0e-06
    gn_bwd 1x9x64                         dx.row.first         8.4e-08    8.7e-08  2.0e-06
    gn_bwd 2x49x256                       dgamma.cols.64       1.1e-07    1.0e-07  2.0e-06
    gn_bwd 4x36x1024                      dgamma.cols.576      9.9e-08    1.1e-07  2.0e-06
    gn_bwd 5x577x512                      dgamma.cols.320      1.2e-07    2.0e-07  2.0e-06
    gn_bwd 3x100x96                       dbeta.cols.0         9.9e-08    9.0e-08  2.0e-06
    gn_bwd 1x16x32                        dgamma.whole         9.5e-08    8.8e-08  2.0e-06
    gn_bwd 8x16x1024                      dgamma.cols.192      9.7e-08    9.5e-08  2.0e-06
    gn_bwd 40x4x1024                      dgamma.cols.896      1.5e-07    1.7e-07  2.0e-06
    gn_bwd 5x577x1024                     dbeta.cols.320       1.3e-07    1.8e-07  2.0e-06
    gn_bwd 2x49x256_alias                 dgamma.cols.64       1.1e-07    1.0e-07  2.0e-06
    gn_bwd 3x100x96_no_dx                 dbeta.cols.0         9.9e-08    9.0e-08  2.0e-06
    gn_bwd 5x577x512_no_param             dx.sample4           5.2e-08    6.5e-08  2.0e-06
    ws_bwd stem                           dw.sample7           7.3e-08    7.4e-08  2.0e-06
    ws_bwd 1x1                            dw.sample4           6.6e-08    6.8e-08  2.0e-06
    ws_bwd 3x3_288                        dw.sample2           6.4e-08    7.4e-08  2.0e-06
    ws_bwd 3x3_4608                       dw.sample0           5.9e-08    7.5e-08  2.0e-06
    bilinear_bwd (1, 1, 1, 2, 2, 4)       dlo.whole            3.3e-08    3.3e-08  2.0e-06
    bilinear_bwd (2, 2, 3, 4, 6, 3)       dlo.img0.ring        1.2e-07    1.2e-07  2.0e-06
    bilinear_bwd (1, 8, 8, 16, 16, 128)   dlo.img0.interior    9.9e-08    2.4e-07  2.0e-06
    bilinear_bwd (3, 12, 12, 24, 24, 3)   dlo.img0.interior    1.9e-07    5.4e-07  2.0e-06
    bilinear_bwd (1, 5, 7, 10, 14, 6)     dlo.img0.interior    9.1e-08    1.7e-07  2.0e-06
    bilinear_bwd (2, 16, 16, 32, 32, 256) dlo.img0.ring        5.7e-07    6.5e-07  2.0e-06
    bilinear_bwd (1, 4, 4, 7, 9, 8)       dlo.img0.interior    7.1e-08    7.1e-08  2.0e-06
    maxpool_bwd (1, 4, 64, 2)             dA.img0.interior     2.7e-08    2.5e-08  2.0e-06
    maxpool_bwd (2, 6, 64, 2)             dA.img0.interior     3.8e-08    2.5e-08  2.0e-06
    maxpool_bwd (1, 10, 32, 1)            dA.img0.interior     2.9e-08    2.7e-08  2.0e-06
    maxpool_bwd (3, 16, 96, 3)            dA.img1.interior     2.7e-08    2.7e-08  2.0e-06
    depth_tail (32, 1)                    inv.whole            8.2e-08    1.2e-07  2.0e-06
    depth_tail (32, 37)                   inv.whole            4.4e-08    6.0e-08  2.0e-06
    depth_tail (32, 4096)                 inv.whole            6.9e-08    8.3e-08  2.0e-06
    depth_tail (32, 262181)               inv.whole            7.7e-08    8.9e-08  2.0e-06
    depth_tail (8, 37)                    inv.whole            4.2e-08    4.1e-08  2.0e-06
    depth_tail (8, 1000)                  de.row.first         4.1e-08    4.1e-08  2.0e-06
    depth_tail (33, 37)                   inv.whole            7.3e-08    6.5e-08  2.0e-06
    depth_tail (33, 1000)                 inv.whole            7.9e-08    8.2e-08  2.0e-06
    smallk (37, 128, 3)                   dw.cols.0            6.8e-08    1.2e-07  2.0e-06
    smallk (1000, 100, 4)                 dw.cols.0            1.2e-07    2.7e-07  2.0e-06
    smallk (5, 64, 1)                     dw.whole             4.7e-08    4.2e-08  2.0e-06
    gelu_bwd                              dx.whole             4.7e-08    8.6e-08  2.0e-06
    relu_bwd                              dx.whole             2.2e-08    2.2e-08  2.0e-06
    relu_bwd_halo                         dx.whole             2.0e-08    2.0e-08  2.0e-06
    seg_act_bwd                           dup.whole            4.1e-08    4.1e-08  2.0e-06
"""
import ctypes
import math

import pytest
import torch

from tests import train_aux_refs as R

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
SCRATCH_BYTES = 48 << 20
MEASURED = {}          # test label -> (worst error / bound, slice label, error, bound, torch-f32 error)


# ---------------- specs of the small kernels ----------------
def spec_gelu(n):
    return R.Spec("gelu_bwd", [n], ins=["dy", "pre"], outs=[R._o("dx", (n,))])


def spec_relu(shape, with_add, halo):
    if halo:
        return R.Spec("relu_bwd_halo", list(shape), ins=["dy", "ref_halo", "add" if with_add else None], outs=[R._o("dx", shape)])
    return R.Spec("relu_bwd", [shape[0]], ins=["dy", "ref", "add" if with_add else None], outs=[R._o("dx", shape)])


def spec_seg_act(sigmoid):
    B, K, S = 2, 3, 18
    return R.Spec("seg_act_bwd", [B, K, S], flags=sigmoid, ins=["dseg", "seg"], outs=[R._o("dup", (B, S, S, K))])


def spec_merge_scatter():
    B, Rr, C = 2, 6, 20
    return R.Spec("merge_scatter", [B, Rr, C], ins=["dg"], outs=[R._o("dx", (B, Rr, Rr, C))])


def spec_scale_rows():
    M, C, rps = 24, 12, 6
    return R.Spec("scale_rows", [M, C, rps], ins=["in", "scale"], outs=[R._o("out", (M, C))])


def spec_unscale(n, inv_scale):
    return R.Spec("unscale_check", [n], f=(inv_scale, 0.0, 0.0), outs=[R._o("g", (n,)), R._o("found", (1,), torch.int32)], preset={"g": "g0", "found": "found0"})


def spec_drop_path(B, p, seed, stream_id):
    return R.Spec("drop_path_fill", [B, stream_id], f=(p, 0.0, 0.0), seed=seed, outs=[R._o("out", (B,))])


RELU_HALO_SHAPE = (2, 5, 7, 12)


def all_specs():
    """(label, Spec) of every call shape this module makes: tests/test_train_aux_refs.py sizes their scratch on the CPU."""
    out = [(f"ln/{c}", R.spec_ln(c)) for c in R.LN_CASES]
    for s in R.COLSUM_SHAPES:
        for wb in (False, True):
            out += [(f"colsum/{s}/b{int(wb)}/acc{acc}", R.spec_colsum(s, wb, acc, False)) for acc in (0, 1)]
            out.append((f"colsum2/{s}/b{int(wb)}", R.spec_colsum(s, wb, 0, True)))
    for c in R.BN_CASES:
        out += [(f"bn_fwd/{c}", R.spec_bn_fwd(c)), (f"bn_bwd/{c}", R.spec_bn_bwd(c))]
    out += [(f"gn/{c}", R.spec_gn(c)) for c in R.GN_CASES]
    out += [(f"ws/{c}", R.spec_ws(c)) for c in R.WS_CASES]
    out += [(f"bilinear/{s}/acc{acc}", R.spec_bilinear(s, acc)) for s in R.BILINEAR_SHAPES for acc in (0, 1)]
    out += [(f"maxpool/{s}", R.spec_maxpool(s)) for s in R.MAXPOOL_SHAPES]
    out += [(f"depth_tail/{s}", R.spec_depth_tail(s)) for s in R.DEPTH_TAIL_SHAPES]
    out += [(f"smallk/{s}", R.spec_smallk(s)) for s in R.SMALLK_SHAPES]
    out += [("gelu", spec_gelu(R.GELU_LINSPACE + R.GELU_RANDOM)), ("relu", spec_relu((R.RELU_N,), True, None)), ("relu_halo", spec_relu(RELU_HALO_SHAPE, True, True)),
            ("seg_act/0", spec_seg_act(0)), ("seg_act/1", spec_seg_act(1)), ("merge_scatter", spec_merge_scatter()), ("scale_rows", spec_scale_rows()),
            ("unscale", spec_unscale(70001, 0.5)), ("drop_path", spec_drop_path(37, 0.1, 7, 3))]
    return out


def bad_args(make):
    """(label, TrainAuxArgs) the entry must refuse; make(spec, ptr=...) fills every named pointer slot."""
    def mod(spec, **kw):
        a = make(spec)
        for k, v in kw.items():
            if k.startswith("dim"):
                a.dim[int(k[3:])] = v
            elif k.startswith("in"):
                a.inp[int(k[2:])] = v
            elif k.startswith("out"):
                a.out[int(k[3:])] = v
            else:
                setattr(a, k, v)
        return a
    base = make(R.spec_ln("5x96")).inp[0]
    ln, cs, gn = R.spec_ln("5x96"), R.spec_colsum((17, 65), True, 0, False), R.spec_gn("1x9x64")
    bil4, bil3 = R.spec_bilinear((1, 4, 4, 7, 9, 8), 0), R.spec_bilinear((2, 2, 3, 4, 6, 3), 0)
    yield "unknown kind", mod(ln, kind=len(R.KINDS))
    yield "negative kind", mod(ln, kind=-1)
    yield "ln: null y", mod(ln, in0=None)
    yield "ln: null dy", mod(ln, out0=None)
    yield "ln: M = 0", mod(ln, dim0=0)
    yield "ln: C < 0", mod(ln, dim1=-96)
    yield "ln: dgamma without xhat", mod(ln, out1=None)
    yield "ln: dy = dout with parameter gradients", mod(ln, out0=make(ln).inp[2])
    yield "colsum: null a", mod(cs, in0=None)
    yield "colsum: null out", mod(cs, out0=None)
    yield "colsum: N = 0", mod(cs, dim1=0)
    yield "colsum2: null out_a", mod(R.spec_colsum((17, 65), True, 0, True), out1=None)
    yield "bn_fwd: running_var without running_mean", mod(R.spec_bn_fwd("2x5"), out1=None)
    yield "bn_fwd: p = 1", mod(R.spec_bn_fwd("2x5", p=1.0))
    yield "bn_bwd: null keep", mod(R.spec_bn_bwd("2x5"), in2=None)
    yield "gn: no output", mod(gn, out0=None, out1=None, out2=None)
    yield "gn: C > 1024", mod(gn, dim2=2048, dim3=64)
    yield "gn: C % cpg", mod(gn, dim3=5)
    yield "gn: B = 0", mod(gn, dim0=0)
    yield "ws: Kpad below the fan-in", mod(R.spec_ws("stem"), dim3=144)
    yield "ws: null w", mod(R.spec_ws("stem"), in2=None)
    yield "smallk: K = 5", mod(R.spec_smallk((37, 128, 3)), dim2=5)
    yield "smallk: dw without x", mod(R.spec_smallk((37, 128, 3)), in2=None)
    yield "bilinear: C % 4 == 0 with a 4-byte aligned dhi", mod(bil4, in0=base + 4)
    yield "bilinear: C % 4 == 0 with a 4-byte aligned dlo", mod(bil4, out0=base + 8)
    yield "bilinear: h = 0", mod(bil3, dim1=0)
    yield "bilinear: null dlo", mod(bil3, out0=None)
    yield "maxpool: odd Hi", mod(R.spec_maxpool((1, 4, 64, 2)), dim1=5)
    yield "maxpool: C % cpg", mod(R.spec_maxpool((1, 4, 64, 2)), dim3=3)
    yield "depth_tail: K = 32 with a 4-byte aligned e", mod(R.spec_depth_tail((32, 37)), in0=base + 4)
    yield "depth_tail: null rowterm", mod(R.spec_depth_tail((8, 37)), out2=None)
    yield "merge_scatter: odd R", mod(spec_merge_scatter(), dim1=5)
    yield "scale_rows: C % 4", mod(spec_scale_rows(), dim1=10)
    yield "unscale: null found", mod(spec_unscale(64, 1.0), out1=None)
    yield "drop_path: p = 1", mod(spec_drop_path(8, 1.0, 0, 0))


# ---------------- harness ----------------
class Buf:
    """A device tensor with a 4 KB guard of 0xFF bytes directly behind it; without a value it is 0xFF bytes itself (NaN in f32)."""

    def __init__(self, shape, dtype, dev, value=None):
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.raw[: self.nbytes].view(dtype).view(tuple(shape))
        if value is not None:
            self.t.copy_(value.to(dtype))

    def ptr(self):
        return self.raw.data_ptr()

    def guard_untouched(self):
        return bool((self.raw[self.nbytes:] == 0xFF).all())


@pytest.fixture(scope="module")
def scratch(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return torch.empty((SCRATCH_BYTES + GUARD_BYTES,), dtype=torch.uint8, device=gpu_device)


def make_args(spec, ins=None, outs=None, ptr=None):
    from soccdpt_amd.lib import AUX, TrainAuxArgs
    a = TrainAuxArgs(kind=AUX[spec.kind], flags=spec.flags, seed=spec.seed)
    for i, v in enumerate(spec.dim):
        a.dim[i] = v
    for i, v in enumerate(spec.f):
        a.f[i] = v
    for i, n in enumerate(spec.ins):
        a.inp[i] = None if n is None else (ptr + 4096 * i if ins is None else ins[n].ptr())      # ptr: a placeholder per slot, 4 KB apart
    for i, o in enumerate(spec.outs):
        a.out[i] = None if o is None else (ptr + 4096 * (8 + i) if outs is None else outs[o[0]].ptr())
    return a


def call(spec, inp, scratch, finite=True):
    """One soccdpt_op_train_aux with canaries -> {output name: host tensor}."""
    from soccdpt_amd.lib import op_train_aux, op_train_aux_scratch_bytes
    dev = scratch.device
    outs, ins = {}, {}
    for o in spec.outs:
        if o is not None:
            name, shape, dtype = o
            src = spec.alias.get(name) or spec.preset.get(name)
            outs[name] = Buf(shape, dtype, dev, inp[src] if src else None)
    for n in spec.ins:
        if n is not None and n not in ins:
            aliased = [o for o, i in spec.alias.items() if i == n]
            ins[n] = outs[aliased[0]] if aliased else Buf(inp[n].shape, inp[n].dtype, dev, inp[n])
    a = make_args(spec, ins, outs)
    need = op_train_aux_scratch_bytes(a)
    assert need + GUARD_BYTES <= scratch.numel(), need
    scratch.fill_(0xFF)
    op_train_aux(a, scratch[:need])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_op_train_aux ({spec.kind} {spec.dim}): {e}", returncode=3)
    assert bool((scratch[need:] == 0xFF).all()), "the guard behind the scratch was written"
    for n, b in ins.items():
        assert b.guard_untouched(), f"the guard behind operand {n} was written"
        if b not in outs.values():
            assert torch.equal(b.t.cpu(), inp[n].to(b.t.dtype)), f"operand {n} was written"
    got = {}
    for n, b in outs.items():
        assert b.guard_untouched(), f"the guard behind {n} was written"
        got[n] = b.t.cpu()
        if finite and got[n].is_floating_point():
            assert bool(torch.isfinite(got[n]).all()), f"{n} is not finite everywhere: {int((~torch.isfinite(got[n])).sum())} of {got[n].numel()} elements"
    return got


def call_twice(spec, inp, scratch, finite=True):
    got = call(spec, inp, scratch, finite)
    again = call(spec, inp, scratch, finite)
    for k in got:
        assert torch.equal(got[k].view(torch.uint8), again[k].view(torch.uint8)), f"{spec.kind} {spec.dim}: {k} differs between two calls"
    return got


def check(label, kind, got, ref64, yard32, names=None):
    """Relative L2 on the whole tensor and on every slice against max(3 x torch-f32 error, 2e-6); prints every figure."""
    worst = MEASURED.get(label, (0.0, "", 0.0, 0.0, 0.0))
    failures = []
    for name in (names or [n for n in got if got[n].is_floating_point()]):
        for (sl, gs), (_, rs), (_, ts) in zip(R.slices(kind, name, got[name]), R.slices(kind, name, ref64[name]), R.slices(kind, name, yard32[name])):
            err, torch_err = R.rel_l2(gs, rs), R.rel_l2(ts, rs)
            bound = max(R.F32_FACTOR * torch_err, R.F32_FLOOR)
            print(f"  {label} {name}.{sl}: kernel {err:.2e}  bound {bound:.2e}  torch-f32 {torch_err:.2e}")
            if err / bound > worst[0]:
                worst = (err / bound, f"{name}.{sl}", err, bound, torch_err)
            if not err < bound:
                failures.append((name, sl, err, bound))
    MEASURED[label] = worst
    print(f"MEASURED {label}: worst {worst[1]} kernel {worst[2]:.1e} bound {worst[3]:.1e} torch-f32 {worst[4]:.1e}")
    assert not failures, failures


# ---------------- the tests ----------------
@pytest.mark.parametrize("case", list(R.LN_CASES))
def test_ln_bwd(scratch, case):
    inp, spec = R.build_ln(case), R.spec_ln(case)
    got = call_twice(spec, inp, scratch)
    assert set(got) == {o[0] for o in spec.outs if o}
    check(f"ln_bwd {case}", "ln_bwd", got, R.ref_ln(inp), R.torch_ln(inp, torch.float32))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=str)
def test_colsum(scratch, shape, with_b, accumulate):
    inp = R.build_colsum(shape, with_b, accumulate, False)
    got = call_twice(R.spec_colsum(shape, with_b, accumulate, False), inp, scratch)
    check(f"colsum {shape} b{int(with_b)} acc{accumulate}", "colsum", got, R.ref_colsum(inp), R.ref_colsum(inp, torch.float32))


@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("shape", R.COLSUM_SHAPES, ids=str)
def test_colsum2(scratch, shape, with_b):
    inp = R.build_colsum(shape, with_b, 0, True)
    got = call_twice(R.spec_colsum(shape, with_b, 0, True), inp, scratch)
    check(f"colsum2 {shape} b{int(with_b)}", "colsum2", got, R.ref_colsum(inp), R.ref_colsum(inp, torch.float32))
    # the same additions in the same order as the single form
    single = call(R.spec_colsum(shape, with_b, 0, False), inp, scratch)
    assert torch.equal(single["out"].view(torch.int32), got["out_ab"].view(torch.int32))


@pytest.mark.parametrize("case", list(R.BN_CASES))
def test_bn_train(scratch, case):
    """Statistics (incl. the running buffers), forward at p = 0, and the backward over the forward's own outputs."""
    inp = R.build_bn(case)
    ref, yard = R.ref_bn(inp), R.torch_bn(inp, torch.float32)
    fwd = call_twice(R.spec_bn_fwd(case), inp, scratch)
    assert bool((fwd["keep"] == 1).all())
    check(f"bn_fwd {case}", "bn_fwd", fwd, ref, yard)
    assert torch.equal(fwd["y"] > 0, inp["pre64"] > 0)
    bwd = call_twice(R.spec_bn_bwd(case), dict(inp, y=fwd["y"], keep=fwd["keep"], stats=fwd["stats"]), scratch)
    check(f"bn_bwd {case}", "bn_bwd", bwd, ref, yard)


def test_bn_dropout(scratch):
    """Dropout p = 0.1 has no torch parity (a counter hash): the mask's properties, and the backward pinned to the returned mask."""
    case, p = "4099x128", 0.1
    inp = R.build_bn(case)
    fwd = call_twice(R.spec_bn_fwd(case, p, seed=1234), inp, scratch)      # the same seed: the same mask and values
    keep = fwd["keep"]
    assert bool(((keep == 0) | (keep == 1)).all())
    assert bool((fwd["y"][keep == 0] == 0).all())
    n = keep.numel()
    assert abs(float(keep.float().mean()) - (1 - p)) <= 5.0 * math.sqrt(p * (1 - p) / n)
    other = call(R.spec_bn_fwd(case, p, seed=1235), inp, scratch)
    differ = float((other["keep"] != keep).float().mean())
    assert abs(differ - 2 * p * (1 - p)) <= 5.0 * math.sqrt(0.18 * 0.82 / n), differ          # two independent masks
    ref, yard = R.ref_bn(inp, keep=keep, p=p), R.ref_bn(inp, torch.float32, keep=keep, p=p)
    check("bn_fwd dropout", "bn_fwd", fwd, ref, yard, names=["y", "stats", "rmean", "rvar"])
    kept = keep == 1
    assert R.rel_l2(fwd["y"][kept], ref["y"][kept]) < 2e-6                                       # the kept values carry 1 / (1 - p)
    bwd = call_twice(R.spec_bn_bwd(case, p), dict(inp, y=fwd["y"], keep=keep, stats=fwd["stats"]), scratch)
    check("bn_bwd dropout", "bn_bwd", bwd, ref, yard)


@pytest.mark.parametrize("case", list(R.GN_CASES))
def test_gn_bwd(scratch, case):
    inp, spec = R.build_gn(case), R.spec_gn(case)
    got = call_twice(spec, inp, scratch)
    assert set(got) == {o[0] for o in spec.outs if o}
    check(f"gn_bwd {case}", "gn_bwd", got, R.ref_gn(inp), R.torch_gn(inp, torch.float32))


@pytest.mark.parametrize("case", list(R.WS_CASES))
def test_ws_bwd(scratch, case):
    inp = R.build_ws(case)
    inp_dev = dict(inp, dwh=torch.nan_to_num(inp["dwh"], nan=1e30), wh=torch.nan_to_num(inp["wh"], nan=1e30))   # columns behind the fan-in: must not be read
    got = call_twice(R.spec_ws(case), inp_dev, scratch)
    check(f"ws_bwd {case}", "ws_bwd", got, R.ref_ws(inp), R.ref_ws(inp, torch.float32))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", R.BILINEAR_SHAPES, ids=str)
def test_bilinear_bwd(scratch, shape, accumulate):
    inp = R.build_bilinear(shape, accumulate)
    got = call_twice(R.spec_bilinear(shape, accumulate), inp, scratch)
    check(f"bilinear_bwd {shape} acc{accumulate}", "bilinear_bwd", got, R.ref_bilinear(inp), R.torch_bilinear(inp, torch.float32))


def test_bilinear_reaches_both_kernels():
    assert {s[5] % 4 == 0 for s in R.BILINEAR_SHAPES} == {True, False}


@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=str)
def test_maxpool_bwd(scratch, shape):
    inp = R.build_maxpool(shape)
    got = call_twice(R.spec_maxpool(shape), inp, scratch)
    idx = got["idx"]
    assert bool((idx < 9).all())
    win = R._pool_windows(R.pool_activation(inp))
    first, decided, wmax = R.pool_classes(win)
    assert torch.equal(idx[decided], first[decided].to(torch.uint8)), "a decided window resolved to another position than the float64 argmax"
    at = win.gather(-1, idx.long().unsqueeze(-1)).squeeze(-1)
    assert bool(((wmax - at)[~decided] <= R.POOL_VALUE_TOL).all()) and bool(torch.isfinite(at).all())
    Hi = shape[1]
    ref = {"dA": R.pool_scatter(inp["dpool"], idx, Hi)}
    mag = R.pool_scatter(inp["dpool"].abs(), idx, Hi)
    assert bool(((got["dA"].double() - ref["dA"]).abs() <= 2.0 ** -22 * mag).all()), "dA is not the scatter of dpool by the returned bytes"
    check(f"maxpool_bwd {shape}", "maxpool_bwd", got, ref, {"dA": R.pool_scatter(inp["dpool"], idx, Hi, torch.float32)}, names=["dA"])


@pytest.mark.parametrize("shape", R.DEPTH_TAIL_SHAPES, ids=str)
def test_depth_tail(scratch, shape):
    inp = R.build_depth_tail(shape)
    got = call_twice(R.spec_depth_tail(shape), inp, scratch)
    assert torch.equal(got["inv"] > 0, inp["s64"] > 0)
    check(f"depth_tail {shape}", "depth_tail", got, R.ref_depth_tail(inp), R.ref_depth_tail(inp, torch.float32))


@pytest.mark.parametrize("shape", R.SMALLK_SHAPES, ids=str)
def test_smallk(scratch, shape):
    inp = R.build_smallk(shape)
    got = call_twice(R.spec_smallk(shape), inp, scratch)
    check(f"smallk {shape}", "smallk", got, R.ref_smallk(inp), R.ref_smallk(inp, torch.float32))


def test_gelu_bwd(scratch):
    inp = R.build_gelu()
    got = call_twice(spec_gelu(inp["pre"].numel()), inp, scratch)
    check("gelu_bwd", "gelu_bwd", got, R.ref_gelu(inp), R.torch_gelu(inp, torch.float32))
    lin = slice(0, R.GELU_LINSPACE)                                                   # the linspace(-12, 12) part on its own
    err, yard = R.rel_l2(got["dx"][lin], R.ref_gelu(inp)["dx"][lin]), R.rel_l2(R.torch_gelu(inp, torch.float32)["dx"][lin], R.ref_gelu(inp)["dx"][lin])
    print(f"  gelu_bwd linspace: kernel {err:.2e} torch-f32 {yard:.2e}")
    assert err < max(R.F32_FACTOR * yard, R.F32_FLOOR)


@pytest.mark.parametrize("with_add", [False, True])
def test_relu_bwd(scratch, with_add):
    inp = R.build_relu(with_add)
    got = call_twice(spec_relu((R.RELU_N,), with_add, None), inp, scratch)
    check(f"relu_bwd add{int(with_add)}", "relu_bwd", got, R.ref_relu(inp), R.torch_relu(inp, torch.float32))
    assert torch.equal(got["dx"], R.torch_relu(inp, torch.float32)["dx"])   # a mask and at most one addition: the same bits


@pytest.mark.parametrize("with_add", [False, True])
def test_relu_bwd_halo(scratch, with_add):
    inp = R.build_relu(with_add, RELU_HALO_SHAPE)
    got = call_twice(spec_relu(RELU_HALO_SHAPE, with_add, True), inp, scratch)
    check(f"relu_bwd_halo add{int(with_add)}", "relu_bwd_halo", got, R.ref_relu(inp), R.torch_relu(inp, torch.float32))
    assert torch.equal(got["dx"], R.torch_relu(inp, torch.float32)["dx"])


@pytest.mark.parametrize("sigmoid", [0, 1])
def test_seg_act_bwd(scratch, sigmoid):
    inp = R.build_seg_act(sigmoid)
    got = call_twice(spec_seg_act(sigmoid), inp, scratch)
    check(f"seg_act_bwd sigmoid{sigmoid}", "seg_act_bwd", got, R.ref_seg_act(inp), R.ref_seg_act(inp, torch.float32))


def test_merge_scatter_is_the_permutation(scratch):
    inp = R.build_merge_scatter()
    got = call_twice(spec_merge_scatter(), inp, scratch)
    assert torch.equal(got["dx"].view(torch.int32), R.ref_merge_scatter(inp)["dx"].view(torch.int32))


def test_scale_rows_is_one_product(scratch):
    inp = R.build_scale_rows()
    got = call_twice(spec_scale_rows(), inp, scratch)
    assert torch.equal(got["out"].view(torch.int32), R.ref_scale_rows(inp)["out"].view(torch.int32))


def test_unscale_check(scratch):
    n = 70001
    g0 = torch.randn(n, generator=torch.Generator().manual_seed(5))
    zero = torch.zeros(1, dtype=torch.int32)
    got = call_twice(spec_unscale(n, 0.5), {"g0": g0, "found0": zero}, scratch)
    assert int(got["found"]) == 0 and torch.equal(got["g"], g0 * 0.5)
    for bad, where in ((float("inf"), n - 1), (float("-inf"), 0), (float("nan"), 4097)):
        g1 = g0.clone()
        g1[where] = bad
        got = call_twice(spec_unscale(n, 0.5), {"g0": g1, "found0": zero}, scratch, finite=False)
        assert int(got["found"]) == 1, (bad, where)
        ok = torch.ones(n, dtype=torch.bool)
        ok[where] = False
        assert torch.equal(got["g"][ok], (g0 * 0.5)[ok])
    # a large finite value times a scale above 1 overflows: found
    g2 = g0.clone()
    g2[17] = 3.0e38
    assert int(call(spec_unscale(n, 4.0), {"g0": g2, "found0": zero}, scratch, finite=False)["found"]) == 1


def test_drop_path_fill(scratch):
    B, p = 4001, 0.1
    got = call_twice(spec_drop_path(B, p, seed=7, stream_id=3), {}, scratch)["out"]          # the same seed: the same scales
    one = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    assert bool(((got == 0) | (got == one)).all())
    assert abs(float((got != 0).float().mean()) - (1 - p)) <= 5.0 * math.sqrt(p * (1 - p) / B)
    for seed, stream in ((8, 3), (7, 4)):
        other = call(spec_drop_path(B, p, seed=seed, stream_id=stream), {}, scratch)["out"]
        assert not torch.equal(other, got)
    # constant per sample: sample b's scale does not depend on how many samples are filled
    assert torch.equal(call(spec_drop_path(37, p, seed=7, stream_id=3), {}, scratch)["out"], got[:37])
    assert bool((call(spec_drop_path(64, 0.0, seed=7, stream_id=3), {}, scratch)["out"] == 1).all())


def test_bad_arguments_launch_nothing(scratch, gpu_device):
    from soccdpt_amd.lib import load_library, op_train_aux, op_train_aux_scratch_bytes
    L = load_library()
    arena = Buf((1 << 18,), torch.float32, gpu_device, torch.zeros(1 << 18))         # every pointer of the refused calls points into real memory
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    n = 0
    for label, a in bad_args(lambda spec: make_args(spec, ptr=arena.ptr())):
        with pytest.raises(RuntimeError, match="soccdpt_op_train_aux"):
            op_train_aux_scratch_bytes(a)
        with pytest.raises(RuntimeError, match="soccdpt_op_train_aux"):
            op_train_aux(a, scratch[:1 << 20])
        n += 1
    assert n >= 30
    good = make_args(R.spec_colsum((17, 65), True, 0, False), ptr=arena.ptr())
    need = op_train_aux_scratch_bytes(good)
    with pytest.raises(RuntimeError, match="too small"):
        op_train_aux(good, scratch[:need - 256])
    with pytest.raises(RuntimeError, match="aligned"):
        op_train_aux(good, scratch[128:128 + need])
    assert L.soccdpt_op_train_aux(None, ctypes.c_void_p(scratch.data_ptr()), need, None) == 1
    assert int(L.soccdpt_launch_counter()) == before, "a refused call launched a kernel"
    torch.cuda.synchronize()
    assert bool((arena.t == 0).all()) and arena.guard_untouched()
    op_train_aux(good, scratch[:need])                                     # and the good one launches: colsum's two kernels
    torch.cuda.synchronize()
    assert int(L.soccdpt_launch_counter()) == before + 2
