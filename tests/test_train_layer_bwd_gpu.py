"""GPU: linear_bwd / conv3_bwd / conv_gen_bwd of the training step, one layer at a time through soccdpt_op_train_layer_bwd, against float64 in every
operand format (f32, x3, bf16, f16) and on every staging route.

The whole-step tests hold the 16-bit modes to bf16's rounding floor (1e-2 .. 6e-2), which hides every staging mistake.  Here the bf16 / f16 operands
are pre-rounded (tests/layer_bwd_refs.py operand): the library's conversion is exact, the float64 reference over the same values differs from the
kernels by f32 accumulation only, and the bounds are those of the inner GEMM (test_wgrad_tn_linear / _conv3x3): 2e-5 for bf16 / f16, 2e-6 for x3.
Where a layer runs in f32 (the f32 mode, and shapes an amp mode cannot take) the bound is 3 x the error of torch's own CPU f32 result of the same
operation on the same inputs, floor 2e-6.  Errors are relative L2 on the whole tensor and on every slice of layer_bwd_refs.slices (taps, border ring /
interior per image, the last partial 64-row block); no case and no element is excluded.

Per call: the scratch is 0xFF bytes (NaN in f32, bf16, fp16 and both halves of x3) and every output NaN beforehand; 0xFF guards of 4 KB sit behind
the scratch and -- after 127 elements of readable room -- behind every operand and output; afterwards every requested output is finite, every guard
and every output not asked for is untouched, the SOCCDPT_ROUTE_* bits equal the expectation derived below from the conditions in the sources, and a
second call gives the same bits.  test_every_route_was_reached closes the module: the routes seen cover every bit the library defines.

Case tables: the shapes of the issue this module answers, with two adjustments the sources require.  conv3 case h (N = 12) cannot take dX -- the dgrad
GEMM's K is N and the igemm needs K % 32 == 0 -- so it runs dW / db only, and case h2 (1, 5, 32, 48) adds the f32 fallback with all outputs (C % 32 != 0).
Linear (300, 96, 64) runs "full" with every output and "bare" like the patch embedding: no dX, unstaged W.  conv3 case i (odd r, C % 64 == 0) holds the
16-bit modes to the im2col^T route the alignment rule of csrc/train_plan.h sends them on; it came after the table below was measured and is held to the same bounds.

Measured on MI355X: the worst relative L2 over every output, slice and variant of a case, per mode, and torch's CPU f32 error on the f32 mode's
inputs (3 x it stays under the 2e-6 floor everywhere, so every layer that runs in f32 is held to 2e-6).  Bounds: f32 2e-6, x3 2e-6, bf16 / f16
2e-5; a mode that falls back to f32 on a shape (conv3 h, h2; linear 320x64x32, 256x96x36 in x3; conv_gen outside the 16-bit TN branch) is held to
the f32 bound.  Every test prints each figure with -s.

    case                      f32       x3     bf16      f16  torch f32
    conv3 a               6.2e-07  2.3e-07  2.0e-07  2.2e-07    3.1e-07
    conv3 a2 (reuse_xt)   2.9e-07  1.5e-07  2.9e-07  3.1e-07    3.0e-07
    conv3 b               6.0e-07  2.3e-07  2.0e-07  2.2e-07    2.5e-07
    conv3 c               6.3e-07  2.3e-07  2.0e-07  2.2e-07    2.2e-07
    conv3 d               3.0e-07  1.4e-07  9.5e-08  1.1e-07    2.1e-07
    conv3 e               3.0e-07  1.5e-07  3.0e-07  3.0e-07    2.8e-07
    conv3 f               2.9e-07  1.4e-07  2.9e-07  3.0e-07    2.1e-07
    conv3 g               3.0e-07  1.5e-07  3.0e-07  3.2e-07    2.3e-07
    conv3 h               8.6e-08  8.6e-08  2.7e-08  8.2e-08    9.0e-08
    conv3 h2              3.3e-07  3.3e-07  1.4e-07  2.7e-07    1.4e-07
    linear 577x96x128     3.1e-07  1.2e-07  7.5e-08  8.9e-08    2.5e-07
    linear 256x192x96     2.9e-07  1.2e-07  7.9e-08  9.5e-08    2.5e-07
    linear 144x128x512    2.2e-07  1.1e-07  6.5e-08  8.1e-08    2.1e-07
    linear 512x384x128    3.5e-07  1.5e-07  1.1e-07  1.3e-07    2.5e-07
    linear 300x96x64      3.0e-07  1.1e-07  7.2e-08  8.9e-08    2.2e-07
    linear 320x64x32      3.2e-07  3.2e-07  1.2e-07  3.0e-07    2.3e-07
    linear 256x96x36      3.0e-07  3.0e-07  8.4e-08  1.0e-07    2.2e-07
    linear 64x1536x384    2.9e-07  1.4e-07  2.3e-07  2.5e-07    2.5e-07
    conv_gen same_s2      1.6e-07  1.6e-07  6.3e-08  1.4e-07    2.4e-07
    conv_gen pp4          1.5e-07  1.5e-07  6.2e-08  1.5e-07    1.5e-07
    conv_gen s1_f32       4.3e-07  4.3e-07  1.7e-07  4.2e-07    2.3e-07
    conv_gen s1_tn        6.1e-07  6.1e-07  2.0e-07  2.2e-07    3.0e-07
"""
from dataclasses import dataclass

import pytest
import torch

from tests import layer_bwd_refs as LR

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
ROOM = 127                         # elements an operand may be read past its end (tr_wgrad_tn's contract for masked edge tiles)
TAIL = ROOM + GUARD_BYTES // 4     # f32 elements of 0xFF behind every operand and output


# ---------------- cases ----------------
@dataclass(frozen=True)
class Route:
    """What the sources say a (case, format) does.  fmt: operand format of the layer's GEMMs; wgrad: tn | x3shift | im2colT | haloshift | transpose;
    big / skd: gemm_wgrad's 128 x 128 tile / deferred split-K sum; dsplit: the dgrad GEMM splits K."""
    fmt: str
    wgrad: str
    big: bool = False
    skd: bool = False
    dsplit: bool = False


def _r(wgrad, big=False, skd=False, dsplit=False):
    return lambda fmt: Route(fmt, wgrad, big, skd, dsplit)


def _per_fmt(f32, x3, bf16, f16=None, fallback=()):
    """{mode: Route}; modes in `fallback` run the layer in f32."""
    rows = {"f32": f32, "x3": x3, "bf16": bf16, "f16": f16 or bf16}
    return {m: rows[m]("f32" if (m == "f32" or m in fallback) else m) for m in LR.FORMATS}


ALL_AMP = ("x3", "bf16", "f16")

# conv3: (B, r, N, C).  fmt = the amp mode's when N, C % 32 == 0.  TN: fmt != f32, halo pixels padded to 64 >= 256, N, C % 128 == 0.  Otherwise x3 with
# C % 64 == 0: three-copy shift; C % 64 != 0 (or x3, or 16-bit with an odd r: the vertical taps of the halo-shift would sit on 2-byte boundaries): im2col^T;
# else halo-shift.  gemm_wgrad: big = M, N % 128 == 0, K % 64 == 0, >= 8 big tiles, C % 128 == 0;
# splits S = min(512 / tiles, nk / 8 (16-bit: nk / 2)), sk_defer with big and S > 1.  gemm (dgrad, f32 / x3 only): split when tiles <= 96 and 9 N / 32 >= 48.
CONV3 = {
    # 392 halo pixels padded to 448.  f32: ld = 512, 9 big tiles, nk = 16 -> S = 2
    "a": ((2, 12, 128, 128), _per_fmt(_r("haloshift", big=True, skd=True), _r("tn"), _r("tn"))),
    # a, second layer on the same input (N = 256): dgrad K = 9 * 256 / 32 = 72 k-tiles -> split
    "a2": ((2, 12, 256, 128), _per_fmt(_r("haloshift", big=True, skd=True, dsplit=True), _r("tn", dsplit=True), _r("tn"))),
    # r + 2 = 16, 256 halo pixels: the TN minimum, no K padding.  f32: ld = 384, nk = 12 -> S = 1: the big tile is given up
    "b": ((1, 14, 128, 256), _per_fmt(_r("haloshift"), _r("tn"), _r("tn"))),
    # 128 halo pixels < 256: not TN.  16-bit: two copies, ld = 256, big, nk = 4 -> S = 2.  x3: ld = 320, nk = 10 -> S = 1.  f32: nk = 8 -> S = 1
    "c": ((2, 6, 128, 128), _per_fmt(_r("haloshift"), _r("x3shift"), _r("haloshift", big=True, skd=True))),
    "d": ((1, 12, 32, 128), _per_fmt(_r("haloshift"), _r("x3shift"), _r("haloshift"))),
    # C = 96: im2col^T everywhere; M = 243 -> 256.  dgrad: 8 tiles, 72 k-tiles -> split
    "e": ((3, 9, 256, 96), _per_fmt(_r("im2colT", dsplit=True), _r("im2colT", dsplit=True), _r("im2colT"))),
    "f": ((1, 8, 256, 192), _per_fmt(_r("haloshift", dsplit=True), _r("x3shift", dsplit=True), _r("haloshift"))),
    # 16-bit: ld = 256, 36 big tiles, nk = 4 -> S = 2, deferred.  x3 (nk = 10) and f32 (nk = 8): S = 1
    "g": ((2, 6, 256, 256), _per_fmt(_r("haloshift", dsplit=True), _r("x3shift", dsplit=True), _r("haloshift", big=True, skd=True))),
    "h": ((1, 5, 12, 32), _per_fmt(_r("im2colT"), _r("im2colT"), _r("im2colT"), fallback=ALL_AMP)),
    "h2": ((1, 5, 32, 48), _per_fmt(_r("im2colT"), _r("im2colT"), _r("im2colT"), fallback=ALL_AMP)),
    # odd r with C % 64 == 0: f32 shifts by elements of 4 bytes, x3 pitches the rows to 16; the 16-bit modes take im2col^T (M = 25 -> 128).  No splits anywhere
    "i": ((1, 5, 32, 64), _per_fmt(_r("haloshift"), _r("x3shift"), _r("im2colT"))),
}
CONV3_NO_DX = {"h"}
CONV3_EXTRA = {"a", "c", "e"}      # also dW-only and dX-only

# linear: (M, N, K).  fmt = the mode's when N % 32 == 0, K > 32 and K % 32 == 0 (16-bit: K % 4 == 0).  TN: fmt != f32, M padded to 64 >= 256, K % 32 == 0.
LINEAR = {
    "577x96x128": ((577, 96, 128), _per_fmt(_r("transpose"), _r("tn"), _r("tn"))),
    "256x192x96": ((256, 192, 96), _per_fmt(_r("transpose"), _r("tn"), _r("tn"))),
    "144x128x512": ((144, 128, 512), _per_fmt(_r("transpose"), _r("transpose"), _r("transpose"))),
    "512x384x128": ((512, 384, 128), _per_fmt(_r("transpose"), _r("tn"), _r("tn"))),
    "300x96x64": ((300, 96, 64), _per_fmt(_r("transpose"), _r("tn"), _r("tn"))),
    "320x64x32": ((320, 64, 32), _per_fmt(_r("transpose"), _r("transpose"), _r("transpose"), fallback=ALL_AMP)),
    "256x96x36": ((256, 96, 36), _per_fmt(_r("transpose"), _r("transpose"), _r("transpose"), fallback=("x3",))),
    # dgrad: 6 tiles, 48 k-tiles -> split in f32 and x3
    "64x1536x384": ((64, 1536, 384), _per_fmt(_r("transpose", dsplit=True), _r("transpose", dsplit=True), _r("transpose"))),
}
LINEAR_EXTRA = {"577x96x128", "256x192x96", "144x128x512"}
LINEAR_BARE_NO_DX = {"300x96x64"}

# conv_gen: (B, Hi, Ho, N, C, stride, pad).  16-bit modes, stride 1 / pad 1, TN shapes: the TN branch; everything else in f32 with im2col^T.
CONV_GEN = {
    "same_s2": ((2, 12, 6, 64, 64, 2, 0), _per_fmt(_r("im2colT"), _r("im2colT"), _r("im2colT"), fallback=ALL_AMP)),
    "pp4": ((1, 6, 3, 64, 64, 2, 1), _per_fmt(_r("im2colT"), _r("im2colT"), _r("im2colT"), fallback=ALL_AMP)),
    "s1_f32": ((2, 8, 8, 64, 64, 1, 1), _per_fmt(_r("im2colT"), _r("im2colT"), _r("im2colT"), fallback=ALL_AMP)),
    "s1_tn": ((2, 12, 12, 128, 128, 1, 1), _per_fmt(_r("im2colT"), _r("im2colT"), _r("tn"), fallback=("x3",))),
}


@dataclass(frozen=True)
class Variant:
    name: str
    dX: bool = True
    dW: bool = True
    db: bool = True
    res: bool = False
    stage: bool = False
    defer: bool = False


FULL = Variant("full", res=True, stage=True, defer=True)
BARE = Variant("bare")
DW_ONLY = Variant("dW_only", dX=False, db=False, defer=True)
DX_ONLY = Variant("dX_only", dW=False, db=False, stage=True)


def _has_slot(kind, N, C):
    """The shapes stage_weights() keeps a slot for (csrc/train_step.cpp wt_slot_kind)."""
    if kind == "conv_gen":
        return False
    return N % 32 == 0 and C % 32 == 0 and (kind == "conv3" or C > 32)


def expected_path(kind, N, C, route: Route, v: Variant) -> int:
    from soccdpt_amd.lib import ROUTE_BITS as R
    p = R["fmt_" + route.fmt]
    if v.dX:
        p |= R["w_staged"] if (v.stage and _has_slot(kind, N, C)) else R["w_fallback"]
        if route.dsplit:
            p |= R["dgrad_splitk"]
    if v.dW:
        p |= R["wgrad_" + route.wgrad]
        if route.wgrad == "tn":
            p |= R["sum_deferred"] if (v.defer and kind != "conv_gen") else R["sum_immediate"]
        p |= (R["wgrad_big_tile"] if route.big else 0) | (R["wgrad_sk_defer"] if route.skd else 0)
    return p


# ---------------- harness ----------------
_SEEN = set()          # every path_out of the module
MEASURED = {}          # (kind, case, mode) -> (worst kernel error / bound ratio, label, error, bound)


@pytest.fixture(scope="module")
def engine(gpu_device):
    from oracle import soccdpt_ref as R
    from soccdpt_amd.lib import PREC_F32, Engine, make_config
    cam, cfg = R.Camera(), R.ProjConfig()
    c = make_config("swin2t16_256", 3, 256, True, False, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                    cfg.grid_size, cfg.occupancy_shape(), cfg.pc_scale, cfg.pc_shift, cfg.correction_angle, precision=PREC_F32)
    eng = Engine(c, gpu_device)
    yield eng
    eng.train_set_amp(0)
    eng.close()


class Guarded:
    """A device f32 tensor with 127 readable elements and a 4 KB guard behind it, all 0xFF bytes (NaN)."""

    def __init__(self, shape, dev, value=None):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.raw = torch.full(((n + TAIL) * 4,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.raw[: n * 4].view(torch.float32).view(shape)
        if value is not None:
            self.t.copy_(value)

    def ptr(self):
        return self.raw.data_ptr()

    def tail_untouched(self):
        return bool((self.raw[self.n * 4:] == 0xFF).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


class Scratch:
    """The module's one scratch buffer (plus its guard): large enough for every case here, so no call moves it."""

    def __init__(self, dev):
        self.dev = dev
        self.buf = torch.empty(((96 << 20) + GUARD_BYTES,), dtype=torch.uint8, device=dev)

    def take(self, need):
        assert need + GUARD_BYTES <= self.buf.numel(), need
        return self.buf


@pytest.fixture(scope="module")
def scratch(gpu_device):
    return Scratch(gpu_device)


def _shape_fields(kind, shape):
    if kind == "linear":
        M, N, K = shape
        return dict(kind=0, M=M, N=N, C=K)
    if kind == "conv3":
        B, r, N, C = shape
        return dict(kind=1, B=B, r=r, N=N, C=C)
    B, Hi, Ho, N, C, s, p = shape
    return dict(kind=2, B=B, Hi=Hi, Ho=Ho, N=N, C=C, stride=s, pad=p)


def _tensor_shapes(kind, shape):
    """-> shapes of dY, X (plain NHWC / rows), W, dX."""
    if kind == "linear":
        M, N, K = shape
        return (M, N), (M, K), (N, K), (M, K)
    if kind == "conv3":
        B, r, N, C = shape
        return (B, r, r, N), (B, r, r, C), (N, C, 3, 3), (B, r, r, C)
    B, Hi, Ho, N, C, s, p = shape
    return (B, Ho, Ho, N), (B, Hi, Hi, C), (N, 9, C), (B, Hi, Hi, C)


def make_inputs(kind, shape, mode, dev, seed, X=None):
    """Host operands (f32, pre-rounded for the 16-bit modes) and their guarded device copies; X: reuse another case's input (host, device)."""
    g = torch.Generator().manual_seed(seed)
    sdy, sx, sw, sdx = _tensor_shapes(kind, shape)
    h = {"dY": LR.operand(mode, sdy, g), "W": LR.operand(mode, sw, g), "res": torch.randn(sdx, generator=g)}
    if X is None:
        h["X"] = LR.operand(mode, sx, g)
        dX = Guarded(LR.halo(h["X"]).shape if kind != "linear" else sx, dev, LR.halo(h["X"]) if kind != "linear" else h["X"])
    else:
        h["X"], dX = X
    d = {"dY": Guarded(sdy, dev, h["dY"]), "W": Guarded(sw, dev, h["W"]), "res": Guarded(sdx, dev, h["res"]), "X": dX}
    return h, d


def references(kind, shape, h, res, dtype):
    r = h["res"] if res else None
    if kind == "linear":
        return LR.linear_bwd_ref(h["dY"], h["X"], h["W"], r, dtype)
    if kind == "conv3":
        return LR.conv3_bwd_ref(h["dY"], h["X"], h["W"], r, dtype)
    return LR.conv_gen_bwd_ref(h["dY"], h["X"], h["W"], shape[5], shape[6], dtype)


def call(engine, scratch, kind, shape, d, v: Variant, reuse_xt=False, fill=True, guard_from=None):
    """One soccdpt_op_train_layer_bwd with canaries -> ({name: host tensor}, path, scratch bytes of the call)."""
    from soccdpt_amd.lib import TrainLayerBwdArgs, op_train_layer_bwd, op_train_layer_bwd_scratch_bytes
    dev = d["dY"].raw.device
    sdy, sx, sw, sdx = _tensor_shapes(kind, shape)
    N = sdy[-1]
    outs = {"dX": Guarded(sdx, dev), "dW": Guarded(sw, dev), "db": Guarded((N,), dev)}
    want = {"dX": v.dX, "dW": v.dW, "db": v.db}
    a = TrainLayerBwdArgs(**_shape_fields(kind, shape))
    a.stage_weight, a.defer, a.reuse_xt = int(v.stage), int(v.defer), int(reuse_xt)
    a.dY, a.X, a.W = d["dY"].ptr(), d["X"].ptr(), d["W"].ptr()
    a.dX_res = d["res"].ptr() if (v.res and v.dX and kind != "conv_gen") else None
    for k in outs:
        setattr(a, k, outs[k].ptr() if want[k] else None)
    need = op_train_layer_bwd_scratch_bytes(a)
    buf = scratch.take(need)
    if fill:
        buf.fill_(0xFF)
    path = op_train_layer_bwd(engine, a, buf[:need])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_op_train_layer_bwd ({kind} {shape} {v.name}): {e}", returncode=3)
    _SEEN.add(path)
    lo = need if guard_from is None else max(need, guard_from)
    assert bool((buf[lo:] == 0xFF).all()), "the guard behind the scratch was written"
    for k, gd in d.items():
        assert gd.tail_untouched(), f"the guard behind operand {k} was written"
    got = {}
    for k, o in outs.items():
        if want[k]:
            assert o.tail_untouched(), f"the guard behind {k} was written"
            assert bool(torch.isfinite(o.t).all()), f"{k} is not finite everywhere: {int((~torch.isfinite(o.t)).sum())} of {o.n} elements"
            got[k] = o.t.cpu()
        else:
            assert o.untouched(), f"{k} was not requested but was written"
    return got, path, need


def check_values(kind, key, mode, route: Route, got, ref64, ref32, tag):
    """Relative L2 on the whole tensor and on every slice, against the bound of the format the layer ran in."""
    worst = MEASURED.get(key, (0.0, "", 0.0, 0.0))
    failures = []
    for name, g in got.items():
        for (label, gs), (_, rs), (_, ts) in zip(LR.slices(kind, name, g), LR.slices(kind, name, ref64[name]), LR.slices(kind, name, ref32[name])):
            err = LR.rel_l2(gs, rs)
            torch_err = LR.rel_l2(ts, rs)
            bound = max(LR.F32_FACTOR * torch_err, LR.F32_FLOOR) if route.fmt == "f32" else LR.BOUND[route.fmt]
            print(f"  {tag} {name}.{label}: kernel {err:.2e}  bound {bound:.2e}  torch-f32 {torch_err:.2e}")
            if err / bound > worst[0]:
                worst = (err / bound, f"{tag} {name}.{label}", err, bound)
            if not err < bound:
                failures.append((tag, name, label, err, bound))
    MEASURED[key] = worst
    assert not failures, failures


def run_case(engine, scratch, gpu_device, kind, case, shape, routes, mode, variants, seed):
    from soccdpt_amd.lib import ROUTE_BITS
    engine.train_set_amp(LR.AMP_CODE[mode])
    route = routes[mode]
    h, d = make_inputs(kind, shape, mode, gpu_device, seed)
    N, C = (shape[1], shape[2]) if kind == "linear" else (shape[2], shape[3]) if kind == "conv3" else (shape[3], shape[4])
    refs = {}
    for v in variants:
        res = v.res and v.dX and kind != "conv_gen"
        if res not in refs:
            refs[res] = (references(kind, shape, h, res, torch.float64), references(kind, shape, h, res, torch.float32))
        got, path, _ = call(engine, scratch, kind, shape, d, v)
        want = expected_path(kind, N, C, route, v)
        names = lambda p: sorted(k for k, b in ROUTE_BITS.items() if p & b)
        assert path == want, f"{kind} {case} {mode} {v.name}: route {names(path)}, expected {names(want)}"
        check_values(kind, (kind, case, mode), mode, route, got, *refs[res], tag=f"{kind}/{case}/{mode}/{v.name}")
        again, path2, _ = call(engine, scratch, kind, shape, d, v)
        assert path2 == path
        for k in got:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{kind} {case} {mode} {v.name}: {k} differs between two calls"
    print(f"MEASURED {kind}/{case}/{mode}: route {route}, worst {MEASURED[(kind, case, mode)]}")
    return h, d


# ---------------- the tests ----------------
@pytest.mark.parametrize("mode", LR.FORMATS)
@pytest.mark.parametrize("case", [c for c in CONV3 if c != "a2"])
def test_conv3_bwd(engine, scratch, gpu_device, case, mode):
    shape, routes = CONV3[case]
    if case in CONV3_NO_DX:
        variants = [Variant("full", dX=False, stage=True, defer=True), Variant("bare", dX=False)]
    else:
        variants = [FULL, BARE] + ([DW_ONLY, DX_ONLY] if case in CONV3_EXTRA else [])
    run_case(engine, scratch, gpu_device, "conv3", case, shape, routes, mode, variants, seed=100 + sorted(CONV3).index(case))


@pytest.mark.parametrize("mode", LR.FORMATS)
def test_conv3_bwd_reuses_the_staged_input(engine, scratch, gpu_device, mode):
    """output_conv.0 and seg_head.0 share path_1: case a, then on the same scratch a second layer (N = 256, with a residual) over the same zero-bordered
    input with reuse_xt = 1.  Its result equals the same call made cold, bit for bit, and the float64 reference within the bounds."""
    engine.train_set_amp(LR.AMP_CODE[mode])
    shape1, routes1 = CONV3["a"]
    shape2, routes2 = CONV3["a2"]
    h1, d1 = make_inputs("conv3", shape1, mode, gpu_device, seed=100)
    h2, d2 = make_inputs("conv3", shape2, mode, gpu_device, seed=199, X=(h1["X"], d1["X"]))
    _, p1, need1 = call(engine, scratch, "conv3", shape1, d1, FULL)
    assert p1 == expected_path("conv3", shape1[2], shape1[3], routes1[mode], FULL)
    warm, pw, _ = call(engine, scratch, "conv3", shape2, d2, FULL, reuse_xt=True, fill=False, guard_from=need1)
    cold, pc, _ = call(engine, scratch, "conv3", shape2, d2, FULL)
    assert pw == pc == expected_path("conv3", shape2[2], shape2[3], routes2[mode], FULL)
    for k in cold:
        assert torch.equal(warm[k].view(torch.int32), cold[k].view(torch.int32)), f"{k}: the reused staging gives other bits than a cold call"
    ref64, ref32 = (references("conv3", shape2, h2, True, dt) for dt in (torch.float64, torch.float32))
    check_values("conv3", ("conv3", "a2", mode), mode, routes2[mode], warm, ref64, ref32, tag=f"conv3/a2/{mode}/reuse_xt")
    print(f"MEASURED conv3/a2/{mode}: route {routes2[mode]}, worst {MEASURED[('conv3', 'a2', mode)]}")
    # without a matching previous call the flag is refused
    h3, d3 = make_inputs("conv3", shape2, mode, gpu_device, seed=198)
    with pytest.raises(RuntimeError, match="reuse_xt"):
        call(engine, scratch, "conv3", shape2, d3, FULL, reuse_xt=True)


@pytest.mark.parametrize("mode", LR.FORMATS)
@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_bwd(engine, scratch, gpu_device, case, mode):
    shape, routes = LINEAR[case]
    bare = Variant("bare", dX=False) if case in LINEAR_BARE_NO_DX else BARE
    variants = [FULL, bare] + ([DW_ONLY, DX_ONLY] if case in LINEAR_EXTRA else [])
    run_case(engine, scratch, gpu_device, "linear", case, shape, routes, mode, variants, seed=200 + list(LINEAR).index(case))


@pytest.mark.parametrize("mode", LR.FORMATS)
@pytest.mark.parametrize("case", list(CONV_GEN))
def test_conv_gen_bwd(engine, scratch, gpu_device, case, mode):
    shape, routes = CONV_GEN[case]
    run_case(engine, scratch, gpu_device, "conv_gen", case, shape, routes, mode, [FULL, BARE], seed=300 + list(CONV_GEN).index(case))


def test_bad_arguments_are_errors(engine, scratch, gpu_device):
    from soccdpt_amd.lib import TrainLayerBwdArgs, op_train_layer_bwd, op_train_layer_bwd_scratch_bytes
    engine.train_set_amp(0)
    t = Guarded((64, 64), gpu_device, torch.zeros(64, 64))
    o = Guarded((64, 64), gpu_device)

    def args(**kw):
        a = TrainLayerBwdArgs(kind=0, M=64, N=64, C=64)
        a.dY = a.X = a.W = t.ptr()
        a.dW = o.ptr()
        for k, val in kw.items():
            setattr(a, k, val)
        return a
    good = args()
    need = op_train_layer_bwd_scratch_bytes(good)
    buf = scratch.take(need)
    for bad in (args(kind=3), args(N=0), args(C=30), args(M=0), args(dY=None), args(dW=None), args(dX_res=t.ptr()), args(reuse_xt=1),
                args(N=48, dX=o.ptr()), args(kind=1, B=0, r=4), args(kind=1, B=1, r=0), args(kind=2, B=1, Hi=5, Ho=3, stride=2, pad=0),
                args(kind=2, B=1, Hi=6, Ho=6, stride=2, pad=1), args(kind=2, B=1, Hi=6, Ho=6, stride=1, pad=1, dX_res=t.ptr(), dX=o.ptr())):
        with pytest.raises(RuntimeError):
            op_train_layer_bwd_scratch_bytes(bad)
        with pytest.raises(RuntimeError):
            op_train_layer_bwd(engine, bad, buf[:need])
    with pytest.raises(RuntimeError, match="too small"):
        op_train_layer_bwd(engine, good, buf[:need - 256])
    with pytest.raises(RuntimeError, match="aligned"):
        op_train_layer_bwd(engine, good, buf[128:128 + need])
    torch.cuda.synchronize()
    assert o.untouched()


def test_every_route_was_reached():
    """The union of the routes this module's calls reported covers every SOCCDPT_ROUTE_* bit: a route added to the library without a case here, or a
    case that silently falls back (its bits then missing), fails.  Needs the whole module to have run."""
    from soccdpt_amd.lib import ROUTE_ALL, ROUTE_BITS
    assert sum(ROUTE_BITS.values()) == ROUTE_ALL and len(set(ROUTE_BITS.values())) == len(ROUTE_BITS)
    seen = 0
    for p in _SEEN:
        assert p & ~ROUTE_ALL == 0, hex(p)
        seen |= p
    missing = sorted(k for k, b in ROUTE_BITS.items() if not seen & b)
    assert not missing, f"routes never reached: {missing}"
