"""GPU: the fused training criterion (csrc/loss.hip) through the C entry soccdpt_training_loss, every element of d_inv and d_seg, the three
loss values and every image's scale / shift against the float64 reference of tests/loss_refs.py.

Bound, per slice (tests/loss_refs.compare): |kernel - ref64| <= max(3 x max |torch f32 - ref64|, 8 * 2^-24 * max |ref64|), the yardstick being
oracle/loss_ref.py in float32 on the same inputs.  No element is excluded: the inputs are pinned (no sign() of the gradient-matching stencil and
no clamp decision can differ between float32 and float64; asserted on the CPU by tests/test_loss_refs.py, which also shows the bound rejecting
eleven planted faults).  tests/test_loss_gpu.py keeps the golden and the full camera resolution under its own, looser tolerance.

Per call: the scratch is exactly soccdpt_loss_scratch_bytes bytes of 0xFF, every output 0xFF (NaN), a 4 KB 0xFF guard sits behind the scratch,
every operand and every output; afterwards the outputs are finite, guards and operands untouched, a second call gives the same bits in d_inv /
d_seg and scalars within 2 float32 ulp (the order of the float64 atomics is free).  A HIP error ends the session.

Cases (tests/loss_refs.CASES; B, C, h x w -> H x W): the shapes are the smallest at which each edge exists -- non-integer ratios with h != w and
odd H, W; exact ratio 8; ratio 33.75 / 16.75 (the footprint scan windows); the launcher's minimum 2 x 2 with every tap clamped; 1 x 9 and 1 x 1
images (no vertical / no neighbours, M_k of one point); down-sampling (source cells without footprint) in both and in one axis; more than 65536
pixels and more than 262144 seg cells (the grid-stride loops).  Variants on the first shape: scale / shift off, alpha = 0, weights (0.3, 0.7)
and (0, 1), an empty depth mask in the middle image of three, M_3 = 0, an image with exactly two and with exactly one valid pixel, an empty seg
mask, one class masked out, class probabilities of exactly 0 and 1 (the -100 log clamp, the 1e-12 denominator), 1 - 2^-24 and 2^-30 under both
targets, a positive network output (no clamp).

Measured on MI355X: per case the slice with the largest error / bound, with torch's float32 error on that slice and the bound it gives
(every slice is printed with -s).  Where kernel and torch agree to the digit, both returned the same float32 number.

    case                 worst slice                  kernel     torch f32  bound
    8x12-37x53           scale.img1                   3.0e-08    3.0e-08  8.9e-08
    8x8-64x64            d_seg.img1.class1.last       8.3e-09    1.8e-08  5.4e-08
    4x4-135x67           loss                         7.3e-08    4.7e-08  2.8e-07
    2x2-9x7              d_inv.img0.border            1.7e-08    1.7e-08  5.0e-08
    2x2-1x9              d_inv.img0.border            1.7e-08    1.9e-08  5.6e-08
    2x2-1x1              d_seg.img0.class0.rest       1.0e-06    1.0e-06  1.4e-05
    2x2-1x1-positive     d_seg.img0.class0.rest       1.0e-06    1.0e-06  1.4e-05
    24x16-20x13          d_inv.img0.clampfoot         2.6e-09    3.5e-09  1.1e-08
    16x8-12x40           d_seg.img0.class2.rest       7.1e-07    2.3e-07  2.8e-06
    16x16-258x257        loss                         7.1e-08    7.1e-08  3.1e-07
    300x300-40x56        d_inv.img0.border            4.8e-10    4.9e-10  1.5e-09
    noss                 d_inv.img1.clampfoot         6.5e-09    7.6e-09  2.3e-08
    alpha0               scale.img1                   3.0e-08    3.0e-08  8.9e-08
    w37                  scale.img1                   3.0e-08    3.0e-08  8.9e-08
    m3_zero              d_seg.img1.class2.rest       9.4e-08    8.5e-08  3.5e-07
    two_pixels           scale.img1                   1.2e-07    1.2e-07  3.5e-07
    class_off            scale.img1                   3.0e-08    3.0e-08  8.9e-08
    all_positive         d_seg.img1.class2.rest       9.4e-08    8.5e-08  3.5e-07
    w01                  scale.img1                   3.0e-08    3.0e-08  8.9e-08
    mid_empty            d_seg.img2.class1.last       5.1e-09    5.1e-09  1.7e-08
    one_pixel            d_seg.img1.class2.rest       9.4e-08    8.5e-08  3.5e-07
    seg_empty            scale.img1                   3.0e-08    3.0e-08  8.9e-08
    seg_sat              scale.img1                   3.0e-08    3.0e-08  8.9e-08

What these tests found (the figures before the change, same machine): with one valid pixel the kernel "fitted" it -- scale 1.67 / shift 0.61
(one_pixel, image 1), 0.88 / 0.037 (2x2-1x1-positive) and 1.4e7 / 0.32 on a clamped pixel (2x2-1x1) where the reference gives 0 / 0, loss_disp
off by 1.6e-2; solve_image now calls fewer than two valid pixels singular.  d_seg left its bound where the targets of a footprint are mixed
(8x8-64x64: 5.8e-7 against a bound of 3.5e-7, an f32 running sum over 64 pixels); the footprint sum is kept in f64.  The least-squares sums took
f32-rounded products p * p and p * y; they are exact f64 products now.
"""
import numpy as np
import pytest
import torch

from tests import loss_refs as R

pytestmark = pytest.mark.gpu

GUARD_BYTES = 4096
KEYS = ("inv", "seg", "y_disp", "mask_disp", "y_seg", "mask_seg")


class Buf:
    """A device tensor with a 4 KB guard of 0xFF bytes directly behind it; without a value it is 0xFF bytes itself (NaN in f32)."""

    def __init__(self, shape, dtype, dev, value=None):
        n = int(np.prod(shape))
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.raw[: self.nbytes].view(dtype).view(tuple(shape))
        if value is not None:
            self.t.copy_(value.to(dtype))

    def ptr(self):
        return self.raw.data_ptr()

    def guard_untouched(self):
        return bool((self.raw[self.nbytes:] == 0xFF).all())


def call(name, dev):
    """One soccdpt_training_loss on buffers of its own -> the results on the host."""
    from soccdpt_amd.lib import _call, load_library
    c, ins = R.CASES[name], R.build(name)
    host = {k: (ins[k].to(torch.uint8) if ins[k].dtype == torch.bool else ins[k]) for k in KEYS}
    ops = {k: Buf(v.shape, v.dtype, dev, v) for k, v in host.items()}
    outs = {"out": Buf((3 + 2 * c.B,), torch.float32, dev), "d_inv": Buf((c.B, c.h, c.w), torch.float32, dev), "d_seg": Buf((c.B, c.C, c.h, c.w), torch.float32, dev)}
    need = int(load_library().soccdpt_loss_scratch_bytes(c.B, c.H, c.W, c.h, c.w))
    scratch = Buf((need,), torch.uint8, dev)
    _call("soccdpt_training_loss", c.B, c.H, c.W, c.h, c.w, c.C, int(c.compute_ss), float(c.alpha), float(c.w_d), float(c.w_s),
          *[ops[k].ptr() for k in KEYS], outs["out"].ptr(), outs["d_inv"].ptr(), outs["d_seg"].ptr(), scratch.ptr(), device=dev)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_training_loss ({name}): {e}", returncode=3)
    assert scratch.guard_untouched(), "the guard behind the scratch was written"
    for k, b in ops.items():
        assert b.guard_untouched(), f"the guard behind operand {k} was written"
        assert torch.equal(b.t.cpu(), host[k]), f"operand {k} was written"
    got = {}
    for k, b in outs.items():
        assert b.guard_untouched(), f"the guard behind {k} was written"
        got[k] = b.t.cpu()
        assert bool(torch.isfinite(got[k]).all()), f"{k} is not finite everywhere: {int((~torch.isfinite(got[k])).sum())} of {got[k].numel()} elements"
    out = got.pop("out")
    got.update(loss=out[0], loss_disp=out[1], loss_seg=out[2], scale=out[3::2], shift=out[4::2], scalars=out)
    return got


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def within_ulps(a, b, n=2):
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    return bool((np.abs(a.astype(np.float64) - b.astype(np.float64)) <= n * np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)).all())


def run(name, dev):
    """Two calls with the per-call checks, every slice held to the bound (and printed)."""
    got, again = call(name, dev), call(name, dev)
    assert same_bits(got["d_inv"], again["d_inv"]) and same_bits(got["d_seg"], again["d_seg"]), f"{name}: the gradients differ between two calls"
    assert within_ulps(got["scalars"], again["scalars"]), (got["scalars"], again["scalars"])
    rows = R.compare(name, again)
    for r in rows:
        print(f"  {name} {r.label}: kernel {r.err:.2e}  torch-f32 {r.torch_err:.2e}  bound {r.bound:.2e}{'' if r.ok else '  OUTSIDE'}")
    w = R.worst(rows)
    print(f"MEASURED {name:<20} {w.label:<28} {w.err:.1e}    {w.torch_err:.1e}  {w.bound:.1e}")
    failures = [r for r in rows if not r.ok]
    assert not failures, failures
    return again


SHAPES = [n for n in R.CASES if n[0].isdigit()]
PLAIN_VARIANTS = ["noss", "alpha0", "w37", "m3_zero", "two_pixels", "class_off", "all_positive"]


@pytest.mark.parametrize("name", SHAPES)
def test_shapes(gpu_device, name):
    run(name, gpu_device)


@pytest.mark.parametrize("name", PLAIN_VARIANTS)
def test_variants(gpu_device, name):
    got = run(name, gpu_device)
    if name == "noss":
        assert got["scale"].tolist() == [1.0, 1.0] and got["shift"].tolist() == [0.0, 0.0]


def test_zero_depth_weight(gpu_device):
    got = run("w01", gpu_device)
    assert float(got["d_inv"].abs().max()) == 0.0 and float(got["loss"]) == float(got["loss_seg"])


def test_empty_depth_mask_in_the_middle_image(gpu_device):
    got = run("mid_empty", gpu_device)
    assert float(got["scale"][1]) == 0.0 and float(got["shift"][1]) == 0.0
    assert float(got["d_inv"][1].abs().max()) == 0.0
    assert float(got["d_inv"][0].abs().max()) > 0.0 and float(got["d_inv"][2].abs().max()) > 0.0


def test_one_valid_pixel(gpu_device):
    """With fewer than two valid pixels the least-squares system is singular in any precision: scale = shift = 0, the data term is
    y^2 / (2 M), nothing flows through the solve."""
    got = run("one_pixel", gpu_device)
    assert float(got["scale"][1]) == 0.0 and float(got["shift"][1]) == 0.0


def test_empty_seg_mask(gpu_device):
    got = run("seg_empty", gpu_device)
    assert float(got["loss_seg"]) == 0.0 and float(got["d_seg"].abs().max()) == 0.0
    assert float(got["loss"]) == float(torch.tensor(R.CASES["seg_empty"].w_d) * got["loss_disp"])


def test_saturated_class_probabilities(gpu_device):
    got = run("seg_sat", gpu_device)
    c = R.CASES["seg_sat"]
    n = float(R.build("seg_sat")["mask_seg"].sum())
    quantum = 1e12 * c.w_s / n                                  # one footprint pixel at q = 0 under target 1 (or q = 1 under target 0)
    zero_row, one_row = [r for r, t in R.SAT_ROWS.items() if t == 0.0][0], [r for r, t in R.SAT_ROWS.items() if t == 1.0][0]
    for b in range(c.B):
        assert float(got["d_seg"][b, 0, zero_row, 0]) == 0.0 and float(got["d_seg"][b, 0, one_row, 1]) == 0.0       # q == target: (q - t) = 0
        assert float(got["d_seg"][b, 0, zero_row, 1]) > quantum and float(got["d_seg"][b, 0, one_row, 0]) < -quantum


def test_python_layer_gives_the_bits_of_the_direct_call(gpu_device):
    from soccdpt_amd.utils.loss import training_loss
    name = "w37"
    c, ins = R.CASES[name], R.build(name)
    direct = call(name, gpu_device)
    r = training_loss(*[ins[k].to(gpu_device) for k in KEYS], loss_depth_w=c.w_d, loss_seg_w=c.w_s, alpha=c.alpha, compute_scale_and_shift=c.compute_ss)
    torch.cuda.synchronize()
    assert same_bits(r["d_inv"].cpu(), direct["d_inv"]) and same_bits(r["d_seg"].cpu(), direct["d_seg"])
    for k in ("loss", "loss_disp", "loss_seg", "scale", "shift"):
        assert within_ulps(r[k].cpu().reshape(-1), direct[k].reshape(-1)), k
