"""What tests/test_depth_tail_build_gpu.py and tests/tools/make_golden_depth_tail.py share: the shapes at which the separable patch build of
csrc/depth_tail.hip is held to the bits of the build it replaced, their seeded inputs (tests.fused_refs.depth_tail_inputs), a checksum of the
inputs' bit patterns and the launch itself.

tests/golden/depth_tail_parent.npz holds, per format and shape, `<fmt>.<B>x<h>x<w>.out` (uint32 view of the f32 output [B][2h][2w] of
soccdpt_op_depth_tail from a library built at the commit BEFORE the separable build) and `<fmt>.<B>x<h>x<w>.in` (uint64 checksum of the inputs)."""
from __future__ import annotations

import zlib

import numpy as np
import torch

from tests import fused_refs as FR

GOLDEN_FILE = "depth_tail_parent.npz"
FORMATS = ("bf16", "f16")
DT = {"bf16": torch.bfloat16, "f16": torch.float16}

# (B, h, w) of the low-resolution map; the output is B x 2h x 2w in 8 x 16 tiles
PARENT_SHAPES = [
    (1, 4, 8),      # one tile: fewer source rows than the window holds, all four halo sides outside the image
    (2, 4, 16),     # two tiles side by side and a frame boundary: the clamp must not read the next frame's rows
    (1, 16, 24),    # an interior tile with all eight neighbours; four tile rows whose first source rows lie at different phases
]
BOUND_SHAPES = PARENT_SHAPES + [
    (3, 20, 40),    # "same source row or the next" shifts its pattern inside the image (five tile rows, five tile columns, three frames)
]


def seed_of(B, h, w):
    return 7000 + B * 1000 + 31 * h + w


def key(fmt, B, h, w):
    return f"{fmt}.{B}x{h}x{w}"


def inputs(B, h, w, fmt):
    return FR.depth_tail_inputs(B, h, w, fmt, seed=seed_of(B, h, w))


def input_checksum(d1, wt, bias, w4, b4, fmt) -> np.uint64:
    """CRC-32 of the 16-bit patterns of d1 and wt (high word) and of the f32 patterns of bias, w4 and b4 (low word)."""
    hi = zlib.crc32(d1.to(DT[fmt]).contiguous().view(torch.int16).numpy().tobytes())
    hi = zlib.crc32(wt.to(DT[fmt]).contiguous().view(torch.int16).numpy().tobytes(), hi)
    lo = zlib.crc32(bias.float().numpy().tobytes())
    lo = zlib.crc32(w4.float().numpy().tobytes(), lo)
    lo = zlib.crc32(np.float32(b4).tobytes(), lo)
    return np.uint64((hi << 32) | lo)


def launch(inp, fmt, B, h, w, dev, runs=3):
    """op_depth_tail on a NaN-filled output, `runs` times, every run bitwise equal to the first; returns the CPU copy [B][2h][2w]."""
    from soccdpt_amd import lib
    d1, wt, bias, w4, b4 = inp
    d1_d, wt_d = d1.to(DT[fmt]).contiguous().to(dev), wt.to(DT[fmt]).contiguous().to(dev)
    bias_d, w4_d = bias.float().to(dev), w4.float().to(dev)
    prec = {"bf16": lib.PREC_BF16, "f16": lib.PREC_F16}[fmt]
    first = None
    for _ in range(runs):
        out = torch.full((B, 2 * h, 2 * w), float("nan"), device=dev)
        lib.op_depth_tail(d1_d, wt_d, bias_d, w4_d, b4, out, B, h, w, precision=prec)
        torch.cuda.synchronize()
        got = out.cpu()
        if first is None:
            first = got
        else:
            assert torch.equal(first.view(torch.int32), got.view(torch.int32)), "a rerun changed bits"
    return first


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)
