"""GPU: the separable patch build of csrc/depth_tail.hip (a thread walks down a patch column and lerps each source row once) at its edges.

* Bit-equality with the build it replaced: tests/golden/depth_tail_parent.npz holds soccdpt_op_depth_tail's output from a library built at the
  parent commit (tests/tools/make_golden_depth_tail.py) for both formats at three small shapes; the inputs are re-made from their seeds and a
  checksum of their bit patterns must match the recorded one before the outputs are compared.
* The float64 element-wise bound of tests/fused_refs.py at the same shapes and one more, every tile, three runs bitwise equal.
Each check prints its worst element with -s."""
import os

import numpy as np
import pytest
import torch

from tests import depth_tail_build_refs as D
from tests import fused_refs as FR

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fmt", D.FORMATS)
@pytest.mark.parametrize("B,h,w", D.PARENT_SHAPES)
def test_patch_build_gives_the_parent_commits_bits(gpu_device, golden_dir, fmt, B, h, w):
    gold = np.load(os.path.join(golden_dir, D.GOLDEN_FILE))
    k = D.key(fmt, B, h, w)
    inp = D.inputs(B, h, w, fmt)
    have, want = int(D.input_checksum(*inp, fmt)), int(gold[k + ".in"])
    assert have == want, f"{k}: the seeded inputs are not the recorded ones (checksum {have:#x}, recorded {want:#x}); the comparison would mean nothing"
    got = D.bits(D.launch(inp, fmt, B, h, w, gpu_device))
    ref = gold[k + ".out"]
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    print(f"depth_tail {k}: {got.size} words, {len(bad)} differ from the parent commit's")
    if len(bad):
        t = tuple(bad[0])
        raise AssertionError(f"{k}: {len(bad)} of {got.size} output words differ from the parent commit's; first at (b, y, x) = {t}: "
                             f"{got[t]:#010x} vs {ref[t]:#010x} ({got.view(np.float32)[t]!r} vs {ref.view(np.float32)[t]!r})")


@pytest.mark.parametrize("fmt", D.FORMATS)
@pytest.mark.parametrize("B,h,w", D.BOUND_SHAPES)
def test_patch_build_within_the_float64_bound(gpu_device, fmt, B, h, w):
    inp = D.inputs(B, h, w, fmt)
    n, tx_n, ty_n = FR.depth_tail_tiles(B, h, w)
    got = D.launch(inp, fmt, B, h, w, gpu_device)
    assert bool(torch.isfinite(got).all()), "depth tail left output pixels unwritten"
    tiles = torch.arange(n)
    ref, bnd = FR.depth_tail_ref(*inp, fmt, tiles)
    ratio = FR.check_bound(FR.gather_tiles(got, tiles, tx_n, ty_n), ref, bnd, f"depth_tail {D.key(fmt, B, h, w)}")
    print(f"depth_tail {D.key(fmt, B, h, w)} (all {n} tiles): worst error / bound = {ratio:.3g}")
