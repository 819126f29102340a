"""GPU: the two launchers dpt_swin2_large_384 widened, one launch at a time through soccdpt_op_fwd_aux, against float64 with the a-priori bounds of
tests/fwd_aux_refs.py (cases and references: tests/swin_large_refs.py; harness -- 0xFF outputs, guards, untouched operands and halo rings, finiteness, a
second call with the same bits -- tests/test_fwd_aux_gpu.py's run_twice).

* patch_embed at C0 = 192: the three-channels-per-lane instantiation, every output format, the prepared filter [48][192] bit for bit the transposed input;
* ln_residual at C = 1536 (six float4 groups per lane) in every form of the row function, and once at C = 1280 (five);
* the widths between and beyond stay refusals that launch nothing;
* one existing shape of each launcher gives the bits the library gave before the change (tests/golden/swin_large_parent_kernels.npz).
Every test prints its worst element with -s."""
import os

import numpy as np
import pytest
import torch

from tests import fused_refs as FR
from tests import fwd_aux_refs as R
from tests import swin_large_refs as L
from tests.test_fwd_aux_gpu import check_f32, make_args, run, run_twice, same_bits
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


@pytest.mark.parametrize("case,fmt", L.PATCH_RUNS, ids=lambda v: str(v))
def test_patch_embed_c192(dev, case, fmt):
    inp = L.build_patch(case)
    ref = L.ref_patch(inp, L.PATCH_LD)
    got, _ = run_twice(L.call_patch(case, fmt, inp, L.PATCH_LD), dev)
    label = f"patch_embed {case} fmt {fmt}"
    same_bits(got["wT"], ref["wT"].float(), "the prepared weight [48][192]")
    check_f32(label, "xf", got["xf"], *ref["xf"])
    if fmt is not None:
        R.check_op(got["xb"], fmt, got["xf"].shape, None, None, f"{label} xb", twin=got["xf"])


@pytest.mark.parametrize("case", list(L.LN_CASES))
def test_ln_residual_wide(dev, case):
    c = L.LN_CASES[case]
    inp = L.build_ln(c)
    got, path = run_twice(L.call_ln(c, inp), dev)
    assert path == c.path, f"{case}: kernel {path:#x}, expected {c.path:#x}"
    label = f"ln_residual {case}"
    check_f32(label, "xf", got["xf"], *L.ref_ln(c, inp))
    B = c.M // (c.res * c.res) if c.res else 0
    if c.xb:     # the operand copy: RN16 / x3 of the kernel's own xf, for merge in the PatchMerging layout (a permutation: bitwise)
        twin = L.merge_layout(got["xf"], B, c.res) if c.merge else got["xf"]
        R.check_op(got["xb"], c.fmt, twin.shape, None, None, f"{label} xb", twin=twin)
        if c.merge:
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


def bad_calls():
    C, T, N, fl = R.Call, True, None, R.flags_of
    yield "patch_embed: C0 = 160 (between the two instantiations)", C("patch_embed", [1, 32, 160], ins=[T] * 5, outs=[T, N, T]), {}
    yield "patch_embed: C0 = 256", C("patch_embed", [1, 32, 256], ins=[T] * 5, outs=[T, N, T]), {}
    yield "ln_residual: C = 1792", C("ln_residual", [5, 1792, 0, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, T, N, N]), {}
    yield "ln_residual: C = 1536, y off by 4 bytes", C("ln_residual", [5, 1536, 0, 0], fl(1, 0), ins=[T, T, T, N], outs=[T, T, N, N]), {"in0": 4}


def test_widths_not_instantiated_launch_nothing(dev):
    """In the manner of test_fwd_aux_gpu.test_bad_arguments_launch_nothing: an error that names the entry, no kernel launched, the arena still 0xFF."""
    from soccdpt_amd.lib import load_library, op_fwd_aux
    lib = load_library()
    SLOT = 1 << 16
    arena = Buf((16 * SLOT,), torch.uint8, dev)
    torch.cuda.synchronize()
    before = int(lib.soccdpt_launch_counter())
    n = 0
    for label, call, off in bad_calls():
        ins = [None if t is None else arena.ptr() + SLOT * i + off.get(f"in{i}", 0) for i, t in enumerate(call.ins)]
        outs = [None if t is None else arena.ptr() + SLOT * (8 + i) + off.get(f"out{i}", 0) for i, t in enumerate(call.outs)]
        with pytest.raises(RuntimeError, match="soccdpt_op_fwd_aux"):
            op_fwd_aux(make_args(call, ins, outs), dev)
            pytest.fail(f"accepted: {label}")
        torch.cuda.synchronize()
        assert int(lib.soccdpt_launch_counter()) == before, f"{label}: a refused call launched a kernel"
        assert bool((arena.raw == 0xFF).all()), f"{label}: a refused call wrote"
        n += 1
    assert n == 4
    # and the accepted width launches: the filter preparation and the kernel
    inp = L.build_patch("1x32x192")
    run(L.call_patch("1x32x192", None, inp, L.PATCH_LD), dev)
    assert int(lib.soccdpt_launch_counter()) == before + 2


def test_existing_instantiations_give_the_parent_commits_bits(dev, golden_dir):
    """patch_embed 1x32x96 (two channels per lane) and ln_residual c1024_m7 (four float4 groups): every output word equals what the library built from the
    commit before the launchers were widened wrote for the same call."""
    gold = np.load(os.path.join(golden_dir, L.GOLDEN_FILE))
    seen = 0
    for label, call in L.parent_calls():
        got, _ = run_twice(call, dev)
        for name, t in got.items():
            want = torch.from_numpy(gold[f"{label}.{name}"])
            same_bits(L.bits(t), want, f"{label} {name} vs the parent commit's library")
            seen += 1
    assert seen == 5 and len(gold.files) == 5
