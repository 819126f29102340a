"""GPU: the projection stage away from the default geometry.  Every form launch_project (csrc/projection.hip) chooses between, the two-rotation
path, non-default grids, h != w, down-sampling, the per-frame grids (csrc/occ_frames.hip), the grid plumbing, soccdpt_project_backward
(csrc/upsample_bwd.hip) and the Python mirror, at the cameras / maps / grids / rotations of tests/projection_geometries.py -- bit-exact against
the C oracle (which tests/test_projection_geometries_cpu.py holds equal to the reference's own torch ops at the same rows), every output a
slice of a larger sentinel-filled tensor whose guard bands must come back unchanged."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import cref, soccdpt_ref as R
from tests import projection_geometries as PG

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. eng.project ----
@pytest.mark.parametrize("case_id", PG.CASE_IDS)
def test_project_bit_exact(gpu_device, case_id):
    """inv_up, seg_up, points and the packed union grid equal cref.project bit for bit; nothing is stored outside the outputs."""
    geo = PG.case_inputs(case_id)[0]
    bad = PG.check_project_case(gpu_device, case_id, expect_form=geo.form)
    print(f"{case_id}: {geo.form}, oracle sets {PG.popcount(PG.case_oracle(case_id)['occ_bits'])} bits")
    assert not bad, bad


@pytest.mark.parametrize("case_id", ["G3", "G5"])
def test_project_optional_outputs(gpu_device, case_id):
    geo, inv, seg = PG.case_inputs(case_id)
    ref = PG.case_oracle(case_id)
    eng = PG.make_engine(gpu_device, geo)
    for want in (("occ_bits",), ("inv_up", "points")):
        out = PG.run_project(eng, geo, inv, seg, gpu_device, want=want)
        assert set(out) == set(want)
        bad = PG.project_mismatches(out, ref)
        assert not bad, (want, bad)
    eng0 = PG.make_engine(gpu_device, geo, compute_occ=False)
    out = PG.run_project(eng0, geo, inv, seg, gpu_device, want=("inv_up", "seg_up", "points"))
    bad = PG.project_mismatches(out, ref)
    assert not bad, bad


# ---- b. eng.voxelise_frames on the inv_up of (a) ----
@pytest.mark.parametrize("case_id", PG.CASE_IDS)
def test_voxelise_frames_rows(gpu_device, case_id):
    geo, inv, seg = PG.case_inputs(case_id)
    eng = PG.make_engine(gpu_device, geo)
    out = PG.run_project(eng, geo, inv, seg, gpu_device, want=("inv_up", "occ_bits"))
    rows = PG.Guarded((geo.B, eng.occ_words()), torch.int32, gpu_device, fill=-1)
    eng.voxelise_frames(out["inv_up"].t, seg.to(gpu_device), rows.t, clear_bits=True)
    torch.cuda.synchronize()
    got, want = PG.np_bits(rows.t), PG.case_oracle_frames(case_id)
    for b in range(geo.B):
        assert np.array_equal(got[b], want[b]), f"frame {b}: {int((got[b] != want[b]).sum())} words differ from the single-frame oracle"
    assert np.array_equal(np.bitwise_or.reduce(got, axis=0), PG.case_oracle(case_id)["occ_bits"])
    assert np.array_equal(np.bitwise_or.reduce(got, axis=0), PG.np_bits(out["occ_bits"].t))
    assert rows.guards_intact() and out["inv_up"].guards_intact()


# ---- c. grid plumbing at the table's grids ----
@pytest.mark.parametrize("case_id", ["G1", "G2", "G4", "G5", "G6"])
def test_grid_plumbing(gpu_device, case_id):
    """occ_expand / occ_expand_frames / occ_zero + occ_set / occ_or against the unpacked oracle bits.  Cell counts that are no multiple of 32
    (G5: 5040) are refused by the expansions, odd ones (G6: 14553) by occ_zero as well, without a store; occ_set ignores padding bits."""
    geo = PG.case_inputs(case_id)[0]
    dev, B = gpu_device, geo.B
    eng = PG.make_engine(dev, geo)
    nwords = (geo.ncell + 31) // 32
    assert eng.occ_words() == nwords == math.ceil(geo.ncell / 32)
    union, frames = PG.case_oracle(case_id)["occ_bits"], PG.case_oracle_frames(case_id)
    dense = PG.unpack(union, geo)
    t_union = torch.from_numpy(union.view(np.int32).copy()).to(dev)
    t_frames = torch.from_numpy(frames.view(np.int32).copy()).to(dev)
    shape = (B,) + geo.grid + (3,)

    occ = PG.Guarded(shape, torch.float32, dev, fill=PG.F_SENTINEL)
    occ_f = PG.Guarded(shape, torch.float32, dev, fill=PG.F_SENTINEL)
    if geo.ncell % 32 == 0:
        eng.occ_expand(t_union, B, occ.t)
        eng.occ_expand_frames(t_frames, B, occ_f.t)
        torch.cuda.synchronize()
        for b in range(B):
            assert np.array_equal(occ.t[b].cpu().numpy(), dense)
            assert np.array_equal(occ_f.t[b].cpu().numpy(), PG.unpack(frames[b], geo))
        assert occ.guards_intact() and occ_f.guards_intact()
    else:
        with pytest.raises(RuntimeError, match="multiple of 32"):
            eng.occ_expand(t_union, B, occ.t)
        with pytest.raises(RuntimeError, match="multiple of 32"):
            eng.occ_expand_frames(t_frames, B, occ_f.t)
        torch.cuda.synchronize()
        assert occ.untouched() and occ_f.untouched()

    # occ_zero + occ_set (the multi-GPU path's two halves of occ_expand), the words' padding bits set
    occ2 = PG.Guarded(shape, torch.float32, dev, fill=7.0)
    if geo.ncell % 4 == 0:
        eng.occ_zero(B, occ2.t)
    else:
        before = occ2.whole.clone()
        with pytest.raises(RuntimeError, match="multiple of 4"):
            eng.occ_zero(B, occ2.t)
        torch.cuda.synchronize()
        assert torch.equal(occ2.whole, before)
        occ2.t.zero_()
    padded = union.copy()
    if geo.ncell % 32:
        padded[-1] |= np.uint32((0xFFFFFFFF << (geo.ncell % 32)) & 0xFFFFFFFF)
        assert PG.popcount(padded) == PG.popcount(union) + 32 - geo.ncell % 32
    eng.occ_set(torch.from_numpy(padded.view(np.int32).copy()).to(dev), B, occ2.t)
    torch.cuda.synchronize()
    for b in range(B):
        assert np.array_equal(occ2.t[b].cpu().numpy(), dense)
    assert occ2.guards_intact()
    if geo.ncell % 32:   # every bit of every word set: exactly the ncell cells of each row become 1
        occ3 = PG.Guarded(shape, torch.float32, dev, fill=0.0)
        eng.occ_set(torch.full((nwords,), -1, dtype=torch.int32, device=dev), B, occ3.t)
        torch.cuda.synchronize()
        assert bool((occ3.t == 1.0).all()) and occ3.guards_intact()

    # occ_or: frame 0's grid |= every frame's
    dst = PG.Guarded((nwords,), torch.int32, dev)
    dst.t.copy_(t_frames[0])
    eng.occ_or(dst.t, t_frames, B)
    torch.cuda.synchronize()
    assert np.array_equal(PG.np_bits(dst.t), union) and dst.guards_intact()


# ---- d. eng.project_backward ----
@pytest.mark.parametrize("clamped", [False, True])
@pytest.mark.parametrize("gid", ["G2", "G4", "G5", "G6"])
def test_project_backward_geometries(gpu_device, gid, clamped):
    """soccdpt_project_backward against float64 torch autograd through the same tail (PG.project_backward_reference, shared with
    test_autograd_bridge_gpu.py) at non-integer ratios, h != w and down-sampling, where a gather window computed from the scale factor could
    come out one row short.  Bounds: the larger of the 64^2 -> 1080p test's (d_inv 2e-5 unclamped / 2e-3 clamped, d_seg 2e-6) and 3 x the error
    of torch's own float32 autograd.  d_seg is a plain sum over a footprint, and the footprints partition the frame.
    Measured on an MI355X, relative L2 against float64 autograd (in brackets: torch's float32 autograd over the same function, on the CPU):
        row  map -> camera         d_inv unclamped       d_inv clamped         d_seg
        G2   96x96 -> 250x452      4.30e-07 (1.33e-06)   3.52e-06 (3.55e-06)   6.91e-08 (6.91e-08)
        G4   96x96 -> 120x200      3.98e-07 (2.03e-07)   4.15e-06 (4.17e-06)   3.50e-08 (3.50e-08)
        G5   64x48 -> 181x322      5.43e-07 (9.78e-07)   3.08e-06 (3.13e-06)   8.38e-08 (8.38e-08)
        G6   96x80 -> 40x64        5.58e-07 (4.95e-07)   3.81e-06 (3.82e-06)   0 (0): every footprint is one pixel or empty"""
    geo = PG.GEOMETRIES[gid]
    cam, (h, w), (Wc, Hc), B, dev = geo.cam, geo.map_hw, geo.cam_size, 2, gpu_device
    eng = PG.make_engine(dev, geo)
    g = torch.Generator().manual_seed(7)
    inv = torch.rand((B, h, w), generator=g) * 0.1 + 0.2
    if clamped:
        inv[0, h // 6:h // 6 + max(4, h // 8), w // 3:w // 3 + max(10, w // 5)] = -0.5
    seg = torch.rand((B, 3, h, w), generator=g)
    w1 = torch.randn((B, Hc, Wc), generator=g)
    w2 = torch.randn((B, 3, Hc, Wc), generator=g)
    w3 = None if clamped else torch.randn((B, Hc, Wc, 3), generator=g) * 1e-2
    inv_up = torch.empty((B, Hc, Wc), device=dev)
    eng.project(inv.to(dev), seg.to(dev), inv_up, None, None, None)
    d_inv, d_seg = eng.project_backward(inv_up, w1.to(dev), w2.to(dev), None if w3 is None else w3.to(dev), h, w)
    torch.cuda.synchronize()
    args = (inv, seg, Hc, Wc, cam.fx, cam.fy, cam.cx, cam.cy, geo.pc_scale, w1, w2, w3)
    r_inv, r_seg, raw = PG.project_backward_reference(*args)
    f_inv, f_seg, _ = PG.project_backward_reference(*args, dtype=torch.float32)
    e_inv, e_seg = PG.rel_l2(d_inv.cpu(), r_inv), PG.rel_l2(d_seg.cpu(), r_seg)
    t_inv, t_seg = PG.rel_l2(f_inv, r_inv), PG.rel_l2(f_seg, r_seg)
    print(f"project_backward {gid} ({PG.form_of(geo)}, {h}x{w} -> {Hc}x{Wc}, clamped={clamped}): rel L2 vs float64 autograd "
          f"d_inv {e_inv:.2e} (torch float32 {t_inv:.2e}), d_seg {e_seg:.2e} (torch float32 {t_seg:.2e})")
    if clamped:
        assert int((raw < 1e-8).sum()) > 0
    assert e_inv < max(2e-3 if clamped else 2e-5, 3.0 * t_inv), (e_inv, t_inv)
    assert e_seg < max(2e-6, 3.0 * t_seg), (e_seg, t_seg)
    # footprints partition the frame: per (b, c) the gradient mass is conserved, up to the float32 rounding of the kernel's sequential footprint sums
    # (k terms: at most (k - 1) * 2^-24 * sum |x| per footprint; the totals on both sides are taken in float64)
    k = (Hc // h + 1) * (Wc // w + 1)
    got = d_seg.cpu().double().sum(dim=(2, 3))
    want = w2.double().sum(dim=(2, 3))
    tol = k * 2.0 ** -24 * w2.double().abs().sum(dim=(2, 3))
    assert bool(((got - want).abs() <= tol).all()), ((got - want).abs().max(), tol.min())


# ---- e. the environment-selected forms ----
@pytest.mark.parametrize("switch,form", [("SOCCDPT_PROJECT_ROWS8", PG.ROWS8), ("SOCCDPT_PROJECT_ROWS1", PG.ROWS1)])
def test_project_env_selected_forms(gpu_device, switch, form):
    """SOCCDPT_PROJECT_ROWS8 / SOCCDPT_PROJECT_ROWS1 are read once per process: the check of (a) runs at G3 and at the default geometry in a
    fresh child, which exits non-zero on any mismatch."""
    for g in (PG.G3, PG.D0):
        assert PG.form_of(g, rows8=switch.endswith("ROWS8"), rows1=switch.endswith("ROWS1")) == form
    env = {k: v for k, v in os.environ.items() if k not in ("SOCCDPT_PROJECT_ROWS8", "SOCCDPT_PROJECT_ROWS1")}
    env[switch] = "1"
    r = subprocess.run([sys.executable, "-m", "tests.projection_geometries", "G3", "D0"], env=env, cwd=REPO, timeout=120, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count("bit-exact") == 2 and r.stdout.count(form) == 2


# ---- f. the Python mirror ----
@pytest.fixture(scope="module")
def synth_sd():
    from soccdpt_amd.utils.synth import synth_state_dict
    return synth_state_dict(alias_pretrained=True)


def _net(dev, geo, sd, per_frame):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"), **geo.calib)
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, grid_size=geo.grid, scale=geo.scale, correction_angle=geo.angles,
                   pc_scale=geo.pc_scale, pc_shift=geo.pc_shift, compute_occ=True, occupancy_per_frame=per_frame)
    m.load_state_dict(sd, strict=False)
    return m.eval().to(dev)


def _t_same(a, b):
    return PG.same(a.cpu().numpy(), b.numpy())


def test_python_mirror_non_default_constructor(gpu_device, synth_sd):
    """SOccDPT_V3 built with G3's camera file, grid, scale and rotation and the variant's pc constants: get_semantic_occupancy returns what the
    reference's torch ops return, bit for bit (the union in every row; B = 1 keeps the .squeeze() quirk); with occupancy_per_frame=True row b is the
    single-frame oracle and last_occ_bits the union."""
    geo, inv, seg = PG.case_inputs("G3pc")
    dev = gpu_device
    W, H = geo.cam_size
    uni = _net(dev, geo, synth_sd, False)
    assert (uni.width, uni.height) == geo.cam_size and float(uni.fx) == geo.cam.fx and float(uni.cy) == geo.cam.cy
    for B in (2, 1):
        i, s = inv[:B].contiguous(), seg[:B].contiguous()
        want = R.project(i, s, geo.cam, geo.cfg)
        got = uni.get_semantic_occupancy(i.to(dev), s.to(dev))
        torch.cuda.synchronize()
        assert tuple(got[1].shape) == ((B, 3, H, W) if B > 1 else (3, H, W)) == tuple(want[1].shape)
        assert tuple(got[3].shape) == (B,) + geo.grid + (3,)
        for k in range(4):
            assert tuple(got[k].shape) == tuple(want[k].shape) and _t_same(got[k], want[k]), (B, k)
        assert np.array_equal(PG.np_bits(uni.last_occ_bits), cref.pack_occ(want[3][0])) and uni.last_occ_frame_bits is None
        assert int(want[3][0].sum()) >= 300
    per = _net(dev, geo, synth_sd, True)
    want = R.project(inv, seg, geo.cam, geo.cfg)
    got = per.get_semantic_occupancy(inv.to(dev), seg.to(dev))
    torch.cuda.synchronize()
    for k in range(3):
        assert _t_same(got[k], want[k]), k
    for b in range(geo.B):
        one = R.project(inv[b:b + 1], seg[b:b + 1], geo.cam, geo.cfg)[3][0]
        assert _t_same(got[3][b], one), b
        assert np.array_equal(PG.np_bits(per.last_occ_frame_bits)[b], cref.pack_occ(one))
        assert not torch.equal(one, want[3][0])                       # the frames differ: no row is the union
    assert np.array_equal(PG.np_bits(per.last_occ_bits), cref.pack_occ(want[3][0]))


@pytest.mark.parametrize("per_frame", [False, True])
def test_python_mirror_refuses_unexpandable_grid(gpu_device, synth_sd, per_frame):
    """G5's grid has 5040 cells, no multiple of 32: the dense expansion refuses it, and the Python entry raises instead of returning a tensor."""
    geo, inv, seg = PG.case_inputs("G5")
    net = _net(gpu_device, geo, synth_sd, per_frame)
    with pytest.raises(RuntimeError, match="occupancy cell count must be a multiple of 32"):
        net.get_semantic_occupancy(inv.to(gpu_device), seg.to(gpu_device))
    torch.cuda.synchronize()
