"""GPU: contracts of the C ABI that a non-Python caller relies on (include/soccdpt_hip.h, "Workspace contract"; VERDICT r1 #8 /
ADVICE r1): the library, not the caller, keeps the zero-halo invariant of the workspace; errors are returned, never silent."""
import ctypes
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(gpu_device):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True)
    m.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    return m.eval().to(gpu_device)


def _raw_network(eng, x, ws):
    B, S = x.shape[0], x.shape[2]
    inv = torch.empty((B, S, S), device=x.device)
    seg = torch.empty((B, 3, S, S), device=x.device)
    rc = eng.L.soccdpt_network(eng._h, x.data_ptr(), B, inv.data_ptr(), seg.data_ptr(), ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream(x.device).cuda_stream)
    return rc, inv, seg


def test_library_owns_the_zero_halo_invariant(model, gpu_device):
    """A caller-provided buffer full of garbage, reused across batch sizes, gives the same results as fresh zeroed buffers."""
    from soccdpt_amd.utils.synth import synth_input
    eng = model._engine(gpu_device)
    model._sync_weights(eng)
    x3 = synth_input(3, seed0=50).to(gpu_device)
    ref = {}
    for B in (2, 3):
        inv, seg = model.network(x3[:B])
        ref[B] = (inv.clone(), seg.clone())
    need = max(eng.L.soccdpt_workspace_bytes(eng._h, B) for B in (2, 3))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu_device)      # NaN patterns in every halo
    fills0 = eng.workspace_zero_fills()
    for B in (2, 3, 2, 2):
        rc, inv, seg = _raw_network(eng, x3[:B].contiguous(), ws)
        torch.cuda.synchronize()
        assert rc == 0, eng.L.soccdpt_last_error(eng._h)
        assert torch.equal(inv, ref[B][0]) and torch.equal(seg, ref[B][1]), B
    assert eng.workspace_zero_fills() - fills0 == 3          # one per layout change (2, 3, 2), none for the repeated call
    # somebody scribbles over the buffer: the caller says so, the library re-zeroes
    ws.fill_(0x7F)
    assert eng.L.soccdpt_workspace_invalidate(eng._h) == 0
    rc, inv, seg = _raw_network(eng, x3[:2].contiguous(), ws)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(inv, ref[2][0])


def test_errors_are_returned(model, gpu_device):
    from soccdpt_amd.utils.synth import synth_input
    eng = model._engine(gpu_device)
    model._sync_weights(eng)
    x = synth_input(2, seed0=51).to(gpu_device)
    need = eng.L.soccdpt_workspace_bytes(eng._h, 2)
    small = torch.empty((need // 2,), dtype=torch.uint8, device=gpu_device)
    rc, _, _ = _raw_network(eng, x, small)
    assert rc != 0 and b"workspace too small" in eng.L.soccdpt_last_error(eng._h)
    # the experimental multi-stream mode is opt-in
    old = os.environ.pop("SOCCDPT_ALLOW_MULTISTREAM", None)
    try:
        assert eng.L.soccdpt_set_streams(eng._h, 2) != 0
        assert b"experimental" in eng.L.soccdpt_last_error(eng._h)
        assert eng.L.soccdpt_set_streams(eng._h, 1) == 0
    finally:
        if old is not None:
            os.environ["SOCCDPT_ALLOW_MULTISTREAM"] = old
    # unknown backbone id / wrong ABI version are refused at creation
    cfg = type(eng.cfg)()
    ctypes.memmove(ctypes.byref(cfg), ctypes.byref(eng.cfg), ctypes.sizeof(cfg))
    cfg.backbone = 99
    h = ctypes.c_void_p()
    assert eng.L.soccdpt_create(ctypes.byref(cfg), ctypes.byref(h)) != 0
    cfg.backbone = 0
    cfg.abi_version = 12345
    assert eng.L.soccdpt_create(ctypes.byref(cfg), ctypes.byref(h)) != 0


@pytest.mark.parametrize("backbone", ["swin2t16_256", "swin2b24_384", "vitb_rn50_384"])
def test_weight_keys_are_the_consumed_state_dict(gpu_device, backbone):
    """soccdpt_num_weights / soccdpt_weight_key list the state dict of the backbone without the tensors the forward never reads, in state-dict
    order (the list tests/test_params_cpu.py holds the parameter table to).  Only creates handles: no kernel runs."""
    from oracle import soccdpt_ref as R
    from soccdpt_amd.lib import Engine, make_config
    from tests.consumed_keys import consumed_shapes
    cam, cfg = R.Camera(), R.ProjConfig()
    c = make_config(backbone, 3, 256, False, False, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                    cfg.grid_size, cfg.occupancy_shape(), cfg.pc_scale, cfg.pc_shift, cfg.correction_angle)
    eng = Engine(c, gpu_device)
    try:
        assert eng.weight_keys() == [k for k, _ in consumed_shapes(backbone)]
    finally:
        eng.close()


def test_training_entry_points_return_errors(gpu_device):
    """soccdpt_train_* contract: wrong precision, unbound weights, short workspace, a backward without its forward, a mismatching batch size
    and bad dropout probabilities are refused with a message (non-zero return), never executed; garbage in the workspace is harmless because
    the library zero-fills what it needs."""
    from soccdpt_amd.lib import PREC_F32
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    x = synth_input(1, seed0=2).to(gpu_device)
    inv = torch.empty((1, 256, 256), device=gpu_device)
    seg = torch.empty((1, 3, 256, 256), device=gpu_device)
    err = lambda e: e.L.soccdpt_last_error(e._h).decode()

    # bf16 handle: refused
    m16 = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=False)
    m16.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    m16 = m16.to(gpu_device)
    e16 = m16._engine(gpu_device)
    m16._sync_weights(e16)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=gpu_device)
    assert e16.L.soccdpt_train_forward(e16._h, x.data_ptr(), 1, inv.data_ptr(), seg.data_ptr(), ws.data_ptr(), ws.numel(), 0.0, 0, stream) != 0
    assert "SOCCDPT_PREC_F32" in err(e16)

    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=False, precision=PREC_F32)
    m.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    m = m.to(gpu_device).train()
    m.drop_path_rate = 0.0        # the raw C calls below use the handle's default (no stochastic depth); the Python mirror must do the same step
    eng = m._engine(gpu_device)
    need = eng.L.soccdpt_train_workspace_bytes(eng._h, 1)
    big = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu_device)        # garbage: 0xFF bytes are NaN as f32, bf16, fp16 and in both halves of x3
    # weights not bound yet
    assert eng.L.soccdpt_train_forward(eng._h, x.data_ptr(), 1, inv.data_ptr(), seg.data_ptr(), big.data_ptr(), big.numel(), 0.0, 0, stream) != 0
    assert "not bound" in err(eng)
    m._bind_for_training(eng)
    # short workspace, bad dropout, null pointers
    assert eng.L.soccdpt_train_forward(eng._h, x.data_ptr(), 1, inv.data_ptr(), seg.data_ptr(), big.data_ptr(), need // 2, 0.0, 0, stream) != 0
    assert "workspace too small" in err(eng)
    assert eng.L.soccdpt_train_forward(eng._h, x.data_ptr(), 1, inv.data_ptr(), seg.data_ptr(), big.data_ptr(), big.numel(), 1.0, 0, stream) != 0
    assert eng.L.soccdpt_train_forward(eng._h, None, 1, inv.data_ptr(), seg.data_ptr(), big.data_ptr(), big.numel(), 0.0, 0, stream) != 0
    # backward before any forward on this workspace
    g1 = torch.zeros_like(inv)
    g2 = torch.zeros_like(seg)
    assert eng.L.soccdpt_train_backward(eng._h, x.data_ptr(), 1, g1.data_ptr(), g2.data_ptr(), big.data_ptr(), big.numel(), stream) != 0
    assert "no soccdpt_train_forward ran" in err(eng)
    # a proper forward on the garbage-filled workspace works and matches the Python path
    assert eng.L.soccdpt_train_forward(eng._h, x.data_ptr(), 1, inv.data_ptr(), seg.data_ptr(), big.data_ptr(), big.numel(), 0.0, 0, stream) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(inv).all() and torch.isfinite(seg).all()
    # backward with another batch size than the forward's
    assert eng.L.soccdpt_train_backward(eng._h, x.data_ptr(), 2, g1.data_ptr(), g2.data_ptr(), big.data_ptr(), big.numel(), stream) != 0
    g1.normal_()
    g2.normal_()
    assert eng.L.soccdpt_train_backward(eng._h, x.data_ptr(), 1, g1.data_ptr(), g2.data_ptr(), big.data_ptr(), big.numel(), stream) == 0
    torch.cuda.synchronize()
    # every scratch region the backward reads was initialised by the library: no NaN of the garbage fill reaches a gradient
    grads = m._train_state[id(eng)]["grads"]
    assert sum(g is not None for g in grads.values()) > 250
    assert all(torch.isfinite(g).all() for g in grads.values() if g is not None)
    assert eng.L.soccdpt_bind_grad(eng._h, b"no.such.key", None) != 0 and "unknown key" in err(eng)
    inv2, seg2 = m.train_forward(x, seed=0)
    # the same step through the Python mirror (running buffers have moved on by one update: compare the depth output only)
    assert torch.equal(inv2, inv)
