"""GPU: the fused multi-tensor Adam step (csrc/adam.hip through soccdpt_adam_step).

Two layers.  (1) test_adam_matches_torch / test_forward_after_adam_step_uses_updated_weights: the optimiser against torch.optim.Adam on the CPU with the
reference's hyper-parameters (scripts/train_SOccDPT.py:311-318) after 5 compounded steps, parameters to 2e-6 relative, and the version-counter contract.
(2) One launch at a time through the C entry point against the float64 reference and the term-by-term bounds of tests/adam_refs.py (derivation there; the
CPU companion tests/test_adam_refs.py shows that they admit float32 evaluations and refuse named defects, among them the scalar cast from 0.999f that the
compounded comparison cannot see).  The scalars are derived in the test from (lr, betas, eps, wd, step); step k + 1 starts from what the launch of step k
wrote.  Tables: tensor sizes 1, 255, 256, 257, 131072, 131073 (the 512-block cap and one past it) and 589824; sizes mixed inside one launch with an empty
tensor among them; 0, 1, 48, 49, 96, 97 tensors; steps 1, 2, 1000, 1001, 100000, 100001; 4 (betas, eps) x lr 1e-3 and 1 x wd 0 and 1e-2; gradients over
1e-18 .. 1e18; g = 0 on zero state, g^2 underflowing and overflowing; parameters with differing step counts and empty parameters through Adam.step().

Per call: every operand sits in front of a 4 KB 0xFF guard; afterwards every guard and the gradients are untouched and a second call from the same inputs
gives the same bits; a refused call launches nothing and writes nothing.  A HIP error ends the session.

Found by reading and fixed with these tests: a parameter with numel() == 0 and a gradient made Adam.step() fail (its data_ptr() is 0 and launch_adam refused
"null tensor pointer" for the whole group); it is now stepped over like torch does.

Measured on MI355X, the worst element's error / bound over p, m, v per family (every test prints its figures with -s).  p's bound is dominated by
the final rounding 2^-24 |p'|, which a correctly rounded result uses up to fully.

    family (launches)                 p        m        v
    sizes                         0.991    0.865    0.964
    mixed sizes in one launch     0.996    0.920    0.980
    tensor counts                 0.993    0.977    0.964
    hyper-parameters and steps    0.989    0.894    0.851
    Adam.step()                   0.989    0.561    0.738
"""
import ctypes

import pytest
import torch

from tests import adam_refs as R
from tests.test_train_aux_gpu import Buf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_matches_torch(gpu_device, wd):
    from soccdpt_amd.utils.optim import Adam
    g = torch.Generator().manual_seed(3)
    shapes = [(256, 256, 3, 3), (768,), (3, 256, 1, 1), (1,), (96, 3, 4, 4)] + [(17, 5)] * 60     # > 48 tensors: two fused launches
    ref_p = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    gpu_p = [torch.nn.Parameter(p.detach().clone().to(gpu_device)) for p in ref_p]
    ro = torch.optim.Adam(ref_p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=False, foreach=False)
    go = Adam(gpu_p, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    for step in range(5):
        for i, (a, b) in enumerate(zip(ref_p, gpu_p)):
            if i == 3 and step < 2:          # a parameter without a gradient is skipped and keeps its own step count
                a.grad, b.grad = None, None
                continue
            gr = torch.randn(a.shape, generator=g) * (10.0 ** (i % 5 - 3))
            a.grad, b.grad = gr, gr.to(gpu_device)
        ro.step()
        go.step()
    torch.cuda.synchronize()
    for a, b in zip(ref_p, gpu_p):
        torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=2e-6, atol=1e-7)
    st = go.state[gpu_p[0]]
    torch.testing.assert_close(st["exp_avg"].cpu(), ro.state[ref_p[0]]["exp_avg"], rtol=2e-6, atol=1e-9)
    torch.testing.assert_close(st["exp_avg_sq"].cpu(), ro.state[ref_p[0]]["exp_avg_sq"], rtol=2e-6, atol=1e-12)
    assert go.state[gpu_p[3]]["step"] == 3
    go.zero_grad()
    assert all(p.grad is None for p in gpu_p)


def test_forward_after_adam_step_uses_updated_weights(gpu_device):
    """the fused Adam writes parameters through raw pointers.  The step must bump the tensors' version counters so that
    SOccDPT_V3 re-runs soccdpt_prepare (16-bit weight copies, BN fold, CPB tables): the forward after a step must equal the forward
    of a freshly built model holding the stepped weights, bit for bit.  Same for `p.data = ...` (new storage, no version bump) and a
    non-contiguous gradient (Adam must keep its contiguous copy alive across the launch)."""
    import os
    import tempfile
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.optim import Adam
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))

    def mk(sd):
        m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=False)
        m.load_state_dict(sd, strict=False)
        return m.eval().to(gpu_device)
    sd = synth_state_dict(alias_pretrained=True)
    m = mk(sd)
    x = synth_input(2, seed0=77).to(gpu_device)
    inv0, seg0 = m.network(x)
    g = torch.Generator().manual_seed(5)
    params = [p for p in m.parameters()]
    opt = Adam(params, lr=1e-2)
    for i, p in enumerate(params):
        gr = torch.randn(p.shape, generator=g).to(gpu_device)
        if p.dim() == 2 and i % 2 == 0:
            gr = torch.randn(tuple(reversed(p.shape)), generator=g).to(gpu_device).t()   # non-contiguous view
            assert not gr.is_contiguous()
        p.grad = gr
    opt.step()
    inv1, seg1 = m.network(x)
    torch.cuda.synchronize()
    assert not torch.equal(inv1, inv0)
    fresh = mk({k: v.detach().cpu() for k, v in m.state_dict().items()})
    inv2, seg2 = fresh.network(x)
    torch.cuda.synchronize()
    assert torch.equal(inv1, inv2) and torch.equal(seg1, seg2)
    # p.data = ... : new storage, same version
    w = m.depth_net.scratch.output_conv[4].weight
    w.data = (w.data * 1.5).clone()
    inv3, _ = m.network(x)
    fresh = mk({k: v.detach().cpu() for k, v in m.state_dict().items()})
    inv4, _ = fresh.network(x)
    torch.cuda.synchronize()
    assert not torch.equal(inv3, inv1) and torch.equal(inv3, inv4)


# ---------------- one launch at a time against float64 (tests/adam_refs.py) ----------------
MEASURED = {}


@pytest.fixture(scope="module")
def dev(gpu_device):
    from soccdpt_amd.lib import load_library
    load_library()
    return gpu_device


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def launch(tensors, h, step, dev, expect_launches=None):
    """One soccdpt_adam_step over guarded buffers -> list of {"p", "m", "v"} on the host.  An empty tensor is passed as null pointers, as torch gives them."""
    from soccdpt_amd.lib import _call, load_library
    L = load_library()
    bufs = [{k: Buf(t[k].shape, torch.float32, dev, t[k]) for k in "pgmv"} if t["p"].numel() else None for t in tensors]
    n = len(tensors)
    arr = lambda k: (ctypes.c_void_p * n)(*[None if b is None else b[k].ptr() for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[t["p"].numel() for t in tensors])
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    _call("soccdpt_adam_step", n, arr("p"), arr("g"), arr("m"), arr("v"), sizes, h.lr, h.b1, h.b2, h.eps, h.wd, step, device=dev)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:          # a HIP error: nothing more is started on this GPU
        pytest.exit(f"HIP error after soccdpt_adam_step ({n} tensors, step {step}): {e}", returncode=3)
    if expect_launches is not None:
        assert int(L.soccdpt_launch_counter()) - before == expect_launches
    out = []
    for i, (b, t) in enumerate(zip(bufs, tensors)):
        if b is None:
            out.append({k: torch.zeros(0) for k in "pmv"})
            continue
        for k in "pgmv":
            assert b[k].guard_untouched(), f"tensor {i}: the guard behind {k} was written"
        assert torch.equal(_bits(b["g"].t.cpu()), _bits(t["g"])), f"tensor {i}: the gradient was written"
        out.append({k: b[k].t.cpu() for k in "pmv"})
    return out


def launch_twice(tensors, h, step, dev, **kw):
    got = launch(tensors, h, step, dev, **kw)
    again = launch(tensors, h, step, dev, **kw)
    for i, (a, b) in enumerate(zip(got, again)):
        for k in "pmv":
            assert torch.equal(_bits(a[k]), _bits(b[k])), f"tensor {i}: {k} differs between two calls"
    return got


def held(label, tensors, got, h, step):
    """Every element of every tensor inside its bound; the worst figures recorded."""
    inp, out = R.cat_all(tensors), R.cat_all(got, "pmv")
    s = R.scalars(h, step)
    for k, (ratio, i, err, bound) in R.worst(out, inp, s).items():
        print(f"  {label} step {step} {k}: worst element {i} error {err:.2e} bound {bound:.2e} ({ratio:.3f})")
        key = (label, k)
        if key not in MEASURED or ratio > MEASURED[key][0]:
            MEASURED[key] = (ratio, err, bound)
    R.check_step(out, inp, s, f"{label} step {step}")


def two_steps(label, tensors, h, step, dev, **kw):
    """The launch at `step`, and the one at step + 1 from what it wrote and fresh gradients."""
    got = launch_twice(tensors, h, step, dev, **kw)
    held(label, tensors, got, h, step)
    nxt = [dict(o, g=R.build(t["p"].numel(), 900 + i, step + 1)["g"]) for i, (o, t) in enumerate(zip(got, tensors))]
    got2 = launch(nxt, h, step + 1, dev, **kw)
    held(label, nxt, got2, h, step + 1)


@pytest.mark.parametrize("n", R.SIZES)
def test_adam_sizes(dev, n):
    two_steps("sizes", [R.build(n, 5, 1)], R.DEFAULT, 1, dev, expect_launches=1)


def test_adam_mixed_sizes_in_one_launch(dev):
    tensors = [R.build(n, 20 + i, 2) for i, n in enumerate(R.MIXED_CHUNK)]
    assert 0 in R.MIXED_CHUNK and max(R.MIXED_CHUNK) > 2 * R.GRID_CAP * R.BLOCK
    two_steps("mixed", tensors, R.DEFAULT, 1000, dev, expect_launches=1)


@pytest.mark.parametrize("n", R.COUNTS)
def test_adam_tensor_counts(dev, n):
    two_steps("counts", R.count_case(n), R.DEFAULT, 2, dev, expect_launches=(n + R.CHUNK - 1) // R.CHUNK)


@pytest.mark.parametrize("h", R.HYPERS, ids=lambda h: f"lr{h.lr}-b{h.b1}-{h.b2}-eps{h.eps}-wd{h.wd}")
def test_adam_hyper_parameters_and_steps(dev, h):
    for step in R.STEPS:
        two_steps(f"hyper b1 {h.b1} b2 {h.b2} eps {h.eps}", [R.build(R.HYPER_N, 1, step)], h, step, dev, expect_launches=1)


@pytest.mark.parametrize("kind", R.SPECIAL)
def test_adam_special_values(dev, kind):
    inp = R.special(kind)
    got = launch_twice([inp], R.SPECIAL_HYPER, 1, dev)[0]
    R.check_special(kind, got, inp, R.scalars(R.SPECIAL_HYPER, 1))


def test_adam_refusals_write_nothing(dev):
    from soccdpt_amd.lib import load_library
    L = load_library()
    arena = Buf((8, 1024), torch.float32, dev)                  # 0xFF; every pointer of the refused calls points into it
    P = lambda *rows: (ctypes.c_void_p * len(rows))(*[None if r is None else arena.ptr() + 4096 * r for r in rows])
    S = lambda *ns: (ctypes.c_size_t * len(ns))(*ns)
    torch.cuda.synchronize()
    before = int(L.soccdpt_launch_counter())
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    bad = {
        "step 0": (1, P(0), P(1), P(2), P(3), S(10), *hyper, 0),
        "negative count": (-1, P(0), P(1), P(2), P(3), S(10), *hyper, 1),
        "null table": (1, None, P(1), P(2), P(3), S(10), *hyper, 1),
        "null sizes": (1, P(0), P(1), P(2), P(3), None, *hyper, 1),
        "null gradient of a non-empty tensor": (1, P(0), P(None), P(2), P(3), S(10), *hyper, 1),
        "null parameter behind a good tensor": (2, P(0, None), P(1, 5), P(2, 6), P(3, 7), S(10, 10), *hyper, 1),
        "null state in the second table": (50, P(*([0] * 49 + [None])), P(*([1] * 50)), P(*([2] * 50)), P(*([3] * 50)), S(*([10] * 50)), *hyper, 1),
    }
    for label, args in bad.items():
        assert L.soccdpt_adam_step(*args, None) == 1, f"accepted: {label}"
        assert b"adam" in L.soccdpt_last_error(None)
        torch.cuda.synchronize()
        assert int(L.soccdpt_launch_counter()) == before, f"{label}: a refused call launched a kernel"
        assert bool((arena.raw == 0xFF).all()), f"{label}: a refused call wrote"
    # null pointers whose size is 0 are no refusal: stepped over, nothing launched
    assert L.soccdpt_adam_step(2, P(None, None), P(None, None), P(None, None), P(None, None), S(0, 0), *hyper, 1, None) == 0
    assert L.soccdpt_adam_step(0, None, None, None, None, None, *hyper, 1, None) == 0
    assert int(L.soccdpt_launch_counter()) == before


def test_adam_step_with_empty_and_late_parameters(dev):
    """Through Adam.step(): an empty parameter with a gradient is stepped over (its count advances, nothing is launched for it; torch accepts it too), a
    group of only such parameters launches nothing, and parameters whose step counts differ go into separate launches, each inside its bound."""
    from soccdpt_amd.lib import load_library
    from soccdpt_amd.utils.optim import Adam
    L = load_library()
    h = R.DEFAULT
    shapes = [(300,), (0,), (17, 5), (0, 7), (257,)]
    host = [R.build(max(1, torch.Size(s).numel()), 60 + i, 1)["p"][: torch.Size(s).numel()].reshape(s) for i, s in enumerate(shapes)]
    ref_p = [torch.nn.Parameter(t.clone()) for t in host]
    gpu_p = [torch.nn.Parameter(t.clone().to(dev)) for t in host]
    assert gpu_p[1].data_ptr() == 0
    ro = torch.optim.Adam(ref_p, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd, foreach=False)
    go = Adam(gpu_p, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd)
    only_empty = Adam([gpu_p[1], gpu_p[3]])
    for p in (gpu_p[1], gpu_p[3]):
        p.grad = torch.zeros_like(p)
    before = int(L.soccdpt_launch_counter())
    only_empty.step()
    assert int(L.soccdpt_launch_counter()) == before and only_empty.state[gpu_p[1]]["step"] == 1
    for step in (1, 2, 3):
        launches = {}
        for i, (a, b) in enumerate(zip(ref_p, gpu_p)):
            if i == 4 and step == 1:           # joins one step late: from step 2 on its count is one behind -> a launch of its own
                a.grad = b.grad = None
                continue
            gr = R.build(max(1, a.numel()), 70 + 10 * step + i, 2, gexp=(-6.0, 3.0))["g"][: a.numel()].reshape(a.shape)
            a.grad, b.grad = gr.clone(), gr.to(dev)
            if a.numel():
                st = go.state.get(b, {"step": 0})["step"] + 1
                launches.setdefault(st, []).append((i, b.detach().cpu().clone(), gr,
                                                    *(go.state[b][k].cpu().clone() if b in go.state else torch.zeros_like(gr) for k in ("exp_avg", "exp_avg_sq"))))
        before = int(L.soccdpt_launch_counter())
        ro.step()
        go.step()
        torch.cuda.synchronize()
        assert int(L.soccdpt_launch_counter()) - before == len(launches) == (1 if step == 1 else 2)
        for st, items in launches.items():
            tensors = [{"p": p.reshape(-1), "g": g.reshape(-1), "m": m.reshape(-1), "v": v.reshape(-1)} for _, p, g, m, v in items]
            got = [{"p": gpu_p[i].detach().cpu().reshape(-1), "m": go.state[gpu_p[i]]["exp_avg"].cpu().reshape(-1),
                    "v": go.state[gpu_p[i]]["exp_avg_sq"].cpu().reshape(-1)} for i, *_ in items]
            held("Adam.step", tensors, got, h, st)
    for a, b in zip(ref_p, gpu_p):
        assert go.state[b]["step"] == int(ro.state[a]["step"])
        torch.testing.assert_close(b.detach().cpu(), a.detach(), rtol=2e-6, atol=1e-7)
    assert go.state[gpu_p[1]]["step"] == 3 and go.state[gpu_p[4]]["step"] == 2


def test_adam_measured_table():
    print()
    fam = {}
    for (label, k), rec in MEASURED.items():
        key = (label.split(" b1 ")[0] if label.startswith("hyper") else label, k)
        if key not in fam or rec[0] > fam[key][0]:
            fam[key] = rec
    for (label, k), rec in sorted(MEASURED.items()):
        print(f"TABLE {label:<44} {k}  {rec[1]:.1e}  {rec[2]:.1e}  {rec[0]:.3f}")
    for (label, k), rec in sorted(fam.items()):
        print(f"FAMILY {label:<20} {k}  error {rec[1]:.1e}  bound {rec[2]:.1e}  ratio {rec[0]:.3f}")
