"""CPU: the mask-pinned oracle (oracle/soccdpt_ref.py `pinned_masks`) and the comparison of tests/pinned_backward.py that
tests/test_train_backward_pinned_gpu.py holds the HIP training backward to.

* Pinning with the oracle's own masks changes nothing (outputs and gradients bit-identical to the unpinned oracle).
* Pinning is strict: one flipped mask entry changes the gradient; a missing or an unconsumed mask raises.
* The bounds reject kernel-shaped faults that today's whole-network bound (per tensor max(3 x torch f32, 6e-3)) lets through.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import soccdpt_ref as R
from tests import pinned_backward as PB

FDIMS = (96, 192, 384, 768)


@pytest.fixture(scope="module")
def dec_sd():
    from soccdpt_amd.utils.synth import synth_state_dict
    sd = synth_state_dict()
    return {k: v for k, v in sd.items() if k.startswith(PB.SCR) or k.startswith("seg_head.")}


def _inputs(r0=16, B=1):
    g = torch.Generator().manual_seed(7)
    feats = [torch.randn(B, c, r0 >> l, r0 >> l, generator=g) for l, c in enumerate(FDIMS)]
    a = torch.randn(B, 4 * r0, 4 * r0, generator=g)
    b = torch.randn(B, 3, 4 * r0, 4 * r0, generator=g)
    return feats, a, b


def _decoder_grads(sd, feats, a, b, dtype, ctx=None):
    """Autograd over decoder + heads (train mode) on the given feature maps: (param grads, activation grads as in pinned_backward, inv, seg)."""
    sd_o = {k: (v.clone().to(dtype).requires_grad_("running_" not in k) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    layers = [f.clone().to(dtype).requires_grad_(True) for f in feats]
    import contextlib
    with (ctx if ctx is not None else contextlib.nullcontext()):
        inv, p1 = R.dpt_decoder(sd_o, layers)
        p1.retain_grad()
        seg = R.seg_head(sd_o, p1, False, training=True)
        ((inv * a.to(dtype)).sum() + (seg * b.to(dtype)).sum()).backward()
    grads = {k: v.grad for k, v in sd_o.items() if v.is_floating_point() and v.grad is not None}
    acts = {"d_path1": PB.nhwc(p1.grad), **{f"d_feat{l}": PB.nhwc(t.grad) for l, t in enumerate(layers)}}
    return grads, acts, inv.detach(), seg.detach()


def _record(sd, feats, a, b):
    with R.record_masks() as rec:
        _decoder_grads(sd, feats, a, b, torch.float64)
    return rec.masks


def test_pinning_with_own_masks_is_identity_decoder(dec_sd):
    feats, a, b = _inputs()
    masks = _record(dec_sd, feats, a, b)
    assert len(masks) == 4 * 2 + 3 * 2 + 2 + 1      # RCU relu1 / relu2 (refinenet4 has no resConfUnit1), depth head x 2, seg head
    g0, a0, inv0, seg0 = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    with R.pinned_masks(masks) as pins:
        g1, a1, inv1, seg1 = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    assert sum(pins.flips.values()) == 0
    assert torch.equal(inv0, inv1) and torch.equal(seg0, seg1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in a0:
        assert torch.equal(a0[k], a1[k]), k


def test_pinning_with_own_masks_is_identity_hybrid_stem():
    """ResNetV2 stem (std-conv, GroupNorm + ReLU, MaxPool2dSame) and one bottleneck per stage on a 64 x 64 input."""
    from soccdpt_amd.utils.synth import synth_state_dict
    sd = {k: v.double() for k, v in synth_state_dict("vitb_rn50_384").items() if k.startswith(PB.RN)}
    arch = R.HybridArch(layers=(2, 1, 1))
    x = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ws = [torch.randn(s, generator=torch.Generator().manual_seed(4), dtype=torch.float64) for s in ((1, 256, 16, 16), (1, 512, 8, 8), (1, 1024, 4, 4))]

    def run(ctx):
        so = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        with ctx:
            outs = R.resnetv2_backbone(so, PB.RN, x, arch)
            sum((o * w).sum() for o, w in zip(outs, ws)).backward()
        return [o.detach() for o in outs], {k: v.grad for k, v in so.items() if v.grad is not None}

    import contextlib
    o0, g0 = run(contextlib.nullcontext())
    with R.record_masks() as rec:
        run(contextlib.nullcontext())
    assert PB.RN + "stem.pool" in rec.masks and PB.RN + "stem.norm" in rec.masks and PB.RN + "stages.0.blocks.1.act3" in rec.masks
    with R.pinned_masks(rec.masks) as pins:
        o1, g1 = run(contextlib.nullcontext())
    assert sum(pins.flips.values()) == 0
    got, wmax = pins.pooled[PB.RN + "stem.pool"]
    assert torch.equal(got, wmax)
    assert all(torch.equal(p, q) for p, q in zip(o0, o1))
    assert g0.keys() == g1.keys()
    for k in g0:
        if ".stem." in k:     # the gather's backward adds the overlapping windows' contributions in another order than max_pool2d's: last bit
            assert PB.rel(g1[k], g0[k]) < 1e-14, k
        else:
            assert torch.equal(g0[k], g1[k]), k
    # a pinned max-pool index that is not the window maximum is reported (pooled != window max) and moves the gradient
    idx = rec.masks[PB.RN + "stem.pool"].clone()
    idx[0, 0, 3, 3] = (int(idx[0, 0, 3, 3]) + 1) % 9
    with R.pinned_masks({**rec.masks, PB.RN + "stem.pool": idx}) as pins:
        _, g2 = run(contextlib.nullcontext())
    got, wmax = pins.pooled[PB.RN + "stem.pool"]
    assert pins.flips[PB.RN + "stem.pool"] == 1 and float((wmax - got).max()) > 0
    assert not torch.equal(g2[PB.RN + "stem.conv.weight"], g0[PB.RN + "stem.conv.weight"])


def test_pinning_is_strict(dec_sd):
    feats, a, b = _inputs()
    masks = _record(dec_sd, feats, a, b)
    g0, _, _, _ = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    # one flipped entry at one site changes the gradient, and is counted
    site = PB.SCR + "refinenet1.resConfUnit2.relu2"
    m = masks[site].clone()
    m[0, 5, 7, 9] = ~m[0, 5, 7, 9]
    with R.pinned_masks({**masks, site: m}) as pins:
        g1, _, _, _ = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    assert pins.flips[site] == 1
    k = PB.SCR + "refinenet1.resConfUnit2.conv2.weight"
    assert not torch.equal(g0[k], g1[k])
    # a site without a mask raises
    missing = {s: v for s, v in masks.items() if s != site}
    with pytest.raises(KeyError, match="no mask"):
        with R.pinned_masks(missing):
            _decoder_grads(dec_sd, feats, a, b, torch.float64)
    # a mask no site consumes raises
    with pytest.raises(KeyError, match="never consumed"):
        with R.pinned_masks({**masks, PB.SCR + "refinenet9.resConfUnit1.relu1": masks[site]}):
            _decoder_grads(dec_sd, feats, a, b, torch.float64)
    # outside the context the oracle is unpinned again
    g2, _, _, _ = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    assert torch.equal(g0[k], g2[k])


# ----------------------------------------------------------------------------------------------------------------------------------------------
# fault injection: the f32 pinned gradients stand in for HIP's, the f64 ones are the truth
# ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec_grads(dec_sd):
    feats, a, b = _inputs()
    masks = _record(dec_sd, feats, a, b)
    with R.pinned_masks(masks):
        g64, a64, _, _ = _decoder_grads(dec_sd, feats, a, b, torch.float64)
    with R.pinned_masks(masks):
        g32, a32, _, _ = _decoder_grads(dec_sd, feats, a, b, torch.float32)
    return {**g64, **a64}, {**g32, **a32}


def _old_whole_network_ok(got, ref64, ref32, k):
    """tests/test_train_step_gpu.py's per-tensor criterion for the Swin decoder and heads."""
    return PB.rel(got[k], ref64[k]) <= max(3 * PB.rel(ref32[k], ref64[k]) + 1e-5, 6e-3)


def test_unfaulted_f32_passes(dec_grads):
    ref64, ref32 = dec_grads
    got = {k: v.clone() for k, v in ref32.items()}
    assert PB.compare(got, ref64, ref32, PB.SWIN, "f32 stand-in") == []
    assert PB.compare(got, ref64, ref32, PB.HYBRID, "f32 stand-in") == []


@pytest.mark.parametrize("bounds", ["SWIN", "HYBRID"])
def test_fault_weight_gradient_slab(dec_grads, bounds):
    """A 64-channel slab of a 3x3 weight gradient 1 % off (a wrong wgrad tile): ~5e-3 relative L2 on the tensor, inside the old 6e-3."""
    ref64, ref32 = dec_grads
    k = PB.SCR + "refinenet1.resConfUnit2.conv1.weight"
    r = ref64[k]
    shares = [float(r[i:i + 64].norm() / r.norm()) for i in range(0, 256, 64)]
    i = min(range(4), key=lambda j: abs(shares[j] - 0.5)) * 64      # the slab carrying ~1/4 of the tensor's energy
    got = {kk: v.clone() for kk, v in ref32.items()}
    got[k][i:i + 64] *= 1.01
    e = PB.rel(got[k], r)
    assert 3e-3 < e < 6e-3, e
    assert _old_whole_network_ok(got, ref64, ref32, k), "the slab fault is meant to pass the old bound"
    fails = PB.compare(got, ref64, ref32, getattr(PB, bounds), "slab fault")
    assert any(f.startswith(k + ": rel") for f in fails) and any(f.startswith(k + ": block-local") for f in fails), fails


@pytest.mark.parametrize("bounds", ["SWIN", "HYBRID"])
def test_fault_activation_gradient_tile(dec_grads, bounds):
    """One 64-row tile of d_feat0 off by 1e-3: the block-local metric sees it at full size (1e-3)."""
    ref64, ref32 = dec_grads
    got = {k: v.clone() for k, v in ref32.items()}
    got["d_feat0"][64:128] *= 1.0 + 1e-3
    assert PB.block_max(got["d_feat0"], ref64["d_feat0"]) > 5e-4
    fails = PB.compare(got, ref64, ref32, getattr(PB, bounds), "tile fault")
    assert any(f.startswith("d_feat0: block-local") for f in fails), fails


def _conv_layer(dtype, g):
    """A 3x3 convolution (96 -> 256 channels, 32 x 32, bias) under a random-sign upstream gradient: (dX [pixels][C], dW, db, dY)."""
    x = torch.randn(1, 96, 32, 32, generator=g, dtype=torch.float64)
    w = torch.randn(256, 96, 3, 3, generator=g, dtype=torch.float64) * 0.05
    bias = torch.randn(256, generator=g, dtype=torch.float64)
    dy = torch.randn(1, 256, 32, 32, generator=g, dtype=torch.float64)
    xo, wo, bo = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, bias))
    F.conv2d(xo, wo, bo, padding=1).backward(dy.to(dtype))
    return {"dX": PB.nhwc(xo.grad), "dW": wo.grad, "db": bo.grad}, w, dy


def test_fault_dgrad_border_tap():
    """The dgrad of a 3x3 convolution with one tap (ky = 0, kx = 1) dropped on the top image row: the row's 32 pixels sit in one 64-row block."""
    ref64, w, dy = _conv_layer(torch.float64, torch.Generator().manual_seed(1))
    ref32, _, _ = _conv_layer(torch.float32, torch.Generator().manual_seed(1))
    wt = torch.zeros_like(w)
    wt[:, :, 0, 1] = w[:, :, 0, 1]
    tap = PB.nhwc(F.conv_transpose2d(dy, wt, padding=1))     # the tap's share of dX
    got = {k: v.clone().double() for k, v in ref32.items()}
    got["dX"][:32] -= tap[:32]                               # pixel row y = 0
    assert PB.compare({k: v.clone().double() for k, v in ref32.items()}, ref64, ref32, PB.SWIN, "conv") == []
    for bounds in (PB.SWIN, PB.HYBRID):
        fails = PB.compare(got, ref64, ref32, bounds, "border tap fault")
        assert any(f.startswith("dX: block-local") for f in fails), fails


def test_fault_bias_split_k_partial():
    """A bias gradient (column sum over 1024 pixels in 8 split-K partials of 128 rows) missing one partial."""
    ref64, _, dy = _conv_layer(torch.float64, torch.Generator().manual_seed(2))
    ref32, _, _ = _conv_layer(torch.float32, torch.Generator().manual_seed(2))
    got = {k: v.clone().double() for k, v in ref32.items()}
    got["db"] -= PB.nhwc(dy)[5 * 128:6 * 128].sum(0)
    for bounds in (PB.SWIN, PB.HYBRID):
        fails = PB.compare(got, ref64, ref32, bounds, "split-K fault")
        assert any(f.startswith("db: rel") for f in fails), fails


def test_block_metric_normalisation():
    """||d_block|| / (||ref|| sqrt(|block| / n)): a uniform relative error e gives e in every block; an all-zero reference block is fine."""
    ref = torch.randn(256, 64, dtype=torch.float64)
    assert math.isclose(PB.block_max(ref * (1 + 1e-3), ref), 1e-3, rel_tol=0.2)
    ref[:64] = 0
    got = ref.clone()
    assert PB.block_max(got, ref) == 0.0
    got[0, 0] = 1e-3
    assert PB.block_max(got, ref) > 0
