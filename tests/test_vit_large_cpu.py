"""CPU: dpt_large_384 (backbone vitl16_384 = timm vit_large_patch16_384, the default model_type of load_model / load_transforms) in the architecture
tables, the transforms, the module tree and the synthetic weights, and the CPU statement of its encoder against the reference's own act_postprocess modules
(tests/golden/vit_large_reassemble.npz).  Before these were added, constructing the model raised "Backbone 'vitl16_384' not implemented on the MI355X path".
The library does not build this backbone yet: asking for its handle is refused by name (no other model runs in its place)."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import vit_large_refs as V

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_shapes_are_timms():
    from soccdpt_amd.model.spec import MODEL_TYPE_TO_BACKBONE, VIT_ARCHS, backbone_image_size, v3_state_shapes
    assert MODEL_TYPE_TO_BACKBONE[V.MODEL_TYPE] == V.BACKBONE
    a = VIT_ARCHS[V.BACKBONE]
    assert (a.img, a.patch, a.embed, a.depth, a.heads, a.hooks, a.features, a.grid) == (384, 16, V.E, V.DEPTH, V.HEADS, V.HOOKS, V.FEATURES, V.GRID)
    assert a.timm_name == "vit_large_patch16_384" and backbone_image_size(V.BACKBONE) == 384
    shapes = v3_state_shapes(V.BACKBONE)
    enc = sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("depth_net.pretrained.model."))
    assert enc == V.ENCODER_PARAMS
    m = "depth_net.pretrained.model."
    assert shapes[m + "cls_token"] == (1, 1, 1024) and shapes[m + "pos_embed"] == (1, 577, 1024) and shapes[m + "patch_embed.proj.weight"] == (1024, 3, 16, 16)
    assert shapes[m + "blocks.23.mlp.fc1.weight"] == (4096, 1024) and m + "blocks.24.norm1.weight" not in shapes
    assert [shapes[f"depth_net.scratch.layer{i}_rn.weight"][1] for i in (1, 2, 3, 4)] == [256, 512, 1024, 1024]
    # timm registers a module's own parameters before its children's: cls_token, pos_embed, then patch_embed, blocks, norm, head
    enc_keys = [k[len(m):] for k in shapes if k.startswith(m)]
    assert enc_keys[:4] == ["cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias"]
    assert enc_keys[4] == "blocks.0.norm1.weight" and enc_keys[-4:] == ["norm.weight", "norm.bias", "head.weight", "head.bias"]


def test_reassemble_keys_follow_the_reference():
    """Names and shapes of act_postprocess1..4 in the reference's registration order (recorded from its own _make_vit_b16_backbone)."""
    from soccdpt_amd.model.backbones.vit import _make_pretrained_vitl16_384
    from soccdpt_amd.model.spec import v3_state_shapes
    want = [(k, tuple(s)) for k, s in json.load(open(os.path.join(REPO, "tests", "golden", V.GOLDEN_ORDER)))]
    assert len(want) == 22
    shapes = v3_state_shapes(V.BACKBONE)
    got = [(k[len(V.PRE):], s) for k, s in shapes.items() if k.startswith(V.PRE + "act_postprocess")]
    assert got == want
    pre = _make_pretrained_vitl16_384(False, use_readout="project")
    assert [(k, tuple(p.shape)) for k, p in pre.named_parameters() if k.startswith("act_postprocess")] == want
    assert [k for k, _ in pre.named_children()] == ["model", "act_postprocess1", "act_postprocess2", "act_postprocess3", "act_postprocess4"]
    assert pre.hooks == list(V.HOOKS)


def test_transforms_are_384_and_keep_the_aspect_ratio_unless_square():
    from soccdpt_amd.model.loader import load_transforms
    t, w, h = load_transforms(V.MODEL_TYPE)
    assert (w, h) == (384, 384) and t.keep_aspect_ratio            # model/loader.py:235-240 of the reference
    t, w, h = load_transforms(V.MODEL_TYPE, square=True)
    assert (w, h) == (384, 384) and not t.keep_aspect_ratio
    t, w, h = load_transforms()                                     # the default model_type is this model
    assert (w, h) == (384, 384) and t.keep_aspect_ratio


def test_constructs_and_loads_on_the_cpu():
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(model_type=V.MODEL_TYPE, load_depth=False, sigmoid=True, camera_intrinsics_yaml=calib)
    assert m.depth_net.backbone == V.BACKBONE and m._engine_backbone() == V.BACKBONE
    sd = synth_state_dict(V.BACKBONE, alias_pretrained=True)
    r = m.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys[:3], r.missing_keys[:3])
    assert sum(p.numel() for p in m.depth_net.pretrained.model.parameters()) == V.ENCODER_PARAMS
    assert "pretrained.model.blocks.23.attn.qkv.weight" in sd and "depth_net.pretrained.act_postprocess1.4.weight" in sd      # the alias, the new keys


def test_the_library_path_refuses_the_backbone_by_name():
    """No handle exists for this backbone yet, and nothing else is run in its place: the config is refused with the backbone's name."""
    from soccdpt_amd.lib import BACKBONE_IDS, make_config
    assert V.BACKBONE not in BACKBONE_IDS
    with pytest.raises(AssertionError, match="Backbone 'vitl16_384' not implemented on the MI355X path"):
        make_config(V.BACKBONE, 3, 256, True, True, 1920, 1080, 1250.6, 1254.8, 978.4, 562.1, (256, 256, 32), (128.0, 128.0, 48.0), (10000.0, 50000.0, 800.0),
                    (55.0, -20.0, 15.0), (7.0, 0, 0))


def test_training_is_refused_by_name_before_any_data_is_read():
    from soccdpt_amd.model.spec import FORWARD_ONLY_BACKBONES, TRAIN_REFUSAL, TRAIN_REFUSAL_VIT_LARGE, train_refusal
    from soccdpt_amd.scripts.train_SOccDPT import train_net
    with pytest.raises(RuntimeError, match=r"no training step is built for dpt_large_384 \(ViT-L/16\)"):
        train_net(SOccDPT_version=3, device="cpu", model_type=V.MODEL_TYPE, base_path="/nonexistent")
    assert V.BACKBONE in FORWARD_ONLY_BACKBONES and train_refusal(V.BACKBONE) == TRAIN_REFUSAL_VIT_LARGE and train_refusal("swin2l24_384") == TRAIN_REFUSAL
    # the sentence of the models that have a forward path stays, letter for letter, where the library says it too
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "train_step.cpp")).read()
    assert TRAIN_REFUSAL in src


def test_synthetic_weights_give_a_scene():
    """The CPU statement of the whole network on the synthetic weights and frame the GPU tests of the other models use: four maps of the reference's shapes, and
    an inverse depth inside the range the projection stage places in the grid (synth_state_dict scales this model's patch filter to pixel values for that)."""
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict
    sd = synth_state_dict(V.BACKBONE)
    x = synth_input(1, size=384, seed0=8)
    with torch.no_grad():
        layers = V.encoder(sd, x)
        assert [tuple(l.shape) for l in layers] == [(1, 256, 96, 96), (1, 512, 48, 48), (1, 1024, 24, 24), (1, 1024, 12, 12)]
        assert all(0.3 < float(l.std()) < 8.0 for l in layers), [float(l.std()) for l in layers]
        inv, p1 = V.R.dpt_decoder(sd, layers)
    assert tuple(inv.shape) == (1, 384, 384) and bool(torch.isfinite(inv).all())
    assert 0.02 <= float(inv.min()) and float(inv.max()) <= 0.3, (float(inv.min()), float(inv.max()))


def test_cpu_statement_reproduces_the_reference_reassemble():
    """reassemble() -- F.conv_transpose2d on the stored [ci][co][ky][kx] weight and the rest -- on the seeded tokens against the sample recorded from the
    reference's own modules: within twice reassemble_bound (either f32 evaluation's distance from the float64 value)."""
    from soccdpt_amd.utils.synth import synth_state_dict
    sd = synth_state_dict(V.BACKBONE)
    gold = np.load(os.path.join(REPO, "tests", "golden", V.GOLDEN_REASSEMBLE))
    for n in (1, 2, 3, 4):
        t = V.golden_tokens(n)
        y = V.reassemble(sd, n, t)
        side = 96 >> (n - 1)
        assert tuple(y.shape) == tuple(gold[f"level{n}_shape"]) == (1, V.FEATURES[n - 1], side, side)
        idx = torch.from_numpy(gold[f"level{n}_idx"].astype(np.int64))
        assert torch.equal(idx, V.golden_index(n, y.numel()))
        want = torch.from_numpy(gold[f"level{n}"]).double()
        ref, bound = V.reassemble_bound(sd, n, t)
        got, ref, bound = y.reshape(-1)[idx].double(), ref.reshape(-1)[idx], bound.reshape(-1)[idx]
        err, gerr = (got - want).abs(), (want - ref).abs()
        print(f"level {n}: max |statement - reference| {float(err.max()):.2e}, max |reference - float64| {float(gerr.max()):.2e}, smallest allowance {float(bound.min()):.2e}")
        assert bool((gerr <= bound).all()) and bool((err <= 2 * bound).all()), n
        assert float(want.abs().max()) > 0.5 and float(bound.max()) < 1e-2 * float(want.abs().max())      # the bound can tell a wrong tap: see below
    # a transposed-convolution weight read as [co][ci] or with (ky, kx) swapped is far outside the bound
    t = V.golden_tokens(1)
    k = V.PRE + "act_postprocess1.4.weight"
    idx = torch.from_numpy(gold["level1_idx"].astype(np.int64))
    want = torch.from_numpy(gold["level1"]).double()
    _, bound = V.reassemble_bound(sd, 1, t)
    for wrong in (sd[k].transpose(0, 1), sd[k].transpose(2, 3)):
        y = V.reassemble({**sd, k: wrong.contiguous()}, 1, t).reshape(-1)[idx].double()
        assert float(((y - want).abs() / bound.reshape(-1)[idx]).max()) > 100
