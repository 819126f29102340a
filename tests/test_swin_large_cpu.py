"""CPU: dpt_swin2_large_384 (backbone swin2l24_384 = timm swinv2_large_window12to24_192to384_22kft1k) in the architecture tables, the transforms and the
module tree.  Before the model was added, constructing it raised "Backbone 'swin2l24_384' not implemented on the MI355X path"."""
import os
import tempfile

import pytest
import torch

from tests import swin_large_refs as L


def test_state_shapes_are_timms():
    from soccdpt_amd.model.spec import SWIN_ARCHS, v3_state_shapes
    a = SWIN_ARCHS[L.BACKBONE]
    assert (a.img, a.patch, a.embed, a.depths, a.heads, a.window, a.pretrained_window, a.hooks) == \
        (384, 4, 192, (2, 2, 18, 2), (6, 12, 24, 48), 24, (12, 12, 12, 6), (1, 1, 17, 1))
    assert a.timm_name == "swinv2_large_window12to24_192to384_22kft1k"
    shapes = v3_state_shapes(L.BACKBONE)
    enc = 0
    for k, s in shapes.items():
        if k.startswith("depth_net.pretrained.model."):
            n = 1
            for d in s:
                n *= d
            enc += n
    assert enc == L.ENCODER_PARAMS
    assert [shapes[f"depth_net.scratch.layer{i}_rn.weight"][1] for i in (1, 2, 3, 4)] == [192, 384, 768, 1536]
    # the oracle's row (inserted by tests/swin_large_refs.py) states the same architecture
    o = L.R.ARCHS[L.BACKBONE]
    assert (o.img, o.patch, o.embed, tuple(o.depths), tuple(o.heads), o.window, tuple(o.pretrained_window), tuple(o.hooks)) == \
        (a.img, a.patch, a.embed, a.depths, a.heads, a.window, a.pretrained_window, a.hooks)


def test_transforms_are_384_square():
    from soccdpt_amd.model.loader import load_transforms
    t, w, h = load_transforms(L.MODEL_TYPE)
    assert (w, h) == (384, 384)
    assert not t.keep_aspect_ratio      # as for the other Swin-V2 models (model/loader.py:183-204 of the reference)


def test_constructs_and_loads_on_the_cpu():
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(model_type=L.MODEL_TYPE, load_depth=False, sigmoid=True, camera_intrinsics_yaml=calib)
    assert m.depth_net.backbone == L.BACKBONE and m._engine_backbone() == L.BACKBONE
    sd = synth_state_dict(L.BACKBONE, alias_pretrained=True)
    r = m.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys[:3], r.missing_keys[:3])
    assert sum(p.numel() for p in m.depth_net.pretrained.model.parameters()) == L.ENCODER_PARAMS


def test_every_precision_mode_has_a_config():
    """make_config maps the backbone to its id in each of the five modes (the handle itself is created on the GPU: tests/test_swin_large_gpu.py)."""
    from soccdpt_amd.lib import BACKBONE_IDS, PREC_BF16, PREC_F16, PREC_F16X3, PREC_F32, PREC_MIXED, make_config
    for prec in (PREC_BF16, PREC_F32, PREC_F16, PREC_F16X3, PREC_MIXED):
        cfg = make_config(L.BACKBONE, 3, 256, True, True, 1920, 1080, 1250.6, 1254.8, 978.4, 562.1, (256, 256, 32), (128.0, 128.0, 48.0), (10000.0, 50000.0, 800.0),
                          (55.0, -20.0, 15.0), (7.0, 0, 0), precision=prec)
        assert cfg.backbone == BACKBONE_IDS[L.BACKBONE] == 3 and cfg.precision == prec


def test_training_is_refused_by_name_before_any_data_is_read():
    from soccdpt_amd.scripts.train_SOccDPT import train_net
    with pytest.raises(RuntimeError, match="dpt_swin2_tiny_256, dpt_swin2_base_384 and dpt_hybrid_384"):
        train_net(SOccDPT_version=3, device="cpu", model_type=L.MODEL_TYPE, base_path="/nonexistent/dataset")
    # the header, the library's refusal and the Python one name the same three models
    from soccdpt_amd.model.spec import TRAIN_REFUSAL
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "soccdpt_amd", "csrc", "train_step.cpp")).read()
    assert TRAIN_REFUSAL in src


def test_export_table_has_the_model():
    from soccdpt_amd.model.spec import SWIN_ARCHS
    from soccdpt_amd.scripts.export_SOccDPT import SWIN
    a, e = SWIN_ARCHS[L.BACKBONE], SWIN[L.BACKBONE]
    assert (e["img"], e["patch"], e["embed"], e["depths"], e["heads"], e["window"], e["pretrained"], e["hooks"]) == \
        (a.img, a.patch, a.embed, a.depths, a.heads, a.window, a.pretrained_window, a.hooks)
    assert torch.tensor(e["heads"]).mul(32).tolist() == [a.embed << s for s in range(4)]      # head dim 32 at every stage: the attention kernels' one head size
