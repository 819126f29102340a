"""CPU: dpt_swin_large_384 (backbone swinl12_384 = timm swin_large_patch4_window12_384, Swin-V1-L) in the architecture tables, the transforms, the module
tree and the C ABI's tables; the CPU statement of its encoder against HF transformers' independent SwinModel; the float64 references of its three kernels
against float32 emulations and seeded defects.  Before the model was added, constructing it raised "Backbone 'swinl12_384' not implemented on the MI355X
path", and net.network() took a frame of any size."""
import ctypes
import math
import os
import re
import tempfile

import pytest
import torch

from tests import swin1_large_refs as L
from tests.test_capi_symbols import _c_class, _ctypes_class

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _numel(shape):
    return math.prod(shape)


# ---------------------------------------------------------------------------------------------------------------------------------
# tables, module tree, refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_shapes_and_parameter_counts():
    from soccdpt_amd.model import spec
    a = spec.SWIN1_ARCHS[L.BACKBONE]
    assert (a.img, a.patch, a.embed, a.depths, a.heads, a.window, a.hooks) == (384, 4, 192, (2, 2, 18, 2), (6, 12, 24, 48), 12, (1, 1, 17, 1))
    assert a.timm_name == "swin_large_patch4_window12_384"
    assert L.BACKBONE not in spec.SWIN_ARCHS                     # that table is "Swin-V2, with a training plan"
    assert spec.arch_of(L.BACKBONE) is a and spec.backbone_image_size(L.BACKBONE) == 384
    assert spec.MODEL_TYPE_TO_BACKBONE[L.MODEL_TYPE] == L.BACKBONE and L.BACKBONE in spec.FORWARD_ONLY_BACKBONES
    assert [a.stage_res(s) for s in range(4)] == [96, 48, 24, 12]
    assert [a.window_shift(s, 1) for s in range(4)] == [(12, 6), (12, 6), (12, 6), (12, 0)]      # stage 3: res == window, unshifted
    shapes = spec.v3_state_shapes(L.BACKBONE)
    enc = {k[len(L.PRE):]: s for k, s in shapes.items() if k.startswith(L.PRE)}
    params = {k: s for k, s in enc.items() if k.split(".")[-1] not in spec.SWIN1_BUFFER_LEAVES}
    assert sum(_numel(s) for s in params.values()) == L.ENCODER_PARAMS
    dead = sum(_numel(s) for k, s in params.items() if k.startswith(("norm.", "head.")))
    assert L.ENCODER_PARAMS - dead == L.CONSUMED_ENCODER_PARAMS
    assert enc["layers.0.blocks.0.attn.relative_position_bias_table"] == (529, 6) and enc["layers.3.blocks.1.attn.qkv.bias"] == (3 * 1536,)
    assert enc["layers.2.downsample.norm.weight"] == (4 * 768,) and enc["layers.2.downsample.reduction.weight"] == (1536, 3072)
    assert enc["layers.0.blocks.1.attn_mask"] == (64, 144, 144) and "layers.0.blocks.0.attn_mask" not in enc and "layers.3.blocks.1.attn_mask" not in enc
    assert [shapes[f"depth_net.scratch.layer{i}_rn.weight"][1] for i in (1, 2, 3, 4)] == [192, 384, 768, 1536]
    assert (L.ARCH.img, L.ARCH.patch, L.ARCH.embed, L.ARCH.depths, L.ARCH.heads, L.ARCH.window, L.ARCH.hooks) == \
        (a.img, a.patch, a.embed, a.depths, a.heads, a.window, a.hooks)


def test_transforms_are_384_square():
    from soccdpt_amd.model.loader import load_transforms
    t, w, h = load_transforms(L.MODEL_TYPE)
    assert (w, h) == (384, 384)
    assert not t.keep_aspect_ratio and t.resize_method == "minimal"
    assert tuple(float(v) for v in t.mean) == (0.5, 0.5, 0.5) and tuple(float(v) for v in t.std) == (0.5, 0.5, 0.5)


@pytest.fixture(scope="module")
def model():
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    return SOccDPT_V3(model_type=L.MODEL_TYPE, load_depth=False, sigmoid=True, camera_intrinsics_yaml=calib)


def test_constructs_and_loads_on_the_cpu(model):
    from soccdpt_amd.model import spec
    from soccdpt_amd.utils.synth import synth_state_dict
    m = model
    assert m.depth_net.backbone == L.BACKBONE and m._engine_backbone() == L.BACKBONE
    assert list(m.depth_net.pretrained.hooks) == [1, 1, 17, 1]
    assert [n for n, _ in m.depth_net.pretrained.named_children()] == ["model", "act_postprocess1", "act_postprocess2", "act_postprocess3", "act_postprocess4"]
    sd = synth_state_dict(L.BACKBONE, alias_pretrained=True)
    r = m.load_state_dict(sd, strict=False)
    assert not r.unexpected_keys and not r.missing_keys, (r.unexpected_keys[:3], r.missing_keys[:3])
    assert sum(p.numel() for p in m.depth_net.pretrained.model.parameters()) == L.ENCODER_PARAMS
    # the module tree's own state_dict() lists the encoder in the order the table states, buffers included
    own = [k for k in m.state_dict() if k.startswith(L.PRE)]
    assert own == [k for k in spec.v3_state_shapes(L.BACKBONE) if k.startswith(L.PRE)]
    # the buffers are timm's: the index the kernels' bias arrangement uses, the mask the oracle's helper states
    blk = m.depth_net.pretrained.model.layers[0].blocks[1]
    assert torch.equal(blk.attn.relative_position_index, L.R.relative_position_index(12))
    assert torch.equal(blk.attn_mask, L.R.shift_attn_mask(96, 12, 6))


def test_every_precision_mode_has_a_config():
    from soccdpt_amd.lib import BACKBONE_IDS, PREC_BF16, PREC_F16, PREC_F16X3, PREC_F32, PREC_MIXED, make_config
    for prec in (PREC_BF16, PREC_F32, PREC_F16, PREC_F16X3, PREC_MIXED):
        cfg = make_config(L.BACKBONE, 3, 256, True, True, 1920, 1080, 1250.6, 1254.8, 978.4, 562.1, (256, 256, 32), (128.0, 128.0, 48.0), (10000.0, 50000.0, 800.0),
                          (55.0, -20.0, 15.0), (7.0, 0, 0), precision=prec)
        assert cfg.backbone == BACKBONE_IDS[L.BACKBONE] == 5 and cfg.precision == prec
    assert 4 not in BACKBONE_IDS.values()          # reserved for vitl16_384
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    assert re.search(r"#define\s+SOCCDPT_BACKBONE_SWINL12_384\s+5\b", header)


def test_training_is_refused_by_name_before_any_data_is_read(model):
    from soccdpt_amd.model.spec import TRAIN_REFUSAL, TRAIN_REFUSAL_SWIN1_LARGE, TRAIN_REFUSAL_VIT_LARGE, train_refusal
    from soccdpt_amd.scripts.train_SOccDPT import train_net
    assert train_refusal(L.BACKBONE) == TRAIN_REFUSAL_SWIN1_LARGE and "dpt_swin_large_384" in TRAIN_REFUSAL_SWIN1_LARGE
    assert TRAIN_REFUSAL_SWIN1_LARGE not in (TRAIN_REFUSAL, TRAIN_REFUSAL_VIT_LARGE)
    with pytest.raises(RuntimeError, match=re.escape(TRAIN_REFUSAL_SWIN1_LARGE)):
        train_net(SOccDPT_version=3, device="cpu", model_type=L.MODEL_TYPE, base_path="/nonexistent/dataset")
    # net.train(); net(x): refused before an engine exists (a CPU tensor gets this far and no further)
    model.train()
    try:
        with pytest.raises(RuntimeError, match=re.escape(TRAIN_REFUSAL_SWIN1_LARGE)):
            model(torch.zeros(1, 3, 384, 384))
    finally:
        model.eval()
    # the library's refusal says the same
    src = open(os.path.join(REPO, "soccdpt_amd", "csrc", "train_step.cpp")).read()
    assert TRAIN_REFUSAL_SWIN1_LARGE in src


def test_network_refuses_a_frame_of_another_size_on_the_cpu(model):
    """net.network() allocates its outputs at the INPUT's size while the library reads and writes at the handle's: the assertion forward() has, evaluated before
    the engine is created.  (A tensor of the right size gets past it and is refused for being on the CPU.)"""
    with pytest.raises(AssertionError, match=re.escape("expected x [B,3,384,384], got (1, 3, 256, 256)")):
        model.network(torch.zeros(1, 3, 256, 256))
    with pytest.raises(AssertionError, match="expected x"):
        model.network(torch.zeros(1, 1, 384, 384))
    with pytest.raises(RuntimeError, match="MI355X only"):
        model.network(torch.zeros(1, 3, 384, 384))


# ---------------------------------------------------------------------------------------------------------------------------------
# the fifth header
# ---------------------------------------------------------------------------------------------------------------------------------
def _swin1_header():
    text = open(os.path.join(REPO, "include", "soccdpt_swin1.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    out = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?[\s\*])(soccdpt_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code, flags=re.M):
        assert name not in out, f"{name} is declared twice"
        out[name] = (_c_class(ret, False), [_c_class(" ".join(p.split()), True) for p in params.split(",")])
    assert sorted(out) == sorted(set(re.findall(r"\b(soccdpt_[a-z_0-9]+)\s*\(", code)))
    return out


def test_swin1_prototype_table_matches_the_header():
    from soccdpt_amd import lib
    header = _swin1_header()
    assert list(header) == ["soccdpt_swin1_window_attention", "soccdpt_swin1_ln_rows", "soccdpt_swin1_merge_ln"]
    assert list(lib.SWIN1_PROTOTYPES) == list(header), "the table follows the header's order"
    assert not set(lib.SWIN1_PROTOTYPES) & (set(lib.PROTOTYPES) | set(lib.VIS_PROTOTYPES) | set(lib.DATA_PROTOTYPES) | set(lib.PACK_PROTOTYPES))
    for name, (restype, argtypes) in lib.SWIN1_PROTOTYPES.items():
        want_ret, want_args = header[name]
        assert _ctypes_class(restype) == want_ret, name
        assert len(argtypes) == len(want_args), f"{name}: {len(want_args)} parameters in the header, {len(argtypes)} in the table"
        for i, (a, w) in enumerate(zip(argtypes, want_args)):
            assert _ctypes_class(a) == w, f"{name}: parameter {i} is {w} in the header, {a} in the table"
        assert argtypes[-1] is ctypes.c_void_p, "the stream goes last"
    assert "swin1.hip" in lib.FORWARD_SOURCES


def test_swin1_symbols_exported_and_argument_errors_need_no_gpu():
    """The checks run before anything is launched, so they can be seen without a device: each returns non-zero and names itself in soccdpt_last_error."""
    from soccdpt_amd.lib import ABI_VERSION, LIB_PATH, PREC_F16, PREC_F32, load_library
    raw = ctypes.CDLL(LIB_PATH)
    for name in _swin1_header():
        assert hasattr(raw, name), f"{name} declared in include/soccdpt_swin1.h but not exported"
    lib = load_library()
    assert ABI_VERSION == 13 and lib.soccdpt_abi_version() == 13      # a fifth header, not a new version of the first
    p = 4096      # 16-byte aligned, never dereferenced: every call below fails its argument check

    def refused(rc, word):
        msg = lib.soccdpt_last_error(None).decode()
        assert rc != 0 and msg.startswith("soccdpt_swin1_") and word in msg, (rc, msg)
    # (qkv, table, out, scratch, B, res, ws, shift, heads, precision, out_x3, stream)
    refused(lib.soccdpt_swin1_window_attention(None, p, p, p, 1, 24, 12, 0, 2, PREC_F16, 0, None), "null")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, None, 1, 24, 12, 0, 2, PREC_F16, 0, None), "null")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 0, 24, 12, 0, 2, PREC_F16, 0, None), "positive")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 12, 0, -1, PREC_F16, 0, None), "positive")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 24, 0, 2, PREC_F16, 0, None), "window size not instantiated")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 32, 16, 0, 2, PREC_F32, 0, None), "window size not instantiated")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 12, 3, 2, PREC_F16, 0, None), "shift must be 0 or ws / 2")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 12, 12, 2, PREC_F16, 0, None), "shift outside")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 30, 12, 0, 2, PREC_F16, 0, None), "res % ws")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 12, 0, 2, 9, 0, None), "unknown precision")
    refused(lib.soccdpt_swin1_window_attention(p, p, p, p, 1, 24, 12, 0, 2, PREC_F32, 1, None), "x3 output form")
    refused(lib.soccdpt_swin1_window_attention(p + 2, p, p, p, 1, 24, 12, 0, 2, PREC_F16, 0, None), "aligned")
    # (xf, g, beta, out, format, rows, C, eps, stream)
    refused(lib.soccdpt_swin1_ln_rows(p, None, p, 2 * p, PREC_F16, 5, 192, 1e-5, None), "null")
    refused(lib.soccdpt_swin1_ln_rows(p, p, p, 2 * p, PREC_F16, 0, 192, 1e-5, None), "rows")
    refused(lib.soccdpt_swin1_ln_rows(p, p, p, 2 * p, PREC_F16, 5, 256, 1e-5, None), "C not instantiated")
    refused(lib.soccdpt_swin1_ln_rows(p, p, p, 2 * p, 7, 5, 192, 1e-5, None), "operand format")
    refused(lib.soccdpt_swin1_ln_rows(p, p, p, p, PREC_F32, 5, 192, 1e-5, None), "alias")
    refused(lib.soccdpt_swin1_ln_rows(p, p, p, 2 * p, PREC_F16, 5, 192, 0.0, None), "eps")
    # (xf, g, beta, out, format, B, R, C, eps, stream)
    refused(lib.soccdpt_swin1_merge_ln(p, p, None, 2 * p, PREC_F16, 1, 4, 192, 1e-5, None), "null")
    refused(lib.soccdpt_swin1_merge_ln(p, p, p, 2 * p, PREC_F16, 1, 5, 192, 1e-5, None), "R must be even")
    refused(lib.soccdpt_swin1_merge_ln(p, p, p, 2 * p, PREC_F16, 1, 0, 192, 1e-5, None), "positive")
    refused(lib.soccdpt_swin1_merge_ln(p, p, p, 2 * p, PREC_F16, 0, 4, 192, 1e-5, None), "positive")
    refused(lib.soccdpt_swin1_merge_ln(p, p, p, 2 * p, PREC_F16, 1, 4, 1536, 1e-5, None), "C not instantiated")


# ---------------------------------------------------------------------------------------------------------------------------------
# the statement of the encoder: non-empty scene, HF cross-check
# ---------------------------------------------------------------------------------------------------------------------------------
def test_synthetic_scene_is_not_empty():
    """The pre-norm stream reaches the decoder un-normalised (the hooked maps are block outputs); on the synthetic draw as it stands -- no tensor of this
    backbone is rescaled -- synth_input(1, 384, seed0=8) gives an inverse depth that the projection places inside the grid."""
    import numpy as np
    from oracle import cref
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict
    sd = synth_state_dict(L.BACKBONE, alias_pretrained=True)
    x = synth_input(1, size=384, seed0=8)
    with torch.no_grad():
        inv, seg, _ = L.network(sd, x, sigmoid=True)
    assert tuple(inv.shape) == (1, 384, 384) and bool(torch.isfinite(inv).all()) and bool(torch.isfinite(seg).all())
    assert 0.0 < float(inv.mean()) < 1.0
    bits = cref.project(inv, seg, want=("occ_bits",))["occ_bits"]
    occupied = int(np.unpackbits(bits.view(np.uint8)).sum())
    print(f"swin_large_384 CPU statement: inverse depth {float(inv.min()):.4f} .. {float(inv.max()):.4f}, {occupied} occupied voxel-classes")
    assert occupied > 100          # 738 when the model was added: inverse depth 0.042 .. 0.211, inside the 0.02 .. 0.3 the synthetic heads aim at


HF_CONFIG = dict(image_size=192, patch_size=4, embed_dim=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=6)     # last stage = the window


def test_encoder_statement_matches_hf_swin_in_float64():
    """transformers' SwinModel is an independent implementation of the same network (timm itself is not installed: the timm encoder stays unpinned, as for
    the other models).  Its keys are mapped to timm's names and the statement above runs on them in float64; HF reports each stage's output after its
    PatchMerging.  Every parameter N(0, 0.2), B = 2; a throw-away version of this check agreed to 2e-14 on values up to 22."""
    transformers = pytest.importorskip("transformers")
    c = HF_CONFIG
    cfg = transformers.SwinConfig(image_size=c["image_size"], patch_size=c["patch_size"], num_channels=3, embed_dim=c["embed_dim"], depths=list(c["depths"]),
                                  num_heads=list(c["num_heads"]), window_size=c["window_size"], mlp_ratio=4.0, qkv_bias=True, hidden_dropout_prob=0.0,
                                  attention_probs_dropout_prob=0.0, drop_path_rate=0.0, hidden_act="gelu", use_absolute_embeddings=False, layer_norm_eps=1e-5)
    hf = transformers.SwinModel(cfg, add_pooling_layer=False).double().eval()
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for prm in hf.parameters():
            prm.copy_(0.2 * torch.randn(prm.shape, generator=g, dtype=torch.float64))
    x = torch.randn(2, 3, c["image_size"], c["image_size"], generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = hf(pixel_values=x, output_hidden_states=True).hidden_states          # embeddings, then every stage after its downsample
    sd = L.hf_to_timm({k: v.detach() for k, v in hf.state_dict().items()}, c["depths"])
    arch = L.Arch(c["image_size"], c["patch_size"], c["embed_dim"], c["depths"], c["num_heads"], c["window_size"], (1, 1, 1, 1))
    got = []
    with torch.no_grad():
        L.encoder(sd, x, arch, after_downsample=got)
    assert len(want) == 5 and len(got) == 4
    worst = 0.0
    for s in range(4):
        assert got[s].shape == want[s + 1].shape
        worst = max(worst, float((got[s] - want[s + 1]).abs().max()))
    print(f"statement vs HF SwinModel, float64: worst |difference| {worst:.2e} on values up to {float(max(w.abs().max() for w in want)):.1f}")
    assert worst <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel references: emulations inside, defects outside
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_OUT = {"bf16": "bf16", "f16": "f16", "f32": "f32", "f16_x3": "x3", "f32_x3": "x3"}     # what the launch stores: 16-bit, f32, or x3 pairs of the f32 accumulators


@pytest.mark.parametrize("case", list(L.ATTN_CASES))
@pytest.mark.parametrize("mode", list(ATTN_OUT))
def test_attention_emulation_sits_inside_the_bound(case, mode):
    fmt = mode.split("_")[0]
    inp, ref, bound = L.attention_case(case, fmt)
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
    acc = L.emulate_attention(inp["qkv"], inp["table"], *L.ATTN_CASES[case], fmt)
    L.check_values(L.to_format(acc, ATTN_OUT[mode]), ATTN_OUT[mode], ref, bound, f"emulated attention {case} {mode}")


@pytest.mark.parametrize("defect", L.ATTN_DEFECTS)
@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
def test_attention_defects_leave_the_bound(defect, fmt):
    """Each seeded defect, evaluated exactly, lies outside the bound in every output form.  mask_dropped needs a shifted case; the others use it too."""
    case = "r24_shift"
    inp, ref, bound = L.attention_case(case, fmt)
    bad, _ = L.attention_ref(inp["qkv"], inp["table"], *L.ATTN_CASES[case], fmt, defect=defect)
    for out in ({"bf16": ("bf16",), "f16": ("f16", "x3"), "f32": ("f32", "x3")}[fmt]):
        with pytest.raises(AssertionError):
            L.check_values(L.to_format(bad.float(), out), out, ref, bound, f"{defect} {fmt}->{out}")


@pytest.mark.parametrize("C", L.LN_WIDTHS)
@pytest.mark.parametrize("out", L.OUT_FORMATS)
def test_prenorm_emulation_sits_inside_the_bound(C, out):
    inp, ref, bound = L.prenorm_case(C)
    L.check_values(L.to_format(L.emulate_ln(inp["xf"], inp["g"], inp["beta"]), out), out, ref, bound, f"emulated pre-norm LN C = {C} {out}")


@pytest.mark.parametrize("shape", L.MERGE_CASES)
@pytest.mark.parametrize("out", L.OUT_FORMATS)
def test_merge_ln_emulation_inside_and_defects_outside(shape, out):
    inp, ref, bound = L.merge_case(*shape)
    C = shape[2]
    rows = L.merge_gather(inp["xf"]).reshape(-1, 4 * C)
    L.check_values(L.to_format(L.emulate_ln(rows, inp["g"], inp["beta"]), out), out, ref, bound, f"emulated merge-LN {shape} {out}")
    for defect in ("swapped", "ln_over_c"):
        bad, _ = L.merge_ln_ref(inp, defect=defect)
        with pytest.raises(AssertionError):
            L.check_values(L.to_format(bad.float(), out), out, ref, bound, f"{defect} {shape} {out}")
