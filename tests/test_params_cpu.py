"""CPU: the parameter table of the network (soccdpt_amd/csrc/params.h) without a GPU.

tests/params_main.cpp includes only that header, is built here with the host compiler under the address and undefined-behaviour sanitizers and run
as a child process.  For the three backbones (features 256, 3 classes) it prints every key with its shape in registration order, every typed
reference of the model struct with the index it holds, and every index span.  Checked here, with the expected keys spelt in Python:

  * the key list is soccdpt_amd.model.spec.v3_state_shapes(backbone) without the tensors the HIP path does not consume, in the same order and with
    the same shapes; what is not consumed is stated on its own in tests/consumed_keys.py and once more below (the timm model's final norm and classifier head, refinenet4's unused RCU1);
  * every reference holds the index of the slot whose key its field stands for, every slot is referenced exactly once, and what a backbone lacks
    (the other encoder's tensors, refinenet4.resConfUnit1) is -1;
  * every span holds exactly the indices of the keys under the module prefix it stands for -- or, for a Swin block, of everything at or before
    block (s, j) in forward order: the questions the training backward asks to find where the gradient may stop (train_step.cpp: any_grad)."""
import json
import os
import shutil
import subprocess

import pytest

from soccdpt_amd.model.spec import HYBRID_ARCHS, SWIN_ARCHS, v3_state_shapes
from tests.consumed_keys import ENC, PRE, SCR, consumed_shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKBONES = ("swin2t16_256", "swin2b24_384", "vitb_rn50_384")

@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("params")
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "params_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "params_main.cpp"), "-o", exe]
    # (as tests/test_train_plan_cpu.py: gcc's sanitizer runtimes linked into the program where the static archives exist)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout
    if is_clang or subprocess.run([*cmd, "-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]     # a sanitizer report goes to stderr and ends the program with a non-zero status
    out = {t["backbone"]: t for t in map(json.loads, r.stdout.splitlines())}
    assert tuple(out) == BACKBONES
    return out


# ---------------- the expected key of every field, spelt here ----------------
def _wb(out, field, module):
    out[field + ".w"], out[field + ".b"] = module + ".weight", module + ".bias"


def _gb(out, field, module):
    out[field + ".g"], out[field + ".b"] = module + ".weight", module + ".bias"


def expected_refs(backbone):
    """field path of ModelP -> state-dict key, None where this backbone has no such tensor"""
    e = {}
    hybrid = backbone in HYBRID_ARCHS
    # Swin-V2 encoder
    _wb(e, "swin.patch", ENC + "patch_embed.proj")
    _gb(e, "swin.patch_norm", ENC + "patch_embed.norm")
    for s in range(3):
        d = f"{ENC}layers.{s}.downsample."
        e[f"swin.merge.{s}.red_w"] = d + "reduction.weight"
        _gb(e, f"swin.merge.{s}.norm", d + "norm")
    if hybrid:
        e = dict.fromkeys(e)
    else:
        for s, depth in enumerate(SWIN_ARCHS[backbone].depths):
            for j in range(depth):
                f, b = f"swin.blk.{s}.{j}", f"{ENC}layers.{s}.blocks.{j}."
                for field, name in (("logit_scale", "attn.logit_scale"), ("q_bias", "attn.q_bias"), ("v_bias", "attn.v_bias"), ("cpb0_w", "attn.cpb_mlp.0.weight"),
                                    ("cpb0_b", "attn.cpb_mlp.0.bias"), ("cpb2_w", "attn.cpb_mlp.2.weight"), ("qkv_w", "attn.qkv.weight")):
                    e[f"{f}.{field}"] = b + name
                _wb(e, f + ".proj", b + "attn.proj")
                _gb(e, f + ".n1", b + "norm1")
                _wb(e, f + ".fc1", b + "mlp.fc1")
                _wb(e, f + ".fc2", b + "mlp.fc2")
                _gb(e, f + ".n2", b + "norm2")
    # ViT-hybrid encoder
    h = {"hy.cls": ENC + "cls_token", "hy.pos": ENC + "pos_embed", "hy.stem_w": ENC + "patch_embed.backbone.stem.conv.weight"}
    _gb(h, "hy.stem_n", ENC + "patch_embed.backbone.stem.norm")
    _wb(h, "hy.pe", ENC + "patch_embed.proj")
    for k in range(2):
        _wb(h, f"hy.ro.{k}.project", f"{PRE}act_postprocess{3 + k}.0.project.0")
        _wb(h, f"hy.ro.{k}.conv", f"{PRE}act_postprocess{3 + k}.3")
    _wb(h, "hy.pp4", PRE + "act_postprocess4.4")
    if not hybrid:
        h = dict.fromkeys(h)
    else:
        arch = HYBRID_ARCHS[backbone]
        i = 0
        for s, depth in enumerate(arch.layers):
            for j in range(depth):
                f, b = f"hy.rn.{i}", f"{ENC}patch_embed.backbone.stages.{s}.blocks.{j}."
                h[f + ".ds_w"] = b + "downsample.conv.weight" if j == 0 else None
                _gb(h, f + ".ds_n", b + "downsample.norm")
                if j:
                    h[f + ".ds_n.g"] = h[f + ".ds_n.b"] = None
                for c in (1, 2, 3):
                    h[f"{f}.c{c}_w"] = b + f"conv{c}.weight"
                    _gb(h, f"{f}.n{c}", b + f"norm{c}")
                i += 1
        for i in range(arch.depth):
            f, b = f"hy.vit.{i}", f"{ENC}blocks.{i}."
            _gb(h, f + ".n1", b + "norm1")
            _wb(h, f + ".qkv", b + "attn.qkv")
            _wb(h, f + ".proj", b + "attn.proj")
            _gb(h, f + ".n2", b + "norm2")
            _wb(h, f + ".fc1", b + "mlp.fc1")
            _wb(h, f + ".fc2", b + "mlp.fc2")
    e.update(h)
    # decoder and heads
    for l in range(4):
        e[f"layer_rn.{l}"] = f"{SCR}layer{l + 1}_rn.weight"
        _wb(e, f"refine.{l}.out_conv", f"{SCR}refinenet{l + 1}.out_conv")
        for u in range(2):
            for c in (1, 2):
                _wb(e, f"refine.{l}.rcu.{u}.c{c}", f"{SCR}refinenet{l + 1}.resConfUnit{u + 1}.conv{c}")
                if l == 3 and u == 0:
                    e[f"refine.{l}.rcu.{u}.c{c}.w"] = e[f"refine.{l}.rcu.{u}.c{c}.b"] = None
    for c in (0, 2, 4):
        _wb(e, f"depth.c{c}", f"{SCR}output_conv.{c}")
    e["seg.c0_w"] = "seg_head.0.weight"
    _gb(e, "seg.bn", "seg_head.1")
    e["seg.bn_mean"], e["seg.bn_var"] = "seg_head.1.running_mean", "seg_head.1.running_var"
    _wb(e, "seg.c4", "seg_head.4")
    return e


def expected_spans(backbone):
    """span path -> predicate over keys, as prefix compares"""
    def prefix(*ps):
        return lambda k: k.startswith(ps)
    e = {"encoder": prefix(PRE)}
    for l in range(4):
        rb = f"{SCR}refinenet{l + 1}."
        e[f"refine.{l}.out_conv"] = prefix(rb + "out_conv")
        for u in range(2):
            e[f"refine.{l}.rcu.{u}"] = prefix(rb + f"resConfUnit{u + 1}")
    never = lambda k: False
    depths = (0, 0, 0, 0) if backbone in HYBRID_ARCHS else SWIN_ARCHS[backbone].depths      # (the hybrid's backward never asks: empty spans)
    for s in range(4):
        below = [ENC + "patch_embed."] + [f"{ENC}layers.{t}." for t in range(s)]
        e[f"swin.below.{s}"] = prefix(*below) if depths[s] else never
        for j in range(depths[s]):
            e[f"swin.blk.{s}.{j}.upto"] = prefix(*below, *[f"{ENC}layers.{s}.blocks.{i}." for i in range(j + 1)])      # at or before block (s, j)
    return e


# ---------------- the checks ----------------
@pytest.mark.parametrize("backbone", BACKBONES)
def test_key_list_is_the_consumed_state_dict(tables, backbone):
    got = [(k, tuple(shape)) for k, shape in tables[backbone]["keys"]]
    assert got == consumed_shapes(backbone)
    dropped = set(v3_state_shapes(backbone)) - {k for k, _ in got}
    enc = ENC
    assert dropped == {enc + "norm.weight", enc + "norm.bias", enc + "head.weight", enc + "head.bias"} | {
        f"{SCR}refinenet4.resConfUnit1.conv{c}.{p}" for c in (1, 2) for p in ("weight", "bias")}


@pytest.mark.parametrize("backbone", BACKBONES)
def test_every_reference_points_at_its_key(tables, backbone):
    t = tables[backbone]
    keys = [k for k, _ in t["keys"]]
    want = expected_refs(backbone)
    assert set(t["refs"]) == set(want)
    for field, idx in t["refs"].items():
        if want[field] is None:
            assert idx == -1, field
        else:
            assert 0 <= idx < len(keys) and keys[idx] == want[field], (field, idx)
    held = sorted(i for i in t["refs"].values() if i >= 0)
    assert held == list(range(len(keys)))             # each slot exactly once: nothing registered but unreachable, nothing referenced twice


def test_bottleneck_geometry(tables):
    arch = HYBRID_ARCHS["vitb_rn50_384"]
    want, prev, r = [], arch.stem, arch.img // 4
    for s, depth in enumerate(arch.layers):
        cout = 256 << s
        for j in range(depth):
            stride = 2 if (j == 0 and s > 0) else 1
            want.append([prev, cout, cout // 4, stride, r, r // stride, int(j == 0)])
            prev, r = cout, r // stride
    assert tables["vitb_rn50_384"]["rn"] == want
    assert tables["swin2t16_256"]["rn"] == [] and tables["swin2b24_384"]["rn"] == []


@pytest.mark.parametrize("backbone", BACKBONES)
def test_spans_hold_what_the_prefix_compares_matched(tables, backbone):
    t = tables[backbone]
    keys = [k for k, _ in t["keys"]]
    want = expected_spans(backbone)
    assert set(t["spans"]) == set(want)
    for name, (lo, hi) in t["spans"].items():
        assert 0 <= lo <= hi <= len(keys), name
        assert set(range(lo, hi)) == {i for i, k in enumerate(keys) if want[name](k)}, name
    # layer<l>_rn is asked about as the one-tensor span of its reference
    for l in range(4):
        assert [i for i, k in enumerate(keys) if k.startswith(f"{SCR}layer{l + 1}_rn")] == [t["refs"][f"layer_rn.{l}"]]
