"""CPU: the scratch plans of the training backward (soccdpt_amd/csrc/train_plan.h) without a GPU.

tests/train_plan_main.cpp includes only the plan header, is built here with the host compiler under the address and undefined-behaviour sanitizers
and run as a child process.  It plans every shape of the grid below in the four operand formats and for every request (dX only, dW only, both; with
and without a staged weight; the sum deferred or not) and prints, per plan, the decisions, the layout numbers, the need and what the helpers write
and read with those numbers.  Checked here, for every plan:

  * the operand format and the weight-gradient path are what the rules give -- stated below in Python, independently of the header -- and, for the
    case tables of tests/test_train_layer_bwd_gpu.py, what that module expects of the GPU;
  * everything a helper writes into a region (each copy, each zeroed head, margin and tail) and the over-read allowance are pairwise disjoint and
    lie inside the need; every tap view of a shifted-view GEMM reads only what was written, inside ONE copy;
  * the alignment contracts: x3 view starts, pitches and row strides are multiples of 16 elements, 16-bit TN strides multiples of 8, every 16-bit tap
    base of the halo-shift layout 4-byte aligned, the weight row groups multiples of 64;
  * fits() accepts the need itself and refuses a capacity one float short, one region at a time.

What this does not check: the spans and views are the driver's statement of what linear_bwd / conv3_bwd / conv_gen_bwd do with a plan's numbers
(memset lengths, copy bases, the igemm's tap shifts), not taken from the helpers themselves.  It pins the header's arithmetic and the tightness of the
need; that the helpers execute the plan this way is held by tests/test_train_layer_bwd_gpu.py (0xFF scratch sized by the same need, guards, float64).
The one rule here that is not the parent's: 16-bit halo-shift needs an even r + 2 (4-byte aligned vertical taps), odd r takes im2col^T.

The grid: the CONV3 / LINEAR / CONV_GEN tables of the GPU module, every backward layer of the three models at B = 1, 2, 3, 4, 8 (shapes from
soccdpt_amd/model/spec.py), and edge shapes (r = 1, 2, 14; M one below / above a k-tile multiple)."""
import json
import os
import shutil
import subprocess

import pytest

from soccdpt_amd.model.spec import HYBRID_ARCHS, SWIN_ARCHS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = {"f32": 4, "bf16": 2, "f16": 2, "x3": 4}
REGIONS = ("S_T1", "S_T2", "S_halo", "S_wt", "S_dw")
F = 256                     # decoder features
BATCHES = (1, 2, 3, 4, 8)


def up(v, m):
    return (v + m - 1) // m * m


# ---------------- the grid ----------------
def decoder_layers(B, fres, fdim):
    out = []
    r1, r0 = 2 * fres[0], 4 * fres[0]
    out += [("C", B, r0, 32, F // 2), ("C", B, r1, F // 2, F), ("C", B, r1, F, F)]          # output_conv.2 (N = 32), output_conv.0, seg_head.0
    for r, c in zip(fres, fdim):
        out += [("L", B * r * r, F, F), ("C", B, r, F, F), ("C", B, r, F, c)]                 # out_conv, the RCU convolutions, layer_rn (tiny_256: C = 96)
    return out


def swin_layers(arch, B):
    out = []
    for s in range(4):
        C, res = arch.embed << s, arch.grid >> s
        M = B * res * res
        out += [("L", M, C, 4 * C), ("L", M, 4 * C, C), ("L", M, C, C), ("L", M, 3 * C, C)]   # fc2, fc1, proj, qkv
        if s > 0:
            out.append(("L", M, C, 4 * (C // 2)))                                           # PatchMerging reduction
    out.append(("L", B * arch.grid ** 2, arch.embed, 64))                                    # the padded patch embedding (K = 64)
    return out + decoder_layers(B, [arch.grid >> l for l in range(4)], [arch.embed << l for l in range(4)])


def hybrid_layers(arch, B):
    E, G = arch.embed, arch.grid
    Mt, Mp = B * (G * G + 1), B * G * G                                                       # 577 tokens per sample
    out = [("L", Mt, E, 4 * E), ("L", Mt, 4 * E, E), ("L", Mt, E, E), ("L", Mt, 3 * E, E),
           ("G", B, G, G // 2, 768, 768, 2, 1), ("L", Mp, 768, E), ("L", Mp, E, 2 * E), ("L", Mp, E, 1024),
           ("L", B * (arch.img // 2) ** 2, arch.stem, 160)]                                  # the stem's 7 x 7 as a GEMM
    prev, r = arch.stem, arch.img // 4
    for s, n in enumerate(arch.layers):                                                       # ResNetV2 bottlenecks
        cout = 256 << s
        mid = cout // 4
        for j in range(n):
            stride = 2 if (j == 0 and s > 0) else 1
            rout = r // stride
            out += [("L", B * rout * rout, cout, mid), ("G", B, r, rout, mid, mid, stride, 1 if stride == 1 else 0), ("L", B * r * r, mid, prev)]
            if j == 0:
                out.append(("L", B * rout * rout, cout, prev))
            prev, r = cout, rout
    return out + decoder_layers(B, [arch.img // 4, arch.img // 8, G, G // 2], list(arch.features))


def gpu_table_shapes():
    from tests import test_train_layer_bwd_gpu as T
    return ([("C", *s) for s, _ in T.CONV3.values()] + [("L", *s) for s, _ in T.LINEAR.values()] + [("G", *s) for s, _ in T.CONV_GEN.values()])


EDGES = ([("C", B, r, N, C) for r in (1, 2, 14) for B in (1, 2, 8, 30) for N, C in ((32, 64), (128, 128), (64, 96), (12, 32), (256, 192))]
         + [("L", M, N, K) for M in (255, 256, 257, 319, 321, 127, 129, 1) for N, K in ((96, 128), (64, 32), (96, 36), (128, 64), (100, 64))]
         + [("G", B, H, H, N, N, 1, 1) for H in (1, 2, 14) for B in (1, 8) for N in (64, 128)] + [("G", 2, 14, 7, 128, 128, 2, 0), ("G", 2, 13, 7, 128, 128, 2, 1)])


def grid():
    shapes = gpu_table_shapes() + EDGES
    for B in BATCHES:
        for a in SWIN_ARCHS.values():
            shapes += swin_layers(a, B)
        shapes += hybrid_layers(HYBRID_ARCHS["vitb_rn50_384"], B)
    return sorted(set(shapes), key=str)


# ---------------- the rules, as the sources state them ----------------
def tn_ok(K, N, C, taps):
    if K % 64 or K < 256:
        return False
    return (N % 128 == 0 and C % 128 == 0) if taps == 9 else (N % 32 == 0 and C % 32 == 0)


def expect(kind, shape, mode, dW):
    """-> (operand format, weight-gradient path)"""
    if kind == "linear":
        M, N, K = shape
        ok = N % 32 == 0 and K > 32 and (K % 32 == 0 if mode == "x3" else K % 4 == 0)
        fmt = mode if ok else "f32"
        path = "tn" if fmt != "f32" and tn_ok(up(M, 64), N, K, 1) else "transpose"
    elif kind == "conv3":
        B, r, N, C = shape
        fmt = mode if N % 32 == 0 and C % 32 == 0 else "f32"
        if fmt != "f32" and tn_ok(up(B * (r + 2) ** 2, 64), N, C, 9):
            path = "tn"
        elif fmt == "x3" and C % 64 == 0:
            path = "x3shift"
        elif C % 64 or fmt == "x3" or (fmt in ("bf16", "f16") and r % 2):       # an odd pixel pitch would leave the 16-bit vertical taps 2-byte aligned
            path = "im2colT"
        else:
            path = "haloshift"
    else:
        B, Hi, Ho, N, C, stride, pad = shape
        ok = mode in ("bf16", "f16") and stride == 1 and pad == 1 and Hi == Ho and tn_ok(up(B * (Ho + 2) ** 2, 64), N, C, 9)
        fmt = mode if ok else "f32"
        path = "tn" if ok else "im2colT"
    return fmt, (path if dW else "none")


# ---------------- the run ----------------
@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_plan")
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(d / "train_plan_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(REPO, "tests", "train_plan_main.cpp"), "-o", exe]
    # (as tests/test_calib_select_cpu.py: gcc's sanitizer runtimes linked into the program where the static archives exist)
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout
    if is_clang or subprocess.run([*cmd, "-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    shapes = grid()
    path = d / "shapes.txt"
    path.write_text("".join(" ".join(str(v) for v in s) + "\n" for s in shapes))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]     # a sanitizer report goes to stderr and ends the program with a non-zero status
    out = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(out) == len(shapes) * 4 * 3 * 2 * 2
    return out


def _tag(p):
    return f"{p['kind']} {p['in']} {p['mode']} dX={p['dX']} dW={p['dW']} staged={p['staged']} defer={p['defer']}"


def test_grid_holds_what_it_should(plans):
    seen = {(p["kind"], tuple(p["in"])) for p in plans}
    assert ("conv3", (1, 64, 256, 96)) in seen                  # tiny_256's layer1_rn
    assert ("linear", (2 * 577, 2304, 768)) in seen             # a 577-token ViT Linear
    assert ("conv_gen", (3, 96, 48, 128, 128, 2, 0)) in seen    # the strided ResNetV2 3x3
    assert ("conv3", (8, 256, 32, 128)) in seen                 # output_conv.2
    assert ("linear", (4 * 96 * 96, 128, 64)) in seen           # the padded patch embedding of base_384
    assert {p["wgrad"] for p in plans} == {"none", "tn", "transpose", "x3shift", "im2colT", "haloshift"}
    assert {(p["fmt"], p["wgrad"]) for p in plans} >= {(f, "haloshift") for f in ("f32", "bf16", "f16")} | {(f, "tn") for f in ("bf16", "f16", "x3")}


def test_decisions_follow_the_rules(plans):
    for p in plans:
        assert (p["fmt"], p["wgrad"]) == expect(p["kind"], p["in"], p["mode"], p["dW"]), _tag(p)


def test_decisions_are_what_the_gpu_module_expects(plans):
    from tests import test_train_layer_bwd_gpu as T
    by = {(p["kind"], tuple(p["in"]), p["mode"]): p for p in plans if p["dX"] == 0 and p["dW"] and p["staged"] and p["defer"]}
    for kind, table in (("conv3", T.CONV3), ("linear", T.LINEAR), ("conv_gen", T.CONV_GEN)):
        for case, (shape, routes) in table.items():
            for mode, route in routes.items():
                p = by[(kind, tuple(shape), mode)]
                assert (p["fmt"], p["wgrad"]) == (route.fmt, route.wgrad), (kind, case, mode)


def _union(intervals):
    out = []
    for lo, hi in sorted(intervals):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def test_sub_buffers_are_disjoint_and_inside_the_need(plans):
    for p in plans:
        es = ES[p["fmt"]]
        per = {}
        for region, label, lo, hi in p["spans"]:
            assert 0 <= lo < hi <= 4 * p["need"][region], (_tag(p), REGIONS[region], label, lo, hi, p["need"])
            per.setdefault(region, []).append((lo, hi, label))
        for region, spans in per.items():
            spans.sort()
            for a, b in zip(spans, spans[1:]):
                assert a[1] <= b[0], (_tag(p), REGIONS[region], a, b)
        for i, n in enumerate(p["need"]):               # nothing is asked for that no span accounts for
            assert (n > 0) == (i in per), (_tag(p), REGIONS[i])
            if n and not (p["wgrad"] == "haloshift" and i == 1):       # (the halo-shift copy stride leaves a row and 64 elements behind each image)
                assert 4 * n - max(hi for _, hi, _ in per[i]) < 4, (_tag(p), REGIONS[i])
        # every tap view reads written elements only, inside S_T2's need and inside one copy
        written = _union([(lo, hi) for r, label, lo, hi in p["spans"] if r == 1 and label != "over-read"])
        assert len(p["views"]) == (9 if p["wgrad"] in ("tn", "x3shift", "haloshift") and p["kind"] != "linear" else 0), _tag(p)
        for first, end in p["views"]:
            assert 0 <= first and end * es <= 4 * p["need"][1], (_tag(p), first, end)
            assert any(lo <= first * es and end * es <= hi for lo, hi in written), (_tag(p), first, end, written)
            if p["wgrad"] != "tn":
                assert first // p["copy"] == (end - 1) // p["copy"] < p["ncopies"], (_tag(p), first, end)


def test_alignment_contracts(plans):
    for p in plans:
        if p["wgrad"] == "tn":
            m = 16 if p["fmt"] == "x3" else 8
            assert p["ldA"] % m == 0 and p["ldB"] % m == 0, _tag(p)
            assert (p["Mtn"] if p["kind"] == "linear" else p["Kp"]) % 64 == 0
        if p["wgrad"] == "x3shift":
            assert p["fmt"] == "x3" and p["ncopies"] == 3
            for k in ("ld", "rpp", "head", "copy"):
                assert p[k] % 16 == 0, (_tag(p), k)
            assert all(first % 16 == 0 for first, _ in p["views"]), _tag(p)
        if p["wgrad"] == "haloshift":
            assert p["ncopies"] == (2 if p["fmt"] in ("bf16", "f16") else 1) and p["ld"] % 128 == 0
            assert all(first * ES[p["fmt"]] % 4 == 0 for first, _ in p["views"]), _tag(p)
        if p["wgrad"] in ("x3shift", "haloshift"):
            assert p["wt_grp_rows"] % 64 == 0, _tag(p)
        if p["wgrad"] in ("transpose", "im2colT"):
            assert p["Mp"] % (128 if p["fmt"] in ("bf16", "f16") else 32) == 0, _tag(p)


def test_fits_refuses_one_float_short(plans):
    for p in plans:
        assert p["fits"] == 1
        assert all(s == 0 for s, n in zip(p["short"], p["need"]) if n) and all(s is None for s, n in zip(p["short"], p["need"]) if not n), _tag(p)
