"""CPU: the float64 attention references and their per-element bounds (tests/attention_refs.py) judged on their own, before a GPU sees them.

* The references agree with oracle/soccdpt_ref.py's window attention (float64, through the fused qkv form: roll, partition, cosine logits, clamp, table, mask,
  reverse, roll back) and with the fp32 torch references of the existing GPU tests on every case geometry.
* Soundness: a kernel emulated in f32 on the CPU -- q^ scale, k^ and the weights rounded to the format with round16, f32 accumulation, 32 keys at a time with the
  online rescale -- lies inside the bound for every element of every case.
* Sharpness: each of attention_refs.DEFECTS, applied to the float64 reference, leaves the bound of every precision in every geometry it can affect.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import soccdpt_ref as R
from tests import attention_refs as AR
from tests.attention_refs import U

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
LOG2E = 1.4426950408889634


def _r(x, fmt):
    """f32 -> the format and back (the kernel's rounding of an operand it hands to the matrix cores)."""
    return x if fmt == "f32" else x.to(DT[fmt]).float()


def _online(logit_tile, v, N, fmt, tile=32):
    """The flash loop in f32: logit_tile(k0, k1) -> [P][N][k1 - k0] f32 logits; weights rounded to fmt for P V, the row sum from the unrounded ones."""
    m = l = o = None
    for k0 in range(0, N, tile):
        k1 = min(N, k0 + tile)
        s = logit_tile(k0, k1)
        mt = s.amax(-1, keepdim=True)
        mn = mt if m is None else torch.maximum(m, mt)
        mnl = mn * LOG2E
        p = torch.exp2(s * LOG2E - mnl)
        pv = _r(p, fmt) @ v[:, k0:k1]
        if m is None:
            l, o = p.sum(-1, keepdim=True), pv
        else:
            alpha = torch.exp2(m * LOG2E - mnl)
            l, o = l * alpha + p.sum(-1, keepdim=True), o * alpha + pv
        m = mn
    return o * (1.0 / l)


def emulate_window(inp, B, res, ws, shift, heads, fmt):
    N, nw = ws * ws, res // ws
    rows = AR.window_rows(B, res, ws, shift)
    masked = AR.window_masked(res, ws, shift)
    bias = inp["table"].float()[AR.bias_index(ws)].permute(2, 0, 1).contiguous()      # [heads][N][N]
    scale = inp["scale"].float().view(heads, 1, 1)
    out = torch.zeros(B * res * res, heads * 32)
    for w in range(rows.shape[0]):
        x = inp["qkv"].float()[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]
        qh = _r(q * (scale / (q * q).sum(-1, keepdim=True).sqrt().clamp(min=1e-12)), fmt)
        kh = _r(k * (1.0 / (k * k).sum(-1, keepdim=True).sqrt().clamp(min=1e-12)), fmt)
        b = bias if masked is None else bias - 100.0 * masked[w % (nw * nw)].float()

        def tile(k0, k1):
            return b[:, :, k0:k1] + qh @ kh[:, k0:k1].transpose(-1, -2)
        out[rows[w]] = _online(tile, v, N, fmt).permute(1, 0, 2).reshape(N, heads * 32)
    return out if fmt == "f32" else out.to(DT[fmt])


def emulate_vit(inp, B, N, heads, fmt):
    x = inp["qkv"].float().reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    out = torch.zeros(B, N, heads * 64)
    for b in range(B):
        q, k, v = _r(x[0, b] * 0.125, fmt), x[1, b], x[2, b]
        out[b] = _online(lambda k0, k1: q @ k[:, k0:k1].transpose(-1, -2), v, N, fmt).permute(1, 0, 2).reshape(N, heads * 64)
    out = out.reshape(B * N, heads * 64)
    return out if fmt == "f32" else out.to(DT[fmt])


def _outside(defective, fmt, ref, bound):
    """Does the check of this precision refuse the defective output (rounded to the output format first, as a kernel would store it)?"""
    got = defective.float() if fmt == "f32" else defective.float().to(DT[fmt])
    try:
        AR.check_output(got, fmt, ref, bound, "defect")
    except AssertionError:
        return True
    return False


WIN_GEOMS = sorted({g for cases in (AR.WIN16_CASES, AR.WINF32_CASES, AR.WINANY_CASES, AR.WINF32_WHOLE_CASES) for g in cases.values()})
EMULATED = [("win16", n, f) for n in AR.WIN16_CASES for f in ("bf16", "f16")] + [("winf32", n, "f32") for n in AR.WINF32_CASES] + \
           [("winany", n, "f32") for n in AR.WINANY_CASES]


# ---------------------------------------------------------------------------------------------------------------------------------
# the references against the project's other statements of the same maths
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", WIN_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_window_reference_matches_the_fp32_torch_reference(geom):
    """_attention_ref of tests/test_kernels_gpu.py (torch fp32: roll, partition, F.normalize, oracle index and mask) on the same f32 operands.  That computation is
    itself an f32 evaluation of the formula, in another order and with a few more roundings than the kernels': it is held to 16 x the f32 kernels' bound."""
    from tests.test_kernels_gpu import _attention_ref
    B, res, ws, shift, heads = geom
    inp, ref, bound = AR.cached(("win", geom, "f32"), lambda: _f32_case(geom))
    ref32 = _attention_ref(inp["qkv"].float(), inp["table"].float(), inp["scale"].float(), B, res, ws, shift, heads).double()
    frac = AR.check_bound(ref32, ref, 16 * bound + 1e-30, f"fp32 torch reference {geom}")
    print(f"window reference {geom}: fp32 torch reference at {frac:.3f} of 16 x the f32 bound")


def _f32_case(geom):
    inp = AR.build_window(*geom, "f32")
    ref, bound = AR.window_attention_ref(inp["qkv"], inp["table"], inp["scale"], *geom, AR.window_model("f32", geom[2]))
    return inp, ref, bound


@pytest.mark.parametrize("geom", [(1, 32, 16, 8, 3), (2, 16, 8, 0, 6), (1, 24, 12, 6, 4), (1, 12, 6, 3, 2)], ids=lambda g: "x".join(map(str, g)))
def test_fused_reference_matches_the_oracle_in_float64(geom):
    """oracle/soccdpt_ref.py window_attention run in float64 with an identity output projection: the same x, Wqkv, q / v bias, a logit_scale parameter above the
    clamp for the scale-100 heads, and the table its CPB MLP produces handed to the reference as the table."""
    B, res, ws, shift, heads = geom
    C = heads * 32
    inp = AR.build_window_qkv(*geom, "f16")
    g = torch.Generator().manual_seed(7)
    sd = {"cpb_mlp.0.weight": torch.randn(16, 2, generator=g, dtype=torch.float64) * 2, "cpb_mlp.0.bias": torch.randn(16, generator=g, dtype=torch.float64),
          "cpb_mlp.2.weight": torch.randn(heads, 16, generator=g, dtype=torch.float64), "qkv.weight": inp["w"], "q_bias": inp["bias"][:C], "v_bias": inp["bias"][2 * C:],
          "logit_scale": torch.where(inp["scale"] >= 100.0, torch.full_like(inp["scale"], math.log(250.0)), inp["scale"].log()).view(heads, 1, 1),
          "proj.weight": torch.eye(C, dtype=torch.float64), "proj.bias": torch.zeros(C, dtype=torch.float64)}
    hid = F.relu(F.linear(R.cpb_coords_table(ws, 0).double(), sd["cpb_mlp.0.weight"], sd["cpb_mlp.0.bias"]))
    table = 16 * torch.sigmoid(F.linear(hid, sd["cpb_mlp.2.weight"]))
    want = R.window_attention(sd, "", inp["x"].reshape(B, res * res, C), res, ws, shift, heads, 0).reshape(B * res * res, C)
    got, _ = AR.window_attention_qkv_ref(inp["x"], inp["w"], inp["bias"], table, inp["scale"], *geom, "f16")
    torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("B,N,heads", AR.VIT_CASES)
def test_vit_reference_matches_torch(B, N, heads):
    inp, ref, bound = AR.vit_case(B, N, heads, "f32")
    x = inp["qkv"].float().reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    ref32 = (torch.softmax((x[0] @ x[1].transpose(-2, -1)) * 64 ** -0.5, dim=-1) @ x[2]).transpose(1, 2).reshape(B * N, heads * 64)
    AR.check_bound(ref32.double(), ref, 16 * bound + 1e-30, f"fp32 torch ViT reference {(B, N, heads)}")


# ---------------------------------------------------------------------------------------------------------------------------------
# soundness
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,name,fmt", EMULATED, ids=lambda v: str(v))
def test_emulated_window_kernel_is_inside_the_bound(family, name, fmt):
    geom = {"win16": AR.WIN16_CASES, "winf32": AR.WINF32_CASES, "winany": AR.WINANY_CASES}[family][name]
    inp, ref, bound = AR.window_case(family, name, fmt)
    frac = AR.check_output(emulate_window(inp, *geom, fmt), fmt, ref, bound, f"emulated {fmt} kernel {geom}")
    assert torch.isfinite(bound).all() and (bound >= 0).all()
    print(f"emulated {fmt} window kernel {geom}: worst element at {frac:.3f} of its allowance")


@pytest.mark.parametrize("fmt", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("B,N,heads", AR.VIT_CASES)
def test_emulated_vit_kernel_is_inside_the_bound(B, N, heads, fmt):
    inp, ref, bound = AR.vit_case(B, N, heads, fmt)
    frac = AR.check_output(emulate_vit(inp, B, N, heads, fmt), fmt, ref, bound, f"emulated {fmt} ViT kernel {(B, N, heads)}")
    assert torch.isfinite(bound).all() and (bound >= 0).all()
    print(f"emulated {fmt} ViT kernel {(B, N, heads)}: worst element at {frac:.3f} of its allowance")


@pytest.mark.parametrize("fmt", ["f16", "x2w", "bf16"])
def test_fused_reference_bound_holds_the_unfused_chain_in_float64(fmt):
    """The fused form's allowance contains the projection error: the unfused float64 attention on q, k, v moved by the whole projection allowance in the worst
    direction of each sign pattern tried stays inside it (and the bound is finite, with the zero k row's exact zero kept)."""
    for name, geom in AR.QKV_CASES.items():
        inp, ref, bound = AR.qkv_case(name, fmt)
        assert torch.isfinite(bound).all() and (bound >= 0).all()
        w = AR.x3_value(inp["w"]) if fmt == "x2w" else inp["w"]
        qkv, err = AR.qkv_projection_ref(inp["x"], w, inp["bias"])
        act = "bf16" if fmt == "bf16" else "f16"
        for seed in (0, 1):
            sign = torch.randint(0, 2, qkv.shape, generator=torch.Generator().manual_seed(seed)).double() * 2 - 1
            moved = qkv + sign * err
            moved[:, 2 * qkv.shape[1] // 3:] = AR.round16(moved[:, 2 * qkv.shape[1] // 3:], act)
            got, _ = AR.window_attention_ref(moved, inp["table"], inp["scale"], *geom, AR.window_model(act, geom[2]))
            AR.check_bound(got, ref, bound, f"fused {fmt} {name}: projection moved by its allowance")


# ---------------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------------
DEFECT_GEOMS = {"ws8": (2, 16, 8, 0, 3), "ws16_shift": (1, 32, 16, 8, 3), "ws12": (1, 12, 12, 0, 2), "ws12_shift": (1, 24, 12, 6, 4), "ws24_shift": (1, 48, 24, 12, 3),
                "ws6_shift": (1, 12, 6, 3, 2), "ws10_shift": (1, 20, 10, 5, 2)}


def _applies(defect, geom):
    B, res, ws, shift, heads = geom
    N = ws * ws
    return {"bias_transposed": True, "roll_reversed": shift > 0, "mask_first": shift > 0, "drop_last_key": True, "pad_bias_zero": N % 32 != 0 and ws in (12, 24),
            "next_head_scale": True, "reverse_swapped": res // ws >= 2, "skip_rescale": N > 32, "swap_v_keys": True}[defect]


@pytest.mark.parametrize("defect", AR.DEFECTS)
def test_defect_leaves_the_window_bound(defect):
    """Every geometry the defect can affect, every precision whose kernels run it: at least one element outside."""
    hidden = []
    for name, geom in DEFECT_GEOMS.items():
        if not _applies(defect, geom):
            continue
        per_key = geom[2] in (6, 10)
        for fmt in (("f32",) if per_key else ("bf16", "f16", "f32")):
            inp, ref, bound = AR.cached(("defect", geom, fmt), lambda: _case(geom, fmt, per_key))
            bad, _ = AR.window_attention_ref(inp["qkv"], inp["table"], inp["scale"], *geom, AR.window_model(fmt, geom[2], per_key), defect=defect)
            if not _outside(bad, fmt, ref, bound):
                hidden.append((name, fmt))
    assert not hidden, f"{defect} stays inside the bound in {hidden}"


def _case(geom, fmt, per_key):
    inp = AR.build_window(*geom, fmt)
    ref, bound = AR.window_attention_ref(inp["qkv"], inp["table"], inp["scale"], *geom, AR.window_model(fmt, geom[2], per_key))
    assert _outside(ref, fmt, ref, bound) is False
    return inp, ref, bound


@pytest.mark.parametrize("defect", AR.DEFECTS)
def test_defect_leaves_the_fused_bound(defect):
    hidden = []
    for name, geom in AR.QKV_CASES.items():
        if not _applies(defect, geom):
            continue
        for fmt in ("f16", "x2w", "bf16"):
            inp, ref, bound = AR.qkv_case(name, fmt)
            w = AR.x3_value(inp["w"]) if fmt == "x2w" else inp["w"]
            bad, _ = AR.window_attention_qkv_ref(inp["x"], w, inp["bias"], inp["table"], inp["scale"], *geom, fmt, defect=defect)
            if not _outside(bad, "bf16" if fmt == "bf16" else "f16", ref, bound):
                hidden.append((name, fmt))
    assert not hidden, f"{defect} stays inside the fused bound in {hidden}"


@pytest.mark.parametrize("defect", ["drop_last_key", "pad_bias_zero", "skip_rescale", "swap_v_keys"])
def test_defect_leaves_the_vit_bound(defect):
    hidden = []
    for B, N, heads in [(1, 33, 12), (1, 577, 12), (22, 100, 12)]:
        for fmt in ("bf16", "f16", "f32"):
            inp, ref, bound = AR.vit_case(B, N, heads, fmt)
            bad, _ = AR.vit_attention_ref(inp["qkv"], B, N, heads, AR.vit_model(fmt, N), defect=defect)
            if not _outside(bad, fmt, ref, bound):
                hidden.append((B, N, heads, fmt))
    assert not hidden, f"{defect} stays inside the ViT bound in {hidden}"


def test_plants_sit_where_they_should():
    """The planted keys of every geometry: cosine exactly 1 after rounding, the key in a later 32-key tile than the query's own; the shifted ones are masked pairs."""
    for geom in WIN_GEOMS:
        B, res, ws, shift, heads = geom
        inp = AR.build_window(*geom, "bf16")
        rows, masked = AR.window_rows(B, res, ws, shift), AR.window_masked(res, ws, shift)
        C = heads * 32
        for w, pq, pk in AR.plants(ws, shift, res // ws):
            assert torch.equal(inp["qkv"][rows[w, pk], C:2 * C], inp["qkv"][rows[w, pq], :C])
            assert bool(masked[w, pq, pk]) if w else masked is None or not bool(masked[w, pq, pk])
        r0 = rows[0]
        assert not inp["qkv"][r0[AR.SPECIAL["q_zero"]], :C].any() and not inp["qkv"][r0[AR.SPECIAL["k_zero"]], C:2 * C].any()
        assert set(float(s) for s in inp["scale"]) <= {1.0, 11.75, 100.0} and float(inp["scale"].max()) == (100.0 if heads >= 3 else 11.75)
        assert float(inp["table"].min()) < 0.5 and float(inp["table"].max()) > 15.5
    assert U == 2.0 ** -24
