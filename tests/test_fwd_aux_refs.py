"""CPU: the float64 references and bounds of tests/fwd_aux_refs.py are tight enough to catch subtle faults and loose enough for a correct f32 evaluation.

Per kind, three things: the reference's own output, rounded to f32 as a kernel stores it, passes its check; the same operation with ONE planted fault is
rejected (align_corners flipped -- False where True is due for the resampling, True where False is due for the position embedding --, merge blocks (1,0)
and (0,1) exchanged, unbiased variance, eps 1e-5 <-> 1e-6, 'SAME' padding put in front, the position row off by one, the CPB denominator ws - 1 where
pws - 1 is due, BatchNorm folded with sqrt(var) + eps); and torch's own f32 CPU evaluation of the CORRECT operation passes the same bound, so the bound
is not so tight that a correct f32 kernel must fail.  (Weight standardisation is the exception the kernel itself makes: its statistics are f64 sums, so
the stand-in takes f64 statistics and does the rest in f32.)  The input builders' promises (max-pool windows decided by 1e-3, all-zero windows present,
low-variance and shifted LayerNorm rows present) are checked here too, and the binding's kind table against the header."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import fused_refs as FR
from tests import fwd_aux_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rejects(got, ref, bound, what):
    with pytest.raises(AssertionError):
        FR.check_bound(got, ref, bound, what)


def _ln32(v, g, b, eps):
    return F.layer_norm(v.float(), (v.shape[-1],), g.float(), b.float(), eps)


def test_kind_table_follows_the_header():
    from soccdpt_amd import lib
    header = open(os.path.join(REPO, "include", "soccdpt_hip.h")).read()
    defs = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define\s+SOCCDPT_FWD_([A-Z0-9_]+)\s+(\d+)\b", header) if not m.group(1).startswith("PATH")}
    assert defs.pop("kinds") == len(R.KINDS) == len(lib.FWD_KINDS)
    assert defs == {k: i for i, k in enumerate(R.KINDS)} == lib.FWD
    assert (lib.FWD_PATH_LN_SCALAR, lib.FWD_PATH_LN_V4) == (R.PATH_LN_SCALAR, R.PATH_LN_V4) == (0x100, 0x200)
    for k in R.KINDS:
        assert re.search(r"^ \*   " + k.upper() + r"\s", header, flags=re.M), f"{k}: no line in the header's per-kind comment"


def test_patch_embed_bound():
    for case in ("1x32x96", "1x32x40", "1x32x96_shifted"):
        inp = R.build_patch(case)
        ref, bound = R.ref_patch(inp)["xf"]
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        _rejects(R.ref_patch(inp, unbiased=True)["xf"][0].float(), ref, bound, "unbiased variance")
        C0 = inp["w"].shape[0]
        v32 = F.conv2d(inp["x"].float(), inp["w"].float().view(C0, 3, 4, 4), inp["bias"].float(), stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
        r = FR.check_bound(_ln32(v32, inp["g"], inp["beta"], 1e-5), ref, bound, "torch f32")
        print(f"patch_embed {case}: torch f32 at {r:.3f} of the bound")
    inp = R.build_patch("1x32x96_shifted")
    assert float(inp["bias"].mean()) > 25          # the rows of this case are shifted: a mean of 30 against a spread of about 1


def test_ln_residual_bound():
    for case in ("c100_m5", "c768_m23", "rowscale_c96", "c768_shifted", "c100_shifted", "c1000_m7"):
        inp = R.build_ln(case)
        c = R.LN_CASES[case]
        ref, bound = R.ref_ln(case, inp)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        _rejects(R.ref_ln(case, inp, eps=1e-6)[0].float(), ref, bound, "eps 1e-6")
        _rejects(R.ref_ln(case, inp, unbiased=True)[0].float(), ref, bound, "unbiased variance")
        t32 = _ln32(inp["y"], inp["g"], inp["beta"], 1e-5)
        if c.rps:
            t32 = t32 * inp["row_scale"].float()[torch.arange(c.M) // c.rps][:, None]
        if c.residual:
            t32 = t32 + inp["xf0"].float()
        r = FR.check_bound(t32, ref, bound, "torch f32")
        print(f"ln_residual {case}: torch f32 at {r:.3f} of the bound")
    y, _, _ = R.ln_inputs(7, 100, 21, shifted=True)
    assert float(y[3].mean().abs() / y[3].std()) > 50 and float(y[0].std()) < 0.02      # a shifted and a low-variance row


def test_every_ln_instantiation_has_a_case():
    paths = {c.path for c in R.LN_CASES.values()}
    assert paths == {R.PATH_LN_SCALAR | v for v in (2, 4, 8, 12, 16)} | {R.PATH_LN_V4 | v for v in (1, 2, 3, 4)}
    for c in R.LN_CASES.values():
        want = R.PATH_LN_V4 | (c.C // 256) if c.C % 256 == 0 else R.PATH_LN_SCALAR | min(v for v in (2, 4, 8, 12, 16) if v >= -(-c.C // 64))
        assert c.path == want
    assert {c.M for c in R.LN_CASES.values()} >= {1, 5, 7, 23}


def test_merge_layouts():
    x = torch.arange(2 * 6 * 6 * 4, dtype=torch.float64).reshape(72, 4)
    m = R.merge_layout(x, 2, 6)
    # timm PatchMerging: cat(x[0::2, 0::2], x[1::2, 0::2], x[0::2, 1::2], x[1::2, 1::2])
    img = x.reshape(2, 6, 6, 4)
    assert torch.equal(m.reshape(2, 3, 3, 16)[1, 2, 0], torch.cat([img[1, 4, 0], img[1, 5, 0], img[1, 4, 1], img[1, 5, 1]]))
    assert not torch.equal(m, R.merge_layout_swapped(x, 2, 6))
    sym = torch.ones(8, 4, dtype=torch.float64)           # a symmetric image cannot tell the two: the builders are not symmetric
    assert torch.equal(R.merge_layout(sym, 2, 2), R.merge_layout_swapped(sym, 2, 2))
    for shape in R.MERGE_SHAPES[:3]:
        inp = R.build_merge(shape)["in"]
        assert not torch.equal(R.merge_layout(inp, shape[0], shape[1]), R.merge_layout_swapped(inp, shape[0], shape[1]))


def test_bilinear_bound():
    for name, shape in R.BILINEAR_SHAPES.items():
        B, h, w, H, W = shape
        inp = R.build_bilinear(shape, 12)
        ref, bound = R.ref_bilinear(inp, shape)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        if (h, w) != (H, W) and min(H, W) > 1:
            _rejects(R.ref_bilinear(inp, shape, align_corners=False)[0].float(), ref, bound, f"{name}: align_corners=False")
        got = F.interpolate(inp["in"].float().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
        r = FR.check_bound(got, ref, bound, "torch f32")
        print(f"bilinear {name}: torch f32 at {r:.3f} of the bound")
    # a weight that is off by 1e-3 on the last row is rejected
    shape = R.BILINEAR_SHAPES["nonint"]
    inp = R.build_bilinear(shape, 12)
    ref, bound = R.ref_bilinear(inp, shape)
    got = ref.clone()
    got[:, -2] = ref[:, -2] + 1e-3 * (ref[:, -1] - ref[:, -2])
    _rejects(got.float(), ref, bound, "a weight off by 1e-3")
    # the 16-bit interval rule
    R.check_interval16(ref.to(torch.bfloat16), ref, bound, "bf16", "rounded reference")
    off = ref.to(torch.bfloat16).clone()
    off.view(torch.int16)[0, 1, 1, 3] += 1
    with pytest.raises(AssertionError):
        R.check_interval16(off, ref, bound, "bf16", "one ulp off")


def test_seg_tail_bound():
    for fmt in (0, 1, 2):
        inp = R.build_seg((1, 3, 6), fmt)
        ref, bound = R.ref_seg_logits(inp)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        sw = ref.float().clone()
        sw[:, [1, 2]] = sw[:, [2, 1]]
        _rejects(sw, ref, bound, "classes 1 and 2 swapped")
        got = inp["feat"].float() @ inp["w"].float().t() + inp["bias"].float()
        r = FR.check_bound(got, ref, bound, "torch f32")
        print(f"seg logits fmt {fmt}: torch f32 at {r:.3f} of the bound")
        for sigmoid in (0, 1):
            act, ab = FR.seg_up_act_ref(got.double(), 1, 3, 6, sigmoid)
            up = F.interpolate(got.reshape(1, 3, 6, 3).permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
            FR.check_bound(torch.sigmoid(up) if sigmoid else 0.5 * torch.tanh(up) + 0.5, act, ab, "torch f32 activation")
            _rejects(FR.seg_activation(up.double(), 1 - sigmoid).float(), act, ab, "the other activation")


def test_cvt_expectations():
    x = R.build_cvt(1000, 1)["in"]
    assert float(x[torch.isfinite(x)].abs().max()) > 1e6 and bool(torch.isinf(x).any())
    big = torch.tensor([65519.0, 65520.0, 7.0e4, float("inf"), -65520.0, float("-inf")], dtype=torch.float64)
    assert R.expect_cvt(big, 1).double().tolist() == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, -65504.0]          # half16.h: saturates at +-65504
    assert R.expect_cvt(big, 5).double().tolist() == [65504.0, float("inf"), float("inf"), float("inf"), float("-inf"), float("-inf")]
    assert bool(torch.isfinite(R.build_cvt(1008, 3)["in"]).all()) and float(R.build_cvt(1008, 3)["in"].abs().max()) < 65520


def test_small_weight_kernels_bounds():
    inp = R.build_bn_fold(100)
    ref = R.ref_bn_fold(inp)
    bad = R.ref_bn_fold(inp, eps_outside=True)
    s32 = inp["g"].float() / torch.sqrt(inp["var"].float() + 1e-5)
    t32 = {"scale": s32, "shift": inp["b"].float() - inp["mean"].float() * s32}
    for k in ("scale", "shift"):
        FR.check_bound(ref[k][0].float(), *ref[k], "unmodified")
        _rejects(bad[k][0].float(), *ref[k], "sqrt(var) + eps")
        FR.check_bound(t32[k], *ref[k], "torch f32")
    inp = R.build_logit_scale(100)
    ref, bound = R.ref_logit_scale(inp)
    assert bool((inp["ls"] > R.LN100_F32).any()) and bool((inp["ls"] < R.LN100_F32).any())
    assert float(ref.max()) == float(torch.tensor(R.LN100_F32, dtype=torch.float64).exp())
    FR.check_bound(inp["ls"].float().clamp(max=R.LN100_F32).exp(), ref, bound, "torch f32")
    _rejects(inp["ls"].float().exp(), ref, bound, "no clamp")
    inp = R.build_conv_w("3x5")
    ref, bound = R.ref_conv_w(inp, True)
    FR.check_bound((inp["w"].float() * inp["scale"].float()[:, None, None, None]).permute(0, 2, 3, 1), ref, bound, "torch f32")
    _rejects(R.ref_conv_w(inp, False)[0].float(), ref, bound, "scale dropped")
    assert not torch.equal(R.ref_conv_w(inp, False)[0], inp["w"].permute(0, 3, 2, 1).contiguous())          # ky / kx exchanged is another tensor


def test_cpb_bound():
    for case in R.CPB_CASES:
        ws, pws, H = case
        inp = R.build_cpb(case)
        ref, bound = R.ref_cpb(case, inp)
        assert ref.shape == ((2 * ws - 1) ** 2, H)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        if pws and pws != ws:
            _rejects(R.ref_cpb(case, inp, denom_ws=True)[0].float(), ref, bound, "denominator ws - 1")
        T = 2 * ws - 1
        d = (torch.arange(T, dtype=torch.float32) - (ws - 1)) / float((pws or ws) - 1) * 8
        c = d.sign() * torch.log2(d.abs() + 1) / 3
        coords = torch.stack([c[:, None].expand(T, T), c[None, :].expand(T, T)], -1).reshape(-1, 2)
        got = 16 * torch.sigmoid(torch.relu(coords @ inp["w0"].float().t() + inp["b0"].float()) @ inp["w2"].float().t())
        r = FR.check_bound(got, ref, bound, "torch f32")
        print(f"cpb_table {case}: torch f32 at {r:.3f} of the bound, largest bound {float(bound.max()):.2e}")
        assert float(bound.max()) < 16 * 2.0 ** -12          # the serial 512-term sum dominates: still below 2^-12 of the table's range
    assert any(p and p != w for w, p, _ in R.CPB_CASES) and any(p == 0 for _, p, _ in R.CPB_CASES)
    assert (1536 + 512 * R.CPB_TOO_MANY_HEADS) * 4 > 160 * 1024 >= (1536 + 512 * (R.CPB_TOO_MANY_HEADS - 1)) * 4


def test_ws_conv_w_bound():
    for case, (Cout, Cin, k, Kpad) in R.WS_CASES.items():
        inp = R.build_ws(case)
        ref, bound = R.ref_ws(case, inp)
        fan = Cin * k * k
        assert ref.shape == (Cout, Kpad) and bool((ref[:, fan:] == 0).all()) and bool((bound[:, fan:] == 0).all())
        assert bool((ref[-1] == 0).all()) and float(bound[-1, :fan].min()) > 0          # the all-equal filter: 0, governed by eps
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        _rejects(R.ref_ws(case, inp, unbiased=True)[0].float(), ref, bound, "unbiased variance")
        _rejects(R.ref_ws(case, inp, eps=1e-5)[0].float(), ref, bound, "eps 1e-5")
        w = inp["w"].reshape(Cout, fan)
        mean = w.mean(1, keepdim=True)
        rstd = 1 / (((w - mean) ** 2).mean(1, keepdim=True) + R.WS_EPS).sqrt()
        got = ((w.float() - mean.float()) * rstd.float()).reshape(Cout, Cin, k * k).permute(0, 2, 1).reshape(Cout, fan)      # f64 statistics as in the kernel, f32 arithmetic
        r = FR.check_bound(F.pad(got, (0, Kpad - fan)), ref, bound, "f64 statistics, f32 arithmetic")
        print(f"ws_conv_w {case}: f32 at {r:.3f} of the bound")


def test_stem_im2col_reference():
    for S in R.IM2COL_SIZES:
        inp = R.build_im2col(S)
        A = R.ref_im2col(inp)
        Ho = S // 2
        assert A.shape == (2 * Ho * Ho, 160) and bool((A[:, 147:] == 0).all())
        w = torch.randn(5, 3, 7, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        conv = F.conv2d(F.pad(inp["x"], (2, 3, 2, 3)), w, stride=2).permute(0, 2, 3, 1).reshape(-1, 5)       # TF 'SAME' of a 7 x 7 / 2 convolution at an even side
        assert float((A[:, :147] @ w.permute(0, 2, 3, 1).reshape(5, 147).t() - conv).abs().max()) < 1e-12
        assert not torch.equal(A, R.ref_im2col(inp, pad_left=True))
        assert bool((inp["x"] != 0).all())


def test_pool_builders_and_bound():
    zero_windows = 0
    for shape in R.POOL_SHAPES:
        B, Hi, C, cpg = shape
        inp = R.build_pool(shape)
        gap, zeros = R.pool_gaps(shape, inp)
        assert gap > R.POOL_GAP, (shape, gap)
        zero_windows += zeros
        ref, bound = R.ref_pool(shape, inp)
        assert ref.shape == (B, Hi // 2, Hi // 2, C) and float(bound.max()) < R.POOL_GAP / 100
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        if Hi > 2:
            _rejects(R.ref_pool(shape, inp, pad_left=True)[0].float(), ref, bound, "'SAME' padding in front")
        mean, rstd = (inp["stats"][..., k].float().repeat_interleave(cpg, 1)[:, None, None, :] for k in (0, 1))
        y32 = torch.relu((inp["raw"].float() - mean) * rstd * inp["gamma"].float() + inp["beta"].float())
        got = F.max_pool2d(F.pad(y32.permute(0, 3, 1, 2), (0, 1, 0, 1)), 3, 2).permute(0, 2, 3, 1)
        r = FR.check_bound(got, ref, bound, "torch f32")
        print(f"gn_relu_maxpool {shape}: torch f32 at {r:.3f} of the bound, smallest gap {gap:.2e}, {zeros} all-zero windows")
    assert zero_windows > 0


def test_vit_ln_bound():
    for case in R.VIT_CASES:
        B, g = case
        ntok = 1 + g * g
        inp = R.build_vit(case)
        xf = R.vit_tokens(inp, B, ntok)
        exact = torch.cat([inp["cls"].expand(B, 1, 768), inp["y"].reshape(B, ntok - 1, 768)], 1) + inp["pos"][None]
        assert float((xf.double() - exact.reshape(-1, 768)).abs().max()) < 1e-5 and not torch.equal(xf, R.vit_tokens(inp, B, ntok, off_by_one=True))
        ref, bound = R.ln_bound(xf.double(), inp["g"], inp["be"], R.VIT_EPS)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        _rejects(R.ln_bound(xf.double(), inp["g"], inp["be"], 1e-5)[0].float(), ref, bound, "eps 1e-5")
        _rejects(R.ln_bound(R.vit_tokens(inp, B, ntok, off_by_one=True).double(), inp["g"], inp["be"], R.VIT_EPS)[0].float(), ref, bound, "position row off by one")
        r = FR.check_bound(_ln32(xf, inp["g"], inp["be"], R.VIT_EPS), ref, bound, "torch f32")
        print(f"vit_tokens_ln {case}: torch f32 at {r:.3f} of the bound")
        assert (B * ntok) % 4
    for case in R.LN_ROWS_CASES:
        inp = R.build_ln_rows(case)
        ref, bound = R.ln_bound(inp["xf"], inp["g"], inp["be"], R.VIT_EPS)
        _rejects(R.ln_bound(inp["xf"], inp["g"], inp["be"], 1e-5)[0].float(), ref, bound, "eps 1e-5")
        FR.check_bound(_ln32(inp["xf"], inp["g"], inp["be"], R.VIT_EPS), ref, bound, "torch f32")


def test_pos_embed_bound():
    for case in R.POS_CASES:
        g0, g, C = case
        inp = R.build_pos(case)
        ref, bound = R.ref_pos(case, inp)
        assert ref.shape == (1 + g * g, C)
        FR.check_bound(ref.float(), ref, bound, "unmodified")
        tok = F.interpolate(inp["pos"][1:].float().reshape(1, g0, g0, C).permute(0, 3, 1, 2), size=(g, g), mode="bilinear", align_corners=False)
        got = torch.cat([inp["pos"][:1].float(), tok.permute(0, 2, 3, 1).reshape(g * g, C)])
        r = FR.check_bound(got, ref, bound, "torch f32")
        print(f"pos_embed_resize {case}: torch f32 at {r:.3f} of the bound")
        if g0 != g:
            _rejects(R.ref_pos(case, inp, align_corners=True)[0].float(), ref, bound, "align_corners=True")
        else:
            assert torch.equal(ref, inp["pos"])


def test_operand_checks_reject_faults():
    from soccdpt_amd.lib import x3_encode
    v = R.rnd((4, 32), 7, 3.0)
    bound = 1e-6 * v.abs()
    raw = x3_encode(v.float())
    R.check_x3_interval(raw, v.shape, v, bound, "x3 unmodified")
    hi, lo = R.x3_words(raw, v.shape)
    assert torch.equal(hi.view(torch.float16).double(), FR.x3_parts(raw, v.shape)[0])
    bad = raw.clone().reshape(-1, 2, 8)
    bad[0, 1] = 0                                        # the lo chunk of unit 0
    with pytest.raises(AssertionError):
        R.check_x3_interval(bad.reshape(-1), v.shape, v, bound, "x3 lo zeroed")
    assert R.check_op(v.float(), 2, v.shape, v, bound, "f32") <= 1.0
    with pytest.raises(AssertionError):
        R.check_op(v.to(torch.float16), 1, v.shape, None, None, "copy of another tensor", twin=(v * 1.01).float())


def test_refusals_need_no_gpu():
    """Every call tests/test_fwd_aux_gpu.py expects to be refused is refused by host code alone -- the entry's plan or the launcher's own checks, both in front
    of the launch -- with an error that names the entry.  (That nothing was written is the GPU test's part.)"""
    import ctypes
    from soccdpt_amd.lib import load_library
    from tests import test_fwd_aux_gpu as G
    L = load_library()
    base = 1 << 20                                              # placeholders: a refused call dereferences nothing
    before = int(L.soccdpt_launch_counter())
    n = 0
    for label, call, off in G.bad_calls():
        ins = [None if t is None else base + 65536 * i + off.get(f"in{i}", 0) for i, t in enumerate(call.ins)]
        outs = [None if t is None else base + 65536 * (8 + i) + off.get(f"out{i}", 0) for i, t in enumerate(call.outs)]
        path = ctypes.c_uint32(77)
        assert L.soccdpt_op_fwd_aux(ctypes.byref(G.make_args(call, ins, outs)), ctypes.byref(path), None) == 1, f"accepted: {label}"
        assert L.soccdpt_last_error(None).decode().startswith("soccdpt_op_fwd_aux: "), (label, L.soccdpt_last_error(None).decode())
        assert path.value == 77, label
        n += 1
    assert n >= 45 and int(L.soccdpt_launch_counter()) == before


def test_builders_hand_out_operand_values():
    """Every float64 tensor a builder returns is exactly representable in f32 -- the references must start from the values the kernel reads, not from
    their unrounded ancestors."""
    built = [R.build_patch("1x32x40"), R.build_ln("rowscale_c96"), R.build_bilinear(R.BILINEAR_SHAPES["nonint"], 12), R.build_bilinear(R.BILINEAR_SHAPES["x2"], 8, in_fmt=1),
             R.build_seg((1, 3, 6), 0), R.build_seg((1, 3, 6), 2), R.build_cvt(1000, 5), R.build_conv_w("3x5"), R.build_bn_fold(100), R.build_qkv_bias(100),
             R.build_logit_scale(100), R.build_cpb(R.CPB_CASES[0]), R.build_ws("stem"), R.build_im2col(16), R.build_pool(R.POOL_SHAPES[1]), R.build_vit(R.VIT_CASES[0]),
             R.build_ln_rows("7_shifted"), R.build_pos(R.POS_CASES[1])]
    for inp in built:
        for k, v in inp.items():
            assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), k
