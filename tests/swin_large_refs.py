"""What the dpt_swin2_large_384 tests share (tests/test_swin_large_cpu.py, test_swin_large_kernels_gpu.py, test_swin_large_gpu.py).

* The oracle's architecture entry: oracle/soccdpt_ref.py is generic in its ARCHS table and has no row for swinv2_large_window12to24_192to384_22kft1k; the
  row is inserted here, at import (a dict insert: the oracle's file is not edited).
* The kernel cases of the two launchers the model widened -- patch_embed at C0 = 192 (three channels per lane) and ln_residual at C = 1280 / 1536 (five / six
  float4 groups per lane) -- with their float64 references.  The bound models are tests/fwd_aux_refs.py's (derivations there): patch_embed's e_v = gamma(52)
  (sum |x w| + |bias|) into ln_bound -- the third channel of a lane runs the same two fma chains as the other two --, ln_residual's
  bound(t) |row_scale| + gamma(3) (|t row_scale| + |xres|).  Nothing is fitted to a measured error.
* The two existing-shape cases whose outputs are compared bit for bit with what the library gave BEFORE the launchers were widened (tests/golden/
  swin_large_parent_kernels.npz, written by tests/tools/make_golden_swin_large_kernels.py from a build of the parent commit).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import soccdpt_ref as R
from tests.fwd_aux_refs import Call, LnCase, f32, flags_of, gamma, ln_bound, ln_inputs, merge_layout, rnd  # noqa: F401  (merge_layout: the tests' twin of the merged copy)

BACKBONE = "swin2l24_384"
MODEL_TYPE = "dpt_swin2_large_384"
ENCODER_PARAMS = 196_739_932          # timm's count for swinv2_large_window12to24_192to384_22kft1k
R.ARCHS.setdefault(BACKBONE, R.SwinArch(384, 4, 192, (2, 2, 18, 2), (6, 12, 24, 48), 24, (12, 12, 12, 6), (1, 1, 17, 1)))

PATH_LN_V4 = 0x200

# ---------------------------------------------------------------------------------------------------------------------------------
# PATCH_EMBED at C0 = 192
# ---------------------------------------------------------------------------------------------------------------------------------
#                     B, S, C0, shifted       1x32: 64 tokens = 8 strips, one strip row per wave; 3x64: 768 tokens, more than one block
PATCH_CASES = {"1x32x192": (1, 32, 192, False), "3x64x192": (3, 64, 192, False), "1x32x192_shifted": (1, 32, 192, True)}
PATCH_RUNS = [(c, fmt) for c in ("1x32x192", "3x64x192") for fmt in (None, 0, 1, 3)] + [("1x32x192_shifted", 1)]
PATCH_LD = 192                        # row length of the prepared filter [48][192]


def build_patch(case, table=PATCH_CASES):
    """fwd_aux_refs.build_patch's inputs (same seeds) at the case's shape."""
    B, S, C0, shifted = table[case]
    x = rnd((B, 3, S, S), 11) + 0.2 * torch.arange(B, dtype=torch.float64)[:, None, None, None]
    w = rnd((C0, 48), 12, 1 / math.sqrt(48))
    bias = rnd((C0,), 13, 0.3) + (30.0 if shifted else 0.0)
    g, beta = 1.0 + 0.3 * rnd((C0,), 14), 0.2 * rnd((C0,), 15)
    return {"x": f32(x), "w": w, "bias": f32(bias), "g": f32(g), "beta": f32(beta)}


def ref_patch(inp, ld, eps=1e-5):
    C0 = inp["w"].shape[0]
    wk = inp["w"].view(C0, 3, 4, 4)
    v = F.conv2d(inp["x"], wk, inp["bias"], stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
    mag = F.conv2d(inp["x"].abs(), wk.abs(), inp["bias"].abs(), stride=4).permute(0, 2, 3, 1).reshape(-1, C0)
    wT = torch.zeros(48, ld, dtype=torch.float64)
    wT[:, :C0] = inp["w"].t()
    t, bound = ln_bound(v, inp["g"], inp["beta"], eps, gamma(52) * mag)
    return {"xf": (t, bound), "wT": wT}


def call_patch(case, fmt, inp, ld, table=PATCH_CASES):
    B, S, C0, _ = table[case]
    M = B * (S // 4) ** 2
    return Call("patch_embed", [B, S, C0], flags_of(0, fmt or 0), ins=[inp[k].float() for k in ("x", "w", "bias", "g", "beta")],
                outs=[("xf", (M, C0), 2), None if fmt is None else ("xb", (M, C0), fmt), ("wT", (48, ld), 2)])


# ---------------------------------------------------------------------------------------------------------------------------------
# LN_RESIDUAL at C = 1536 (V4 | 6) and 1280 (V4 | 5)
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln(M, C, **kw):
    return LnCase(M, C, path=PATH_LN_V4 | (C // 256), **kw)


LN_CASES = {
    "c1536_m1": _ln(1, 1536, fmt=1), "c1536_m5_nores": _ln(5, 1536, residual=0, fmt=0), "c1536_m23_x3": _ln(23, 1536, fmt=3),
    "c1536_m5_nores_x3": _ln(5, 1536, residual=0, fmt=3), "c1536_m23_f16": _ln(23, 1536, fmt=1), "c1536_shifted": _ln(5, 1536, shifted=True, fmt=1),
    "c1536_halo16": _ln(18, 1536, res=3, fmt=1, halo="op"), "c1536_x3halo_f16": _ln(18, 1536, res=3, fmt=1, halo="op", halo_fmt=3),
    "c1536_halof32": _ln(18, 1536, res=3, xb=False, halo="f32"), "c1536_rowscale": _ln(11, 1536, res=2, rps=4, fmt=1),
    # the merged operand layout: stage 3 has no PatchMerging behind it, so the forward never asks for it at this width; the row template gives it anyway
    "c1536_merge_r2": _ln(8, 1536, merge=1, res=2, fmt=1),
    "c1280_m7": _ln(7, 1280, fmt=1),
}


def build_ln(c: LnCase):
    y, g, b = ln_inputs(c.M, c.C, 21, c.shifted)
    inp = {"y": y, "g": g, "beta": b, "xf0": rnd((c.M, c.C), 25)}
    if c.rps:
        n = -(-c.M // c.rps)
        inp["row_scale"] = f32(torch.tensor([0.0, 1.0 / 0.9, 1.0 / 0.8, 1.25, 0.5][:n], dtype=torch.float64))
    return inp


def ref_ln(c: LnCase, inp, eps=1e-5):
    t, bt = ln_bound(inp["y"], inp["g"], inp["beta"], eps, None)
    rs = inp["row_scale"][torch.arange(c.M) // c.rps][:, None] if c.rps else torch.ones(c.M, 1, dtype=torch.float64)
    xres = inp["xf0"] if c.residual else torch.zeros_like(t)
    return t * rs + xres, bt * rs.abs() + gamma(3) * ((t * rs).abs() + xres.abs())


def call_ln(c: LnCase, inp):
    B = c.M // (c.res * c.res) if c.res and c.M % (c.res * c.res) == 0 else 0
    hshape = (B, c.res + 2, c.res + 2, c.C)
    hfmt = c.fmt if c.halo_fmt is None else c.halo_fmt
    outs = [("xf", (c.M, c.C), 2), ("xb", (c.M // 4, 4 * c.C) if c.merge else (c.M, c.C), c.fmt) if c.xb else None,
            ("halo", hshape, hfmt) if c.halo == "op" else None, ("halo_f32", hshape, 2) if c.halo == "f32" else None]
    return Call("ln_residual", [c.M, c.C, c.res, c.rps], flags_of(c.residual | (c.merge << 1), c.fmt, c.halo_fmt),
                ins=[inp["y"].float(), inp["g"].float(), inp["beta"].float(), inp["row_scale"].float() if c.rps else None], outs=outs,
                preset={"xf": inp["xf0"].float()} if c.residual else {}, halo=("halo", "halo_f32"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two existing-shape cases recorded from the parent commit's library
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN_FILE = "swin_large_parent_kernels.npz"
PARENT_PATCH = {"1x32x96": (1, 32, 96, False)}           # fwd_aux_refs.PATCH_CASES["1x32x96"], fp16 copy
PARENT_LN = LnCase(7, 1024, fmt=1, path=PATH_LN_V4 | 4)  # fwd_aux_refs.LN_CASES["c1024_m7"]


def parent_calls():
    """(label, Call) of the two recorded cases; the outputs are stored as <label>.<output name> (integer views of the bits)."""
    pi = build_patch("1x32x96", PARENT_PATCH)
    yield "patch_embed_1x32x96", call_patch("1x32x96", 1, pi, 128, PARENT_PATCH)
    yield "ln_residual_c1024_m7", call_ln(PARENT_LN, build_ln(PARENT_LN))


def bits(t: torch.Tensor) -> torch.Tensor:
    """A host tensor as integers of its element size (what the golden file stores and compares)."""
    t = t.contiguous().cpu()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])
