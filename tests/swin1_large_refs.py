"""What the dpt_swin_large_384 tests share (tests/test_swin1_large_cpu.py, test_swin1_kernels_gpu.py, test_swin1_large_gpu.py).

* The CPU statement of the Swin-V1 encoder (timm 0.6.12 swin_large_patch4_window12_384: patch embed + norm, pre-norm blocks with roll / partition / mask,
  PatchMerging = gather, LayerNorm(4C), reduction) in torch, on top of oracle/soccdpt_ref.py's geometry helpers -- the oracle's file has no Swin-V1 block and is
  not edited.  encoder() is generic in its architecture row and dtype (the HF cross-check runs a small row in float64); network() adds the oracle's decoder
  and heads.
* Float64 references of the three kernels of csrc/swin1.hip, each with an a-priori per-element bound, in the manner of tests/attention_refs.py and
  tests/fwd_aux_refs.py; float32 emulations of the kernels and the seeded defects for the CPU self-test.  Nothing is fitted to a measured error.

The attention bound is attention_refs' scaled dot-product bound (stated there for the ViT kernel) at head dimension 32 plus the bias term: per query row
eps = max over keys of  sum_i Eq_i |k_i|  +  gamma(34) (sum_i |q'_i k_i| + |bias| + 100 [masked])  + the exponent terms, q' = q 32^-0.5.  Unlike 1 / 8 the scale
is no power of two: the kernels multiply q by fl32(32^-0.5) in f32 (two roundings, 2 u |q'_i|) and the 16-bit ones round the product to 16 bits again before the
matrix cores read it, Eq_i = |q'_i| (2 u + u16 (1 + 2 u)) + a (a = 2^-25 for fp16: the subnormal grid).  k and v are read as stored.

A defect of tests/attention_refs.py worked round here: _softmax_bound multiplies D by e^(2 eps) - 1, which overflows to inf (and inf x 0 = NaN) once eps
exceeds ~350 -- never with cosine logits (|s| <= 100 + 16), at once with dot-product logits of rows scaled by 2^10.  softmax_bound() below caps every term
by what holds for ANY weights: the output is a combination of the v_j with non-negative weights summing to one (up to the 16-bit rounding of the weights,
kept as its own term), so no logit error moves it further than max_j |v_jd - o_d|, and sum_j p'_j |v_jd| never exceeds max_j |v_jd|.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import soccdpt_ref as R
from tests import attention_refs as A
from tests.attention_refs import SUBNORMAL, U16, bias_index, quantize, window_masked, window_model, window_rows  # noqa: F401
from tests.fused_refs import U, gamma, round16  # noqa: F401
from tests.fwd_aux_refs import ln_bound

BACKBONE = "swinl12_384"
MODEL_TYPE = "dpt_swin_large_384"
ENCODER_PARAMS = 196_735_516          # by formula = timm's published 196.74 M for swin_large_patch4_window12_384 (norm and the 1000-class head included)
CONSUMED_ENCODER_PARAMS = 195_195_444  # without the dead final norm and head
PRE = "depth_net.pretrained.model."
QSCALE = 32.0 ** -0.5


class Arch:
    """The architecture row encoder() walks (spec.SwinV1Arch has the same fields)."""

    def __init__(self, img, patch, embed, depths, heads, window, hooks):
        self.img, self.patch, self.embed, self.depths, self.heads, self.window, self.hooks = img, patch, embed, tuple(depths), tuple(heads), window, tuple(hooks)


ARCH = Arch(384, 4, 192, (2, 2, 18, 2), (6, 12, 24, 48), 12, (1, 1, 17, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder, stated in torch
# ---------------------------------------------------------------------------------------------------------------------------------
def window_attention(sd, pfx, x, res, ws, shift, heads):
    """timm 0.6.12 WindowAttention.forward inside SwinTransformerBlock's roll / partition / reverse: x [B, L, C] (already normalised) -> [B, L, C] after proj."""
    B, L, C = x.shape
    d, nw, N = C // heads, res // ws, ws * ws
    h = x.reshape(B, res, res, C)
    if shift > 0:
        h = torch.roll(h, shifts=(-shift, -shift), dims=(1, 2))
    win = h.reshape(B, nw, ws, nw, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw, N, C)
    qkv = F.linear(win, sd[pfx + "qkv.weight"], sd[pfx + "qkv.bias"]).reshape(-1, N, 3, heads, d).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0] * d ** -0.5, qkv[1], qkv[2]
    attn = q @ k.transpose(-2, -1)
    bias = sd[pfx + "relative_position_bias_table"][R.relative_position_index(ws).reshape(-1)].reshape(N, N, heads).permute(2, 0, 1)
    attn = attn + bias.unsqueeze(0)
    mask = R.shift_attn_mask(res, ws, shift)
    if mask is not None:
        attn = (attn.reshape(B, nw * nw, heads, N, N) + mask.to(attn.dtype)[None, :, None]).reshape(-1, heads, N, N)
    out = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, N, C)
    out = F.linear(out, sd[pfx + "proj.weight"], sd[pfx + "proj.bias"])
    out = out.reshape(B, nw, nw, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, res, res, C)
    if shift > 0:
        out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out.reshape(B, L, C)


def swin1_block(sd, pfx, x, res, ws, shift, heads):
    """Pre-norm block: x + attn(LN1(x)); then + mlp(LN2(.))."""
    C = x.shape[-1]
    x = x + window_attention(sd, pfx + "attn.", F.layer_norm(x, (C,), sd[pfx + "norm1.weight"], sd[pfx + "norm1.bias"], 1e-5), res, ws, shift, heads)
    m = F.layer_norm(x, (C,), sd[pfx + "norm2.weight"], sd[pfx + "norm2.bias"], 1e-5)
    m = F.gelu(F.linear(m, sd[pfx + "mlp.fc1.weight"], sd[pfx + "mlp.fc1.bias"]))
    return x + F.linear(m, sd[pfx + "mlp.fc2.weight"], sd[pfx + "mlp.fc2.bias"])


def merge_gather(h):
    """[B, R, R, C] -> [B, (R/2)^2, 4C] in timm's order."""
    B, Rr, _, C = h.shape
    return torch.cat([h[:, 0::2, 0::2], h[:, 1::2, 0::2], h[:, 0::2, 1::2], h[:, 1::2, 1::2]], dim=-1).reshape(B, Rr * Rr // 4, 4 * C)


def patch_merging(sd, pfx, x, res):
    B, L, C = x.shape
    h = merge_gather(x.reshape(B, res, res, C))
    return F.linear(F.layer_norm(h, (4 * C,), sd[pfx + "norm.weight"], sd[pfx + "norm.bias"], 1e-5), sd[pfx + "reduction.weight"])


def encoder(sd, x, arch=ARCH, pfx=PRE, after_downsample=None):
    """forward_swin with hooks on layers[s].blocks[hooks[s]] -> the four hooked maps [B, C_s, res_s, res_s].  after_downsample: a list that receives each
    stage's output AFTER its PatchMerging (what HF's SwinModel reports as hidden states)."""
    B = x.shape[0]
    t = F.conv2d(x, sd[pfx + "patch_embed.proj.weight"], sd[pfx + "patch_embed.proj.bias"], stride=arch.patch).flatten(2).transpose(1, 2)
    t = F.layer_norm(t, (arch.embed,), sd[pfx + "patch_embed.norm.weight"], sd[pfx + "patch_embed.norm.bias"], 1e-5)
    res = arch.img // arch.patch
    outs = []
    for s, depth in enumerate(arch.depths):
        for j in range(depth):
            ws, shift = R.window_geometry(res, arch.window, j)
            t = swin1_block(sd, f"{pfx}layers.{s}.blocks.{j}.", t, res, ws, shift, arch.heads[s])
            if j == arch.hooks[s]:
                outs.append(t.transpose(1, 2).reshape(B, t.shape[-1], res, res))
        if s < len(arch.depths) - 1:
            t = patch_merging(sd, f"{pfx}layers.{s}.downsample.", t, res)
            res //= 2
        if after_downsample is not None:
            after_downsample.append(t)
    return outs


def network(sd, x, sigmoid=True):
    """(inv_depth [B,H,W], seg [B,C,H,W], path_1): encoder() + the oracle's decoder and heads (soccdpt_v3_network for this backbone)."""
    inv, p1 = R.dpt_decoder(sd, encoder(sd, x))
    return inv, R.seg_head(sd, p1, sigmoid), p1


# ---------------------------------------------------------------------------------------------------------------------------------
# scaled dot-product window attention: float64 reference + bound, emulation, defects
# ---------------------------------------------------------------------------------------------------------------------------------
ATTN_FORMATS = ("bf16", "f16", "f32", "f16_x3")          # operand format [+ the fp16 kernel's x3 store]; 'x3' = f32 qkv in, x3 out (the F16X3 mode)
ATTN_CASES = {"r24_shift": (1, 24, 12, 6, 2), "r24": (1, 24, 12, 0, 2), "r12_b2": (2, 12, 12, 0, 1)}      # B, res, ws, shift, heads
ATTN_DEFECTS = ("no_scale", "bias_transposed", "mask_dropped", "cosine")
Q_GAIN = (1.0, 6.0)          # per head, cycled: "head scale 1 and large" -- Swin-V1 has no learned scale, so the gain sits in the q rows themselves


def table_values(ws, heads, g):
    """relative_position_bias_table [(2 ws - 1)^2][heads] f32: most entries near 0 (trunc-normal 0.02 at initialisation), a tenth at +-16."""
    t = 0.02 * torch.randn((2 * ws - 1) ** 2, heads, generator=g, dtype=torch.float64)
    big = torch.rand(t.shape, generator=g) < 0.1
    sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0).double()
    return torch.where(big, 16.0 * sign, t).float().double()


def build_attention(case, fmt):
    """attention_refs.build_window's q, k, v (planted keys, rows scaled by 2^+-10, a zero q row and k row) with the per-head q gain, and the table above."""
    B, res, ws, shift, heads = ATTN_CASES[case]
    inp = A.build_window(B, res, ws, shift, heads, "f32")
    C = heads * 32
    qkv = inp["qkv"].reshape(-1, 3, heads, 32).clone()
    qkv[:, 0] *= torch.tensor([Q_GAIN[h % 2] for h in range(heads)], dtype=torch.float64).view(1, heads, 1)
    g = torch.Generator().manual_seed(77 + res + heads + shift)
    return {"qkv": quantize(qkv.reshape(-1, 3 * C), fmt), "table": table_values(ws, heads, g)}


def softmax_bound(s, eps_pair, v, model):
    """attention_refs._softmax_bound with every term capped by what holds for any weights (module docstring)."""
    m = s.amax(-1, keepdim=True)
    gap = m - s
    e = torch.exp(-gap)
    rowsum = e.sum(-1, keepdim=True)
    p = e / rowsum
    eps = (eps_pair + 2 * U * gap.clamp(max=1e4)).amax(-1, keepdim=True) + U * (A.EXP_ULPS + 5 * model.rescales)
    o = p @ v
    Aabs = p @ v.abs()
    D = A._mean_abs_dev(p, v, o) * (1 + 2.0 ** -12) + 2.0 ** -22 * (Aabs + o.abs())
    grow = torch.exp((2 * eps).clamp(max=600.0))
    vmax = v.abs().amax(-2, keepdim=True)                                       # [P][1][d]
    hull = (v[:, None, :, :] - o[:, :, None, :]).abs().amax(-2)                 # max_j |v_jd - o_d|, [P][N][d]
    u16 = U16[model.fmt]
    shift_term = torch.minimum((grow - 1) * D, hull)
    wsum = torch.minimum(grow * Aabs, vmax.expand_as(Aabs))                     # sum_j p'_j |v_jd|
    oabs = torch.minimum(grow * o.abs(), vmax.expand_as(o))
    bound = shift_term + (u16 + gamma(model.n_acc)) * wsum + (gamma(model.n_acc) + gamma(3)) * oabs
    if SUBNORMAL[model.fmt]:
        bound = bound + SUBNORMAL[model.fmt] * v.abs().sum(-2, keepdim=True) / rowsum
    return o, bound


def attention_ref(qkv, table, B, res, ws, shift, heads, fmt, defect=None):
    """qkv [B res res][3 C] float64 holding the operand values of fmt, table [(2 ws - 1)^2][heads] -> (out [B res res][C], bound); a defect -> (out, None)."""
    C, N, nw = heads * 32, ws * ws, res // ws
    model = window_model(fmt, ws)
    rows = window_rows(B, res, ws, shift)
    masked = None if defect == "mask_dropped" else window_masked(res, ws, shift)
    bidx = bias_index(ws, transposed=defect == "bias_transposed")
    out = torch.zeros(B * res * res, C, dtype=torch.float64)
    bound = None if defect else torch.zeros_like(out)
    for w in range(rows.shape[0]):
        x = qkv[rows[w]].reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        q, k, v = x[0], x[1], x[2]
        if defect == "cosine":
            q = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12)
            k = k / k.norm(dim=-1, keepdim=True).clamp(min=1e-12)
        qs = q if defect == "no_scale" else q * QSCALE
        bias = table[bidx].permute(2, 0, 1)
        s = qs @ k.transpose(-1, -2) + bias
        mag = qs.abs() @ k.abs().transpose(-1, -2) + bias.abs()
        if masked is not None:
            mk = masked[w % (nw * nw)][None].expand(heads, N, N)
            s = s - 100.0 * mk
            mag = mag + 100.0 * mk
        if defect:
            o = torch.softmax(s, -1) @ v
        else:
            Eq = qs.abs() * (2 * U + U16[fmt] * (1 + 2 * U)) + SUBNORMAL[fmt]
            o, bd = softmax_bound(s, Eq @ k.abs().transpose(-1, -2) + gamma(34) * mag, v, model)
            bound[rows[w]] = bd.permute(1, 0, 2).reshape(N, C)
        out[rows[w]] = o.permute(1, 0, 2).reshape(N, C)
    return out, bound


def emulate_attention(qkv, table, B, res, ws, shift, heads, fmt):
    """What the kernels compute, in float32 torch: q scaled in f32 (and rounded to the 16-bit format), logits, online-free softmax and P V in f32, the weights
    of the 16-bit kernels rounded to 16 bits for P V with the row sum taken from the unrounded ones.  -> the f32 accumulators [B res res][C]."""
    C, N, nw = heads * 32, ws * ws, res // ws
    rows = window_rows(B, res, ws, shift)
    masked = window_masked(res, ws, shift)
    bidx = bias_index(ws)
    out = torch.zeros(B * res * res, C, dtype=torch.float32)
    c32 = torch.tensor(QSCALE, dtype=torch.float32)
    for w in range(rows.shape[0]):
        x = qkv[rows[w]].float().reshape(N, 3, heads, 32).permute(1, 2, 0, 3)
        q = x[0] * c32
        if fmt != "f32":
            q = round16(q.double(), fmt).float()
        s = q @ x[1].transpose(-1, -2) + table.float()[bidx].permute(2, 0, 1)
        if masked is not None:
            s = s - 100.0 * masked[w % (nw * nw)][None].float()
        e = torch.exp(s - s.amax(-1, keepdim=True))
        l = e.sum(-1, keepdim=True)
        if fmt != "f32":
            e = round16(e.double(), fmt).float()
        out[rows[w]] = ((e @ x[2]) / l).permute(1, 0, 2).reshape(N, C)
    return out


_CACHE = {}


def attention_case(case, fmt):
    """(inputs, ref, bound) of an attention case in operand format fmt ('bf16' / 'f16' / 'f32'), computed once per process and left unchanged."""
    key = ("attn", case, fmt)
    if key not in _CACHE:
        inp = build_attention(case, fmt)
        ref, bound = attention_ref(inp["qkv"], inp["table"], *ATTN_CASES[case], fmt)
        _CACHE[key] = (inp, ref, bound)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# pre-norm LayerNorm rows and merge-LN: float64 reference + fwd_aux_refs' LayerNorm bound
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
LN_ROWS = 5                                  # no multiple of the 4 rows of a workgroup
LN_WIDTHS = (192, 384, 768, 1536)
MERGE_CASES = [(1, 4, 192), (2, 6, 384), (1, 2, 768)]      # B, R, C
OUT_FORMATS = ("bf16", "f16", "f32", "x3")


def build_ln(rows, C, seed):
    """xf with a row offset and spread per row (a mean far from 0 is what a one-pass variance would lose), gains around 1, small betas; f32 values."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g, dtype=torch.float64) * (0.5 + torch.arange(rows, dtype=torch.float64)[:, None]) + 3.0 * torch.arange(rows, dtype=torch.float64)[:, None]
    gain = 1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    return {"xf": x.float().double(), "g": gain.float().double(), "beta": beta.float().double()}


def prenorm_case(C):
    key = ("ln", C)
    if key not in _CACHE:
        inp = build_ln(LN_ROWS, C, 300 + C)
        _CACHE[key] = (inp,) + tuple(ln_bound(inp["xf"], inp["g"], inp["beta"], EPS))
    return _CACHE[key]


def build_merge(B, Rr, C):
    inp = build_ln(B * Rr * Rr, C, 500 + C + Rr)
    wide = build_ln(1, 4 * C, 600 + C)
    return {"xf": inp["xf"].reshape(B, Rr, Rr, C), "g": wide["g"], "beta": wide["beta"]}


def merge_ln_ref(inp, defect=None):
    """-> (operand rows [B (R/2)^2][4C], bound).  Defects: 'swapped' = blocks 1 and 2 of the gather exchanged (torch's natural (dy, dx) nesting), 'ln_over_c' = each
    of the four C-wide blocks normalised on its own."""
    h = inp["xf"]
    B, Rr, _, C = h.shape
    if defect == "swapped":
        rows = torch.cat([h[:, 0::2, 0::2], h[:, 0::2, 1::2], h[:, 1::2, 0::2], h[:, 1::2, 1::2]], dim=-1).reshape(-1, 4 * C)
    else:
        rows = merge_gather(h).reshape(-1, 4 * C)
    if defect == "ln_over_c":
        t = F.layer_norm(rows.reshape(-1, 4, C), (C,), None, None, EPS).reshape(-1, 4 * C) * inp["g"] + inp["beta"]
        return t, None
    t, bound = ln_bound(rows, inp["g"], inp["beta"], EPS)
    return t, (None if defect else bound)


def merge_case(B, Rr, C):
    key = ("merge", B, Rr, C)
    if key not in _CACHE:
        inp = build_merge(B, Rr, C)
        _CACHE[key] = (inp,) + tuple(merge_ln_ref(inp))
    return _CACHE[key]


def emulate_ln(rows, g, beta):
    """The kernels' arithmetic in float32: two-pass mean / variance, rsqrt, (v - mean) rstd g + beta."""
    v = rows.float()
    d = v - v.mean(-1, keepdim=True)
    rstd = torch.rsqrt((d * d).mean(-1, keepdim=True) + torch.tensor(EPS, dtype=torch.float32))
    return d * rstd * g.float() + beta.float()


def to_format(t32, fmt):
    """f32 results -> what the kernel stores in fmt, as float64 values ('x3': the decoded pair)."""
    if fmt == "f32":
        return t32.double()
    if fmt == "x3":
        return A.x3_value(t32.double())
    return round16(t32.double(), fmt)


def check_values(vals, fmt, ref, bound, what):
    """Decoded output values (float64) of format fmt against (ref, bound): an f32 output within the bound, a 16-bit one in the rounded interval, an x3 pair within
    bound + 2^-23 |ref| + 2^-36 (fwd_aux_refs.check_x3_interval's decode rule)."""
    from tests.fused_refs import check_bound
    from tests.fwd_aux_refs import check_interval16
    if fmt == "f32":
        return check_bound(vals, ref, bound, what)
    if fmt == "x3":
        return check_bound(vals, ref, bound + 2.0 ** -23 * ref.abs() + 2.0 ** -36, what)
    return check_interval16(vals, ref, bound, fmt, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# HF transformers' SwinModel: key map to timm's names (the cross-check of the statement above)
# ---------------------------------------------------------------------------------------------------------------------------------
def hf_to_timm(hf_sd, depths, pfx=PRE):
    """HF SwinModel state dict (transformers 5: attention.{q,k,v,o}_proj, layernorm_before / _after, mlp.fc1 / fc2) -> timm 0.6.12 names under pfx,
    q / k / v fused into qkv."""
    out = {}
    e = "embeddings.patch_embeddings.projection."
    out[pfx + "patch_embed.proj.weight"], out[pfx + "patch_embed.proj.bias"] = hf_sd[e + "weight"], hf_sd[e + "bias"]
    out[pfx + "patch_embed.norm.weight"], out[pfx + "patch_embed.norm.bias"] = hf_sd["embeddings.norm.weight"], hf_sd["embeddings.norm.bias"]
    for s, depth in enumerate(depths):
        for j in range(depth):
            h, t = f"encoder.layers.{s}.blocks.{j}.", f"{pfx}layers.{s}.blocks.{j}."
            for leaf in ("weight", "bias"):
                out[t + "norm1." + leaf] = hf_sd[h + "layernorm_before." + leaf]
                out[t + "norm2." + leaf] = hf_sd[h + "layernorm_after." + leaf]
                out[t + "attn.qkv." + leaf] = torch.cat([hf_sd[f"{h}attention.{n}_proj.{leaf}"] for n in "qkv"])
                out[t + "attn.proj." + leaf] = hf_sd[f"{h}attention.o_proj.{leaf}"]
                out[t + "mlp.fc1." + leaf] = hf_sd[h + "mlp.fc1." + leaf]
                out[t + "mlp.fc2." + leaf] = hf_sd[h + "mlp.fc2." + leaf]
            out[t + "attn.relative_position_bias_table"] = hf_sd[h + "attention.relative_position_bias.relative_position_bias_table"]
        if s < len(depths) - 1:
            h, t = f"encoder.layers.{s}.downsample.", f"{pfx}layers.{s}.downsample."
            out[t + "reduction.weight"] = hf_sd[h + "reduction.weight"]
            out[t + "norm.weight"], out[t + "norm.bias"] = hf_sd[h + "norm.weight"], hf_sd[h + "norm.bias"]
    return out
