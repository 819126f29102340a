"""What the dpt_large_384 tests share (tests/test_vit_large_cpu.py; the GPU tests of the model will import the same statement).

* The CPU fp32 statement of the encoder (timm vit_large_patch16_384 through forward_flex + the reference's act_postprocess1..4) in torch, on top of
  oracle/soccdpt_ref.py's vit_block / project_readout -- the oracle's file has no pure-ViT encoder and is not edited.  encoder() returns the four NCHW maps
  handed to scratch.layerN_rn, network() adds the oracle's decoder and heads.
* The seeded token tensors and index samples of tests/golden/vit_large_reassemble.npz (written by tests/tools/make_golden_vit_large.py from the
  reference's own modules): what pins the transposed-convolution weight layout and tap order to the reference.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from oracle import soccdpt_ref as R

BACKBONE = "vitl16_384"
MODEL_TYPE = "dpt_large_384"
ENCODER_PARAMS = 304_715_752          # timm's count for vit_large_patch16_384 (norm and the 1000-class head included)
E, DEPTH, HEADS, PATCH, GRID = 1024, 24, 16, 16, 24
HOOKS = (5, 11, 17, 23)               # model/dpt.py:88
FEATURES = (256, 512, 1024, 1024)     # model/blocks.py:96-102
PRE = "depth_net.pretrained."


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder, stated in torch
# ---------------------------------------------------------------------------------------------------------------------------------
def reassemble(sd, n: int, t: torch.Tensor, pfx: str = PRE) -> torch.Tensor:
    """act_postprocess<n> (backbones/utils.py:186-264) on hooked tokens t [B, 577, 1024] -> NCHW map."""
    ap = f"{pfx}act_postprocess{n}."
    B = t.shape[0]
    g = int(round((t.shape[1] - 1) ** 0.5))
    y = R.project_readout(sd, ap + "0.", t).transpose(1, 2).reshape(B, t.shape[2], g, g)
    y = F.conv2d(y, sd[ap + "3.weight"], sd[ap + "3.bias"])
    if n == 1:
        y = F.conv_transpose2d(y, sd[ap + "4.weight"], sd[ap + "4.bias"], stride=4)
    elif n == 2:
        y = F.conv_transpose2d(y, sd[ap + "4.weight"], sd[ap + "4.bias"], stride=2)
    elif n == 4:
        y = F.conv2d(y, sd[ap + "4.weight"], sd[ap + "4.bias"], stride=2, padding=1)
    return y


def encoder(sd, x: torch.Tensor, pfx: str = PRE):
    """forward_vit -> forward_adapted_unflatten(pretrained, x, "forward_flex") for vitl16_384: [B,256,96,96], [B,512,48,48], [B,1024,24,24], [B,1024,12,12].
    At 384 x 384 the resized position embedding is the stored one."""
    m = pfx + "model."
    B = x.shape[0]
    assert x.shape[2] == x.shape[3] == PATCH * GRID
    t = F.conv2d(x, sd[m + "patch_embed.proj.weight"], sd[m + "patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    t = torch.cat((sd[m + "cls_token"].expand(B, -1, -1), t), dim=1) + sd[m + "pos_embed"]      # cat first, then add
    outs = []
    for i in range(DEPTH):
        t = R.vit_block(sd, f"{m}blocks.{i}.", t, HEADS)
        if i in HOOKS:
            outs.append(reassemble(sd, HOOKS.index(i) + 1, t, pfx))
    return outs


def network(sd, x: torch.Tensor, sigmoid: bool = True):
    """(inv_depth [B,H,W], seg [B,C,H,W], path_1): encoder() + the oracle's decoder and heads (soccdpt_v3_network for this backbone)."""
    inv, p1 = R.dpt_decoder(sd, encoder(sd, x))
    return inv, R.seg_head(sd, p1, sigmoid), p1


# ---------------------------------------------------------------------------------------------------------------------------------
# the golden of the reference's own act_postprocess modules
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN_REASSEMBLE = "vit_large_reassemble.npz"
GOLDEN_ORDER = "param_order_vit_large.json"
GOLDEN_SAMPLE = 16384                 # values recorded per level


def golden_tokens(n: int) -> torch.Tensor:
    """The seeded hooked-token tensor [1, 577, 1024] f32 fed to act_postprocess<n>."""
    return torch.randn(1, GRID * GRID + 1, E, generator=torch.Generator().manual_seed(880 + n), dtype=torch.float32)


def golden_index(n: int, numel: int) -> torch.Tensor:
    """The seeded flat indices into act_postprocess<n>'s output that the golden records (the file stores them too)."""
    return torch.randint(0, numel, (GOLDEN_SAMPLE,), generator=torch.Generator().manual_seed(990 + n), dtype=torch.int64)


LAMBDA = 8.0


def gamma_p(n: float) -> float:
    """The probabilistic counterpart of fused_refs.gamma (Higham & Mary 2019, Theorem 2.4): a chain of n roundings, taken as independent and of mean zero,
    errs by at most lambda sqrt(n) u times the ROOT of the sum of squared magnitudes, except with probability 2 n exp(-lambda^2 / 2) -- 1e-10 per value at
    lambda = 8 and n = 9216.  The worst-case gamma(n) sum |.| carried through three layers of |W| allows 0.4 on values of 0.3 here: true, and no test."""
    return LAMBDA * n ** 0.5 * 2.0 ** -24


def reassemble_bound(sd, n: int, t: torch.Tensor, pfx: str = PRE):
    """act_postprocess<n> in float64 and a bound on what an f32 evaluation of it (the reference's modules, reassemble() above) differs from that by.
    Each stage is a sum of K products plus a bias, evaluated in f32 in some order: gamma_p(K + 2) sqrt(sum (w x)^2 + b^2), and the error e of its input
    reaches it as sqrt(sum w^2 e^2).  GELU: |gelu'| <= 1.13, and x (1 + erf(x / sqrt 2)) / 2 cancels for negative x: 2^-21 |x| covers its own rounding."""
    ap = f"{pfx}act_postprocess{n}."
    d = {k: v.double() for k, v in sd.items() if k.startswith(ap)}
    t = t.double()
    B, g = t.shape[0], int(round((t.shape[1] - 1) ** 0.5))
    feats = torch.cat((t[:, 1:], t[:, :1].expand_as(t[:, 1:])), -1)
    w1, b1 = d[ap + "0.project.0.weight"], d[ap + "0.project.0.bias"]
    a = F.linear(feats, w1, b1)
    e = gamma_p(w1.shape[1] + 2) * (F.linear(feats ** 2, w1 ** 2) + b1 ** 2).sqrt()
    h = F.gelu(a)
    e = 1.13 * e + 2.0 ** -21 * a.abs()
    nchw = lambda v: v.transpose(1, 2).reshape(B, v.shape[2], g, g)  # noqa: E731
    h, e = nchw(h), nchw(e)

    def stage(op, w, b, K, v, ev):
        sq = op(v ** 2, w ** 2) + (b ** 2)[None, :, None, None]
        return op(v, w) + b[None, :, None, None], op(ev ** 2, w ** 2).sqrt() + gamma_p(K + 2) * sq.sqrt()
    w3 = d[ap + "3.weight"]
    c, e = stage(F.conv2d, w3, d[ap + "3.bias"], w3.shape[1], h, e)
    if n == 3:
        return c, e
    w4, b4 = d[ap + "4.weight"], d[ap + "4.bias"]
    if n == 4:
        return stage(lambda v, w: F.conv2d(v, w, stride=2, padding=1), w4, b4, 9 * w4.shape[1], c, e)
    return stage(lambda v, w: F.conv_transpose2d(v, w, stride=w4.shape[2]), w4, b4, w4.shape[0], c, e)      # kernel = stride: one tap, a sum over ci


def reassemble_state(sd, pfx: str = PRE):
    """The act_postprocess entries of a state dict, keyed as `pretrained` registers them."""
    return {k[len(pfx):]: v for k, v in sd.items() if k.startswith(pfx + "act_postprocess")}
