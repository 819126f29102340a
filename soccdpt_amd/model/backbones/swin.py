"""Swin-V1 parameter tree with timm-0.6.12 names (what the reference creates through timm.create_model in
/root/reference/SOccDPT/model/backbones/swin.py and wraps in backbones/swin_common.py:_make_swin_backbone: `model`, then act_postprocess1..4 =
Transpose + Unflatten).  These modules only HOLD parameters and buffers so that state_dict() / load_state_dict() / parameters() behave like the
reference's; the arithmetic runs in libsoccdpt_hip.so (patch-embed, pre-norm LayerNorm, window-attention, igemm and merge-LN kernels)."""
import torch
import torch.nn as nn

from ..spec import SWIN1_ARCHS, SwinV1Arch


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: the Swin-V1 encoder runs inside libsoccdpt_hip.so")


def relative_position_index(ws: int) -> torch.Tensor:
    """timm WindowAttention's buffer [N, N]: (rq - rk + ws - 1) (2 ws - 1) + (cq - ck + ws - 1)."""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0) + (ws - 1)
    return rel[..., 0] * (2 * ws - 1) + rel[..., 1]


def shift_attn_mask(res: int, ws: int, shift: int) -> torch.Tensor:
    """timm SwinTransformerBlock's buffer [nW, N, N]: 0 / -100 between the regions of the rolled image."""
    img = torch.zeros(res, res)
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[h, w] = cnt
            cnt += 1
    win = img.view(res // ws, ws, res // ws, ws).permute(0, 2, 1, 3).reshape(-1, ws * ws)
    diff = win[:, None, :] - win[:, :, None]
    return torch.zeros_like(diff).masked_fill(diff != 0, -100.0)


class WindowAttentionParams(_Holder):
    def __init__(self, dim, heads, ws):
        super().__init__()
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) ** 2, heads))
        self.register_buffer("relative_position_index", relative_position_index(ws))
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)


class MlpParams(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)


class BlockParams(_Holder):
    def __init__(self, dim, heads, res, ws, shift):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttentionParams(dim, heads, ws)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MlpParams(dim)
        if shift:
            self.register_buffer("attn_mask", shift_attn_mask(res, ws, shift))


class PatchMergingParams(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)


class StageParams(_Holder):
    def __init__(self, arch: SwinV1Arch, s: int, downsample: bool):
        super().__init__()
        dim = arch.embed << s
        self.blocks = nn.ModuleList([BlockParams(dim, arch.heads[s], arch.stage_res(s), *arch.window_shift(s, j)) for j in range(arch.depths[s])])
        if downsample:
            self.downsample = PatchMergingParams(dim)


class PatchEmbedParams(_Holder):
    def __init__(self, arch: SwinV1Arch):
        super().__init__()
        self.proj = nn.Conv2d(3, arch.embed, kernel_size=arch.patch, stride=arch.patch)
        self.norm = nn.LayerNorm(arch.embed)


class SwinTransformerParams(_Holder):
    """Same registration order as timm 0.6.12 SwinTransformer: patch_embed, layers, norm, head."""

    def __init__(self, arch: SwinV1Arch):
        super().__init__()
        self.arch = arch
        self.patch_embed = PatchEmbedParams(arch)
        n = len(arch.depths)
        self.layers = nn.ModuleList([StageParams(arch, s, downsample=(s < n - 1)) for s in range(n)])
        self.norm = nn.LayerNorm(arch.embed << (n - 1))   # dead on the DPT path (hooks fire earlier)
        self.head = nn.Linear(arch.embed << (n - 1), 1000)  # dead on the DPT path


class Transpose(_Holder):
    def __init__(self, dim0, dim1):
        super().__init__()
        self.dim0, self.dim1 = dim0, dim1


class SwinBackbone(_Holder):
    """`pretrained` of the reference (backbones/swin_common.py): `.model` is the timm network, act_postprocess<n> turns the hooked tokens
    [B, L, C] into a map [B, C, res, res] (parameter-free: the library's activations are token-major already)."""

    def __init__(self, model: SwinTransformerParams, hooks):
        super().__init__()
        self.model = model
        self.hooks = list(hooks)
        arch = model.arch
        for s in range(4):
            r = arch.stage_res(s)
            setattr(self, f"act_postprocess{s + 1}", nn.Sequential(Transpose(1, 2), nn.Unflatten(2, torch.Size([r, r]))))


def _make_pretrained_swinl12_384(pretrained, hooks=None):
    assert not pretrained, "no network access: load weights through load_net / load_state_dict"
    arch = SWIN1_ARCHS["swinl12_384"]
    return SwinBackbone(SwinTransformerParams(arch), arch.hooks if hooks is None else hooks)
