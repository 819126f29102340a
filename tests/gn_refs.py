"""Float64 reference, a-priori bounds, launcher rules and the case table of the reader side of the hybrid's GroupNorm (csrc/hybrid.hip: gn_apply_kernel<OUT, U>,
gn_finish_kernel, gn_sum_partials, gn_finish_groups, gn_finish_direct), shared by tests/test_gn_gpu.py (the kernels) and tests/test_gn_refs.py (this module
against itself, on the CPU).

Contract.  The kernel is handed f32 per-tile partials {sum, sum of squares} of every (sample, group) -- or finished f32 {mean, rstd} -- and the reference starts
from exactly those numbers, in float64, not from the raw tensor (f32 partials of large-mean data do not resolve the variance; that is the producer's matter,
tests/test_igemm_gen_gpu.py):

    a = sum of the tiles' sums, q = sum of their sums of squares, n = pixels per sample * channels per group
    mean = a / n,  var = max(q / n - mean^2, 0),  rstd = 1 / sqrt(var + eps)                  (eps: the f32 value the launcher is given)
    y = ((x - mean) rstd) gamma + beta   [+ the same of (raw2, part2, gamma2, beta2) | + res],  relu when asked.

Bound (fused_refs' vocabulary: U = 2^-24, gamma(k) = k U / (1 - k U); u64 = 2^-53 and gamma64 alike).  Nothing is fitted; |kernel - ref| <= bound for EVERY element.

Statistics {mean, rstd} as stored (stats_w / stats2_w; modes 1, 2 and the finish launch):
* the f64 sums of tps tiles, the product with inv_cnt = 1 / n (itself rounded) : a relative gamma64(tps + 4) of sum |a_t| resp. sum q_t -- taken twice, once for the
  kernel's order of summation and once for the reference's own:  g64 = 2 gamma64(tps + 4);
* mean:  e_mean = U |mean| (the f32 store) + g64 sum|a_t| / n;
* the cancellation in q / n - mean^2:  e_var = g64 (sum q_t / n + 2 |mean| sum|a_t| / n + mean^2) absolute; the clamp at 0 is 1-Lipschitz; it reaches rstd divided
  by 2 (var + eps):  rel_var = e_var / (2 (var + eps - e_var))  (at mean^2 / (var + eps) ~ 1e9 this is the size of U: it is not dropped);
* rsqrtf + one Newton step: the hardware estimate (of the f32-rounded argument) is within RSQ = 2^-22 relative; y1 = y0 (1.5 - 0.5 x y0^2) leaves
  1.5 RSQ^2 + 0.5 RSQ^3, and its six f64 operations gamma64(6);
* the f32 store of rstd: U.   rel_r = U + 1.5 RSQ^2 + 0.5 RSQ^3 + gamma64(6) + rel_var,   e_rstd = rstd rel_r.
Statistics handed in finished (mode 0 from stats) are inputs: e_mean = rel_r = 0.

Outputs.  With d = |x - mean| + e_mean:
* the statistics' errors reach y as  P = |gamma| rstd (e_mean + d rel_r)  -- this holds the mean-rounding term U |mean| rstd |gamma| on every element;
* the normalisation is four f32 roundings (a subtraction, two products, an addition; a contracted fma has fewer) of magnitudes
  Mg = d rstd (1 + rel_r) |gamma| + |beta|:  gamma(4) Mg;
* a shortcut adds its own P2 and Mg2 (projection) or Mg2 = |res| (identity: an input, P2 = 0), and the addition is a fifth rounding:
  bound = P + P2 + gamma(5) (Mg + Mg2);   no shortcut: bound = P + gamma(4) Mg.
* ReLU is 1-Lipschitz: no term.
* 16-bit and x3 stores: the rules fwd_aux_refs / fused_refs use for gn_relu_maxpool's four output modes (imported, not restated): beside an f32 output of the same
  launch a copy is RN16 of it / an x3 pair of it (check_copy16, check_x3_parts), the f32 format is the same bits; with no f32 twin a 16-bit value lies in
  [RN16(ref - bound), RN16(ref + bound)] and an x3 pair decodes within bound + 2^-23 |ref| + 2^-36 (check_interval16, check_x3_interval_parts).

Launcher rules (mode, pixels per thread, the finish launch's group width, the refusals) are restated below as Python next to the source lines they restate (SRC);
tests/test_gn_refs.py holds SRC against the text of csrc/hybrid.hip and csrc/capi.cpp.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from tests import fused_refs as FR
from tests import fwd_aux_refs as FA
from tests.fused_refs import U, gamma

U64 = 2.0 ** -53
RSQ = 2.0 ** -22
NEWTON = 1.5 * RSQ ** 2 + 0.5 * RSQ ** 3
EPS = float(torch.tensor(1e-5, dtype=torch.float32))
G = 32                                   # groups of every GroupNorm of the ResNetV2 (timm GroupNormAct(32))
MODES = {"bf16": 0, "f16": 1, "f32": 2, "x3": 3}                  # OUT of gn_apply_kernel
GUARD = 4096


def gamma64(k):
    return k * U64 / (1.0 - k * U64)


def prec_code(fmt):
    """OUT / halo_mode -> the SOCCDPT_PREC_* value soccdpt_op_gn_apply takes."""
    from soccdpt_amd.lib import PREC_BF16, PREC_F16, PREC_F16X3, PREC_F32
    return {0: PREC_BF16, 1: PREC_F16, 2: PREC_F32, 3: PREC_F16X3}[fmt]


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's rules, restated (csrc/hybrid.hip launch_gn_apply / launch_gn_finish, csrc/capi.cpp op_gn_apply_impl)
# ---------------------------------------------------------------------------------------------------------------------------------
SRC = {
    "thresholds": "constexpr int kGnDirectTps = 12, kGnCoopTps = 64;",
    "tmax": "const int tmax = a.part ? (a.raw2 && a.tps2 > a.tps ? a.tps2 : a.tps) : 0;",
    "mode": "d.mode = !a.part ? 0 : (tmax <= kGnDirectTps ? 1 : (tmax <= kGnCoopTps && 256 % G == 0 ? 2 : 0));",
    "finish launches": "if (a.part && d.mode == 0 && !skip_finish) {",
    "U = 4": "if (per_sample % 1024 == 0 && total / 1024 >= 1024) U = 4;",
    "U = 2": "else if (per_sample % 512 == 0 && total / 512 >= 1024) U = 2;",
    "gw": "while (gw > 1 && gw % 2 == 0 && 256 / gw < tps / 4) gw /= 2;",
    "geometry": "if (a.C % 4 || a.cpg < 2 || (a.cpg != 2 && a.cpg % 4) || a.C % a.cpg || a.HW <= 0 || a.M % (size_t)a.HW) { err = \"gn_apply: bad geometry\"; return 1; }",
    "one shortcut": "if (a.raw2 && a.res) { err = \"gn_apply: one shortcut kind at a time\"; return 1; }",
    "whole workgroups": "if (c4 > 256 || 256 % c4 || per_sample % 256 || G > 256) { err = \"gn_apply: C / 4 must divide 256 and a sample must be whole workgroups\"; return 1; }",
    "deferred": "if (a.part && (a.tps <= 0 || (a.raw2 && (!a.part2 || a.tps2 <= 0)) || !a.stats || (a.raw2 && !a.stats2))) { err = \"gn_apply: bad deferred-statistics arguments\"; return 1; }",
    "finish arguments": "if (!part || !stats || B <= 0 || tps <= 0 || G <= 0 || G > 256) { err = \"gn_finish: bad arguments\"; return 1; }",
    "finish gw": "if (256 % gw) { err = \"gn_finish: the group count must divide 256\"; return 1; }",
    "entry arguments": "if (!dev_raw || !dev_stats || !dev_gamma || !dev_beta || hw <= 0 || w <= 0 || hw % w) return fail(nullptr, std::string(who) + \": bad arguments\");",
    "entry projection": "if (dev_raw2 && (!dev_stats2 || !dev_gamma2 || !dev_beta2)) return fail(nullptr, std::string(who) + \": the projection shortcut needs stats2, gamma2 and beta2\");",
    "entry out_format": "if (om < 0) return fail(nullptr, std::string(who) + \": out_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3\");",
    "entry halo_format": "if (halo_format >= 0 && hm < 0) return fail(nullptr, std::string(who) + \": halo_format is SOCCDPT_PREC_BF16, _F16, _F32 or _F16X3\");",
}
K_DIRECT, K_COOP = 12, 64                                                          # SRC["thresholds"]


def stats_mode(tps, tps2, projection, groups=G):
    """(kernel mode, finish launches first) -- SRC["tmax"], SRC["mode"], SRC["finish launches"].  tps == 0: no partials, finished statistics are read."""
    if not tps:
        return 0, False
    tmax = tps2 if projection and tps2 > tps else tps
    mode = 1 if tmax <= K_DIRECT else (2 if tmax <= K_COOP and 256 % groups == 0 else 0)
    return mode, mode == 0


def pixels_per_thread(B, HW, C):
    """SRC["U = 4"], SRC["U = 2"]."""
    per_sample, total = HW * (C // 4), B * HW * (C // 4)
    if per_sample % 1024 == 0 and total // 1024 >= 1024:
        return 4
    if per_sample % 512 == 0 and total // 512 >= 1024:
        return 2
    return 1


def finish_gw(groups, tps):
    """(groups per workgroup of launch_gn_finish, its refusal or None) -- SRC["finish arguments"], SRC["gw"], SRC["finish gw"]."""
    if tps <= 0 or groups <= 0 or groups > 256:
        return 0, "gn_finish: bad arguments"
    gw = groups
    while gw > 1 and gw % 2 == 0 and 256 // gw < tps // 4:
        gw //= 2
    return gw, ("gn_finish: the group count must divide 256" if 256 % gw else None)


def apply_refusal(B, HW, W, C, cpg, tps=0, tps2=0, projection=False, identity=False, part=None, part2=True, stats2=True, affine2=True):
    """The message launch_gn_apply (or the entry in front of it) refuses these arguments with, or None -- in the launcher's order.  part: partials are handed in
    (default: whenever tps != 0).  With C / 4 and the channels per group both dividing powers of two, the group count always divides 256 here: the finish
    launch's own refusal is reachable through soccdpt_op_gn_finish only."""
    part = bool(tps) if part is None else part
    if HW <= 0 or W <= 0 or HW % W:
        return "soccdpt_op_gn_apply: bad arguments"
    if projection and not (stats2 and affine2):
        return "soccdpt_op_gn_apply: the projection shortcut needs stats2, gamma2 and beta2"
    if C % 4 or cpg < 2 or (cpg != 2 and cpg % 4) or C % cpg:
        return "gn_apply: bad geometry"
    if projection and identity:
        return "gn_apply: one shortcut kind at a time"
    c4, groups = C // 4, C // cpg
    if c4 > 256 or 256 % c4 or (HW * c4) % 256 or groups > 256:
        return "gn_apply: C / 4 must divide 256 and a sample must be whole workgroups"
    if part and (tps <= 0 or (projection and (not part2 or tps2 <= 0 or not stats2))):
        return "gn_apply: bad deferred-statistics arguments"
    if part and stats_mode(tps, tps2, projection, groups)[1]:
        for t in (tps, tps2) if projection else (tps,):
            if finish_gw(groups, t)[1]:
                return finish_gw(groups, t)[1]
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One soccdpt_op_gn_apply launch.  tps == 0: finished statistics are handed in; outs: which of out_f32 / out_op / out_halo are requested; fmt: out_format
    (OUT); halo_fmt: the halo image's own format (soccdpt_op_gn_apply_halo) or None; data: the data set (module docstring of tests/test_gn_gpu.py)."""
    name: str
    B: int
    H: int
    W: int
    C: int
    tps: int
    shortcut: str = "none"
    tps2: int = 0
    relu: int = 1
    fmt: int = 2
    halo_fmt: int | None = None
    outs: tuple = ("f32",)
    data: str = "a"

    @property
    def HW(self):
        return self.H * self.W

    @property
    def cpg(self):
        return self.C // G

    @property
    def n(self):
        return self.HW * self.cpg

    @property
    def mode(self):
        return stats_mode(self.tps, self.tps2, self.shortcut == "projection")

    @property
    def triple(self):
        """(OUT, U, statistics mode: '0s' from stats, '0f' after a finish launch, 1, 2)."""
        m, fin = self.mode
        return self.fmt, pixels_per_thread(self.B, self.HW, self.C), ("0f" if fin else ("0s" if not self.tps else m))


BF, HF, F3, X3 = MODES["bf16"], MODES["f16"], MODES["f32"], MODES["x3"]
_C = Case
CASES = [
    # every tile count of the thresholds, no shortcut / identity; B 1 and 3; cpg 2, 4, 8, 32; relu 0 and 1; the model's output combinations
    _C("t1_c64_b1", 1, 4, 4, 64, 1, fmt=HF, outs=("f32", "op")),
    _C("t9_c1024_b3_id", 3, 3, 3, 1024, 9, "identity", fmt=BF, outs=("f32", "op")),
    _C("t12_c64_b3_norelu_d", 3, 4, 4, 64, 12, relu=0, data="d"),
    _C("t13_c64_b3", 3, 4, 4, 64, 13, fmt=X3, outs=("f32", "op")),
    _C("t36_c128_b1_id_norelu_b", 1, 9, 8, 128, 36, "identity", relu=0, data="b"),
    _C("t64_c128_b3_halo", 3, 9, 8, 128, 64, fmt=HF, outs=("halo",)),
    _C("t65_c128_b3_op", 3, 9, 8, 128, 65, fmt=BF, outs=("op",)),
    _C("t144_c256_b3_id_all", 3, 37, 4, 256, 144, "identity", fmt=HF, outs=("f32", "op", "halo")),
    _C("t144_c64_b1_c", 1, 10, 16, 64, 144, data="c"),
    _C("t65_c64_b3_halo_x3", 3, 8, 10, 64, 65, fmt=X3, outs=("halo",)),
    _C("t9_c64_b3_c", 3, 4, 4, 64, 9, data="c"),
    _C("t13_c64_b3_c", 3, 4, 4, 64, 13, data="c"),
    _C("t12_c64_b3_b", 3, 4, 4, 64, 12, data="b"),
    _C("t36_c1024_b1_id_b", 1, 6, 6, 1024, 36, "identity", data="b"),
    _C("t36_c64_b3_d", 3, 6, 8, 64, 36, data="d", fmt=F3, outs=("op", "halo")),
    _C("t9_c256_b3_op_halo_bf16", 3, 2, 6, 256, 9, fmt=BF, outs=("op", "halo")),
    _C("t1_c1024_b3_id_op_x3", 3, 2, 2, 1024, 1, "identity", fmt=X3, outs=("op",)),
    # the projection shortcut: one mode for both tensors from the larger tile count
    _C("p9_36_c64_b3", 3, 6, 8, 64, 9, "projection", 36),
    _C("p36_9_c128_b1_norelu", 1, 9, 8, 128, 36, "projection", 9, relu=0),
    _C("p12_13_c1024_b3", 3, 4, 4, 1024, 12, "projection", 13, fmt=HF, outs=("f32", "op")),
    _C("p64_65_c64_b3", 3, 8, 10, 64, 64, "projection", 65),
    _C("p65_64_c256_b1_d", 1, 17, 4, 256, 65, "projection", 64, data="d"),
    _C("p144_144_c64_b3_b", 3, 10, 16, 64, 144, "projection", 144, data="b"),
    _C("p12_9_c64_b3", 3, 4, 4, 64, 12, "projection", 9, fmt=BF, outs=("f32", "op", "halo")),
    _C("p9_12_c128_b3_c", 3, 2, 8, 128, 9, "projection", 12, data="c"),
    # finished statistics handed in (the training step's form)
    _C("s_c64_b3", 3, 4, 4, 64, 0),
    _C("s_c512_b1_proj", 1, 1, 2, 512, 0, "projection", fmt=HF, outs=("f32", "op")),
    _C("s_c1024_b3_id_norelu", 3, 2, 2, 1024, 0, "identity", relu=0, fmt=X3, outs=("f32", "op", "halo")),
    # the halo image in a format of its own (SOCCDPT_PREC_MIXED: a hooked stage output feeds the decoder's group)
    _C("h_f16_x3_t9", 3, 4, 4, 64, 9, "identity", fmt=HF, halo_fmt=X3, outs=("f32", "op", "halo")),
    _C("h_f16_bf16_t13", 3, 4, 4, 64, 13, fmt=HF, halo_fmt=BF, outs=("f32", "op", "halo")),
    _C("h_f16_f32_t65", 3, 8, 10, 64, 65, "projection", 64, fmt=HF, halo_fmt=F3, outs=("op", "halo")),
    _C("h_bf16_f16_s", 1, 4, 4, 128, 0, fmt=BF, halo_fmt=HF, outs=("f32", "op", "halo")),
    # U = 4 (B = 2) and U = 2 (B = 1) of every format: the only large cases
    _C("u4_bf16_t9", 2, 48, 48, 1024, 9, "identity", fmt=BF, outs=("f32", "op")),
    _C("u4_f16_t36", 2, 48, 48, 1024, 36, fmt=HF, outs=("op",)),
    _C("u4_f32_t144", 2, 48, 48, 1024, 144, fmt=F3, outs=("op",)),
    _C("u4_x3_s", 2, 48, 48, 1024, 0, fmt=X3, outs=("op",)),
    _C("u2_bf16_t144", 1, 48, 48, 1024, 144, fmt=BF, outs=("op",)),
    _C("u2_f16_s", 1, 48, 48, 1024, 0, "identity", fmt=HF, outs=("f32", "op")),
    _C("u2_f32_t9", 1, 48, 48, 1024, 9, fmt=F3, outs=("f32", "op")),
    _C("u2_x3_t36", 1, 48, 48, 1024, 36, fmt=X3, outs=("f32", "op")),
]
CASE = {c.name: c for c in CASES}
LARGE = 300_000                          # elements: only the u4_* / u2_* cases are above it

FINISH_TPS = (1, 3, 31, 32, 33, 255, 576, 577)
FINISH_G = (8, 32, 64, 256)
FINISH_REFUSED = {96: "gn_finish: the group count must divide 256", 24: "gn_finish: the group count must divide 256", 512: "gn_finish: bad arguments"}   # at tps = 64


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_sizes(HW, tps, gen):
    """An uneven partition of a sample's HW pixel rows into tps tiles (every tile at least one row)."""
    assert 1 <= tps <= HW
    extra = torch.randint(0, tps, (HW - tps,), generator=gen)
    return torch.bincount(extra, minlength=tps) + 1


def partials(raw, B, HW, C, sizes):
    """[B * tps][G][2] = {sum, sum of squares} of every tile and group in float64, rounded to f32 as the producing convolution leaves them."""
    cpg = C // G
    x = raw.double().reshape(B, HW, G, cpg)
    edges = torch.cat([torch.zeros(1, dtype=torch.long), sizes.cumsum(0)])
    cs = torch.cat([torch.zeros(B, 1, G, dtype=torch.float64), x.sum(3).cumsum(1)], 1)
    cq = torch.cat([torch.zeros(B, 1, G, dtype=torch.float64), (x * x).sum(3).cumsum(1)], 1)
    a, q = cs[:, edges[1:]] - cs[:, edges[:-1]], cq[:, edges[1:]] - cq[:, edges[:-1]]
    if HW * C * B < LARGE:               # small: tile by tile, no difference of running sums
        a = torch.stack([x[:, edges[t]:edges[t + 1]].sum((1, 3)) for t in range(len(sizes))], 1)
        q = torch.stack([(x[:, edges[t]:edges[t + 1]] ** 2).sum((1, 3)) for t in range(len(sizes))], 1)
    return torch.stack((a, q), -1).reshape(B * len(sizes), G, 2).float()


def _levels(B, C, data, which, gen):
    """Per (sample, channel) offset and scale of the raw tensor.  (a): neighbouring groups and samples differ by >= 10x in mean and >= 4x in spread."""
    cpg = C // G
    g = torch.arange(G)[None, :]
    b = torch.arange(B)[:, None]
    if data == "b":                      # the stem's un-normalised levels: mean over spread 30 and 700
        mean = torch.where((g + b + which) % 2 == 0, 30.0, 700.0) + 0.25 * b
        spread = torch.ones(B, G)
    else:
        k = (g + b + 2 * which) % 4
        sign = torch.where((g + which) % 3 == 0, -1.0, 1.0)
        mean = sign * 0.02 * 10.0 ** k
        spread = 0.05 * 4.0 ** ((k + 1) % 4)
    return mean.double().repeat_interleave(cpg, 1), spread.double().repeat_interleave(cpg, 1)


def _tensor(c, which, gen):
    """raw [B][HW][C] f32 and its partials (tps tiles) of the main tensor (which = 0) or the projection shortcut's (1)."""
    tps = c.tps if which == 0 else c.tps2
    mean, spread = _levels(c.B, c.C, c.data, which, gen)
    cpg = c.cpg
    z = torch.randn((c.B, c.HW, G, cpg), generator=gen, dtype=torch.float32).double()
    z = (z - z.mean((1, 3), keepdim=True)) / z.std((1, 3), unbiased=False, keepdim=True)   # the levels are the groups' own mean and spread, at 32 values a group too
    raw = (mean[:, None, :] + spread[:, None, :] * z.reshape(c.B, c.HW, c.C)).float()
    if c.data == "c":
        raw[:, :, :cpg] = 3.0                                                            # group 0: constant, var = 0 exactly
        raw[:, :, cpg:2 * cpg] = (3.0 + 0.01 * torch.randn((c.B, c.HW, cpg), generator=gen)).float()
    if not tps:
        return raw, None, None
    sizes = tile_sizes(c.HW, tps, gen)
    part = partials(raw, c.B, c.HW, c.C, sizes)
    if c.data == "c":                    # group 1: hand-made partials, q / n one f32 ulp below mean^2 -- the clamp decides
        nt = (sizes * cpg).float().repeat(c.B)
        part[:, 1, 0] = 3.0 * nt
        part[:, 1, 1] = torch.nextafter(9.0 * nt, torch.zeros(()))
    return raw, part, sizes


@functools.lru_cache(maxsize=3)
def build(name):
    """Host inputs of a case (f32 tensors holding what the kernel reads)."""
    c = CASE[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 7 + 1)
    inp = {}
    inp["raw"], inp["part"], inp["sizes"] = _tensor(c, 0, gen)
    inp["gamma"], inp["beta"] = torch.rand((c.C,), generator=gen) + 0.5, torch.randn((c.C,), generator=gen) * 0.3
    if c.data == "d":
        inp["gamma"][1::5] = 0.0
        inp["gamma"][2::5] *= -1.0
        inp["beta"][::3] = -0.0          # -0: the sum keeps the sign of a -0 product (gamma < 0), +0 would hide it
    if c.shortcut == "projection":
        inp["raw2"], inp["part2"], inp["sizes2"] = _tensor(c, 1, gen)
        inp["gamma2"], inp["beta2"] = torch.rand((c.C,), generator=gen) + 0.5, torch.randn((c.C,), generator=gen) * 0.3
    elif c.shortcut == "identity":
        inp["res"] = torch.randn((c.B, c.HW, c.C), generator=gen)
    if not c.tps:                        # finished statistics: f32 {mean, rstd} of the raw tensor
        for k, r in (("stats", "raw"), ("stats2", "raw2")):
            if r in inp:
                x = inp[r].double().reshape(c.B, c.HW, G, c.cpg)
                inp[k] = torch.stack((x.mean((1, 3)), 1.0 / torch.sqrt(x.var((1, 3), unbiased=False) + EPS)), -1).float()
    if c.data == "d":                    # raw values at the f32 mean itself and one ulp either side, in channels with beta = 0: the pre-ReLU value is +-0 / tiny
        st = stats_ref(inp["part"], c.B, c.tps, c.n) if c.tps else given_stats(inp["stats"])
        mhat = st["mean"].float().repeat_interleave(c.cpg, 1)                             # [B][C]
        ch = torch.arange(0, c.C, 3)
        inp["raw"][:, 0, ch] = mhat[:, ch]
        inp["raw"][:, 1, ch] = torch.nextafter(mhat[:, ch], torch.full((), float("inf")))
        inp["raw"][:, 2, ch] = torch.nextafter(mhat[:, ch], torch.full((), float("-inf")))
    return inp


def build_finish(tps, groups, B=2, seed=0):
    """Hand-made partials [B * tps][groups][2] for gn_finish alone: uneven tiles of hw = 4 tps + 3 pixels, cpg = 2, levels that differ per sample and group."""
    gen = torch.Generator().manual_seed(seed + tps * 1000 + groups)
    hw, cpg = 4 * tps + 3, 2
    nt = (tile_sizes(hw, tps, gen) * cpg).double()[None, :, None]
    g, b = torch.arange(groups)[None, None, :], torch.arange(B)[:, None, None]
    mu = torch.where(g % 3 == 0, -1.0, 1.0) * 0.02 * 10.0 ** ((g + b) % 4)
    sg = 0.05 * 4.0 ** ((g + b + 1) % 4)
    a = nt * mu + sg * nt.sqrt() * torch.randn((B, tps, groups), generator=gen, dtype=torch.float64)
    q = a * a / nt + nt * sg * sg * (0.5 + torch.rand((B, tps, groups), generator=gen, dtype=torch.float64))
    return torch.stack((a, q), -1).reshape(B * tps, groups, 2).float(), hw, cpg


# ---------------------------------------------------------------------------------------------------------------------------------
# reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------
def stats_ref(part, B, tps, n, eps=EPS):
    """part [B * tps][groups][2] f32 -> float64 {mean, rstd} [B][groups] and their bounds e_mean (absolute), rel_r (relative); module docstring."""
    p = part.double().reshape(B, tps, -1, 2)
    a, q, sa, sq = p[..., 0].sum(1), p[..., 1].sum(1), p[..., 0].abs().sum(1), p[..., 1].abs().sum(1)
    mean = a / n
    var = (q / n - mean * mean).clamp(min=0.0)
    x = var + eps
    g64 = 2.0 * gamma64(tps + 4)
    e_var = g64 * (sq / n + 2.0 * mean.abs() * sa / n + mean * mean)
    assert bool((e_var < x / 4).all()), "the float64 cancellation reaches var + eps itself: no first-order bound"
    rel_r = U + NEWTON + gamma64(6) + e_var / (2.0 * (x - e_var))
    return {"mean": mean, "rstd": 1.0 / torch.sqrt(x), "e_mean": U * mean.abs() + g64 * sa / n, "rel_r": rel_r}


def given_stats(stats):
    s = stats.double()
    z = torch.zeros_like(s[..., 0])
    return {"mean": s[..., 0], "rstd": s[..., 1], "e_mean": z, "rel_r": z}


def _norm_ref(x, st, gam, bet, cpg):
    """x [B][HW][C] -> ((x - mean) rstd) gamma + beta in float64, P and Mg of the module docstring."""
    m, r, em, rr = (st[k].repeat_interleave(cpg, 1)[:, None, :] for k in ("mean", "rstd", "e_mean", "rel_r"))
    x, gam, bet = x.double(), gam.double(), bet.double()
    d = (x - m).abs() + em
    y = (x - m) * r * gam + bet
    return y, gam.abs() * r * (em + d * rr), d * r * (1.0 + rr) * gam.abs() + bet.abs()


def reference(c, inp):
    """-> dict(y [B][HW][C] float64, bound, st, st2): what the launch must write, from the partials (or finished statistics) as handed."""
    st = stats_ref(inp["part"], c.B, c.tps, c.n) if c.tps else given_stats(inp["stats"])
    y, P, Mg = _norm_ref(inp["raw"], st, inp["gamma"], inp["beta"], c.cpg)
    st2 = None
    if c.shortcut == "projection":
        st2 = stats_ref(inp["part2"], c.B, c.tps2, c.n) if c.tps else given_stats(inp["stats2"])
        y2, P2, Mg2 = _norm_ref(inp["raw2"], st2, inp["gamma2"], inp["beta2"], c.cpg)
        y, bound = y + y2, P + P2 + gamma(5) * (Mg + Mg2)
    elif c.shortcut == "identity":
        res = inp["res"].double()
        y, bound = y + res, P + gamma(5) * (Mg + res.abs())
    else:
        bound = P + gamma(4) * Mg
    return {"y": y.clamp(min=0.0) if c.relu else y, "bound": bound, "st": st, "st2": st2}


# ---------------------------------------------------------------------------------------------------------------------------------
# buffers and checks
# ---------------------------------------------------------------------------------------------------------------------------------
def buf_spec(c, which):
    """(dtype, shape) of an output buffer as the tests view it: x3 tensors as fp16 with 2 C words per pixel (half16.h: a pixel's C elements are 4 C bytes)."""
    fmt = 2 if which == "f32" else (c.halo_fmt if which == "halo" and c.halo_fmt is not None else c.fmt)
    dt, k = FA.op_dtype(fmt)
    lead = (c.B, c.H + 2, c.W + 2) if which == "halo" else (c.B * c.HW,)
    return dt, lead + (c.C * k,), fmt


def _check_vals(fmt, got, shape, sel, ref, bound, twin, what):
    """One operand output (got: the whole buffer, sel: the slice of `shape` that holds the values) by the store rules of fwd_aux_refs / fused_refs."""
    if fmt == 3:
        hi, lo = FR.x3_parts(got.reshape(-1), shape)
        hi, lo = hi[sel].reshape(ref.shape), lo[sel].reshape(ref.shape)
        return FR.check_x3_parts(hi, lo, twin, what) if twin is not None else FA.check_x3_interval_parts(hi, lo, ref, bound, what)
    v = got.reshape(shape)[sel].reshape(ref.shape)
    if fmt == 2:
        if twin is not None:
            assert torch.equal(v.view(torch.int32), twin.view(torch.int32)), f"{what}: the two f32 outputs of one launch differ"
            return 0.0
        return FR.check_bound(v, ref, bound, what)
    if twin is not None:
        FR.check_copy16(v, twin, FA.FMT16[fmt], what)
        return 0.0
    return FA.check_interval16(v, ref, bound, FA.FMT16[fmt], what)


def check_stats(got, st, what):
    """Stored {mean, rstd} [B][groups][2] against stats_ref's values and bounds; -> worst error / bound."""
    g = got.double().cpu()
    tiny = 2.0 ** -149
    return max(FR.check_bound(g[..., 0], st["mean"], st["e_mean"] + tiny, what + " mean"),
               FR.check_bound(g[..., 1], st["rstd"], st["rstd"] * st["rel_r"], what + " rstd"))


def check_outputs(c, ref, got):
    """got: host tensors 'f32' / 'op' / 'halo' (buf_spec views, halo ring pre-filled with 0xFF bytes) and 'stats' / 'stats2' where the launch writes them.
    -> {what: worst error / bound}."""
    y, bound = ref["y"].reshape(c.B * c.HW, c.C), ref["bound"].reshape(c.B * c.HW, c.C)
    ratios = {}
    twin = None
    if "f32" in c.outs:
        twin = got["f32"].cpu().reshape(c.B * c.HW, c.C)
        ratios["out_f32"] = FR.check_bound(twin, y, bound, c.name + " out_f32")
    if "op" in c.outs:
        ratios["out_op"] = _check_vals(c.fmt, got["op"].cpu(), (c.B * c.HW, c.C), slice(None), y, bound, twin, c.name + " out_op")
    if "halo" in c.outs:
        h = got["halo"].cpu()
        _, shape, fmt = buf_spec(c, "halo")
        inner = (slice(None), slice(1, -1), slice(1, -1))
        ratios["out_halo"] = _check_vals(fmt, h, (c.B, c.H + 2, c.W + 2, c.C), inner, y, bound, twin, c.name + " out_halo")
        ring = h.reshape(shape).view(torch.uint8).clone()
        ring[inner] = 0xFF
        assert bool((ring == 0xFF).all()), f"{c.name}: the halo ring was written"
    if c.tps:
        ratios["stats"] = check_stats(got["stats"], ref["st"], c.name + " stats")
        if c.shortcut == "projection":
            ratios["stats2"] = check_stats(got["stats2"], ref["st2"], c.name + " stats2")
    return ratios


# ---------------------------------------------------------------------------------------------------------------------------------
# an f32 emulation of the kernels (the partial sums in f64, the rest in f32, the store formats), with planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("s0_s1_swapped", "sample0_statistics", "last_tile_dropped", "clamped_tile_twice", "clamp_omitted", "unbiased_variance", "eps_dropped",
          "gamma2_beta2_replaced", "part2_walked_with_tps", "halo_off_by_one_pixel", "relu_skipped", "store16_truncated")


def fault_applies(f, c):
    if f == "s0_s1_swapped":
        return c.cpg == 2
    if f == "sample0_statistics":
        return c.B > 1
    if f in ("last_tile_dropped", "unbiased_variance", "eps_dropped"):
        return c.tps > 0
    if f == "clamped_tile_twice":
        return c.tps in (13, 65) or (c.shortcut == "projection" and c.tps2 in (13, 65))
    if f == "clamp_omitted":
        return c.tps > 0 and c.data == "c"
    if f == "gamma2_beta2_replaced":
        return c.shortcut == "projection"
    if f == "part2_walked_with_tps":
        return c.shortcut == "projection" and c.tps > 0 and c.tps != c.tps2
    if f == "halo_off_by_one_pixel":
        return "halo" in c.outs
    if f == "relu_skipped":
        return c.relu == 1
    if f == "store16_truncated":
        return ("op" in c.outs and c.fmt in (0, 1)) or ("halo" in c.outs and buf_spec(c, "halo")[2] in (0, 1))
    raise KeyError(f)


def emulate_stats(part, B, tps, n, eps=EPS, fault=None, walk_tps=None):
    """gn_sum_partials + gn_mean_rstd: [B][groups][2] f32."""
    groups = part.shape[1]
    p = part.double()
    if walk_tps is not None:             # planted: sample b's tiles start at b * walk_tps and there are walk_tps of them
        idx = (torch.arange(B)[:, None] * walk_tps + torch.arange(walk_tps)[None, :]).clamp(max=p.shape[0] - 1)
        p = p[idx]
    else:
        p = p.reshape(B, tps, groups, 2)
    if fault == "last_tile_dropped":
        p = p[:, :-1]
    if fault == "clamped_tile_twice":
        p = torch.cat([p, p[:, -1:]], 1)
    a, q = p[..., 0].sum(1), p[..., 1].sum(1)
    inv = 1.0 / float(n)
    mean = a * inv
    var = q * inv - mean * mean
    if fault == "unbiased_variance":
        var = var * (n / (n - 1.0))
    if fault != "clamp_omitted":
        var = var.clamp(min=0.0)
    x = var + (0.0 if fault == "eps_dropped" else eps)
    y0 = torch.rsqrt(x.float()).double()
    y1 = y0 * (1.5 - 0.5 * x * y0 * y0)
    return torch.stack((mean.float(), y1.float()), -1)


def _store(y, fmt, fault):
    """y [...][C] f32 -> the operand words of buf_spec ([...][C k])."""
    from soccdpt_amd.lib import x3_encode
    if fmt == 2:
        return y
    if fmt == 3:
        return x3_encode(y).reshape(*y.shape[:-1], y.shape[-1] * 2)
    dt = FA.op_dtype(fmt)[0]
    h = y.clamp(-65504.0, 65504.0).to(dt) if fmt == 1 else y.to(dt)
    if fault == "store16_truncated":
        over = h.float().abs() > y.abs()
        h = torch.where(over, (h.view(torch.int16) - 1).view(dt), h)      # one 16-bit step towards zero
    return h


def emulate(c, inp, fault=None):
    """The launch of case c on the host: -> the `got` dict check_outputs takes."""
    def stats_of(part, tps, given, walk=None):
        s = emulate_stats(part, c.B, tps, c.n, fault=fault, walk_tps=walk) if c.tps else given.clone()
        if fault == "sample0_statistics":
            s = s[:1].expand_as(s).clone()
        return s

    def norm(x, s, gam, bet):
        if fault == "s0_s1_swapped":
            s = s.reshape(c.B, G // 2, 2, 2).flip(2).reshape(c.B, G, 2)
        m, r = (s[..., k].repeat_interleave(c.cpg, 1)[:, None, :] for k in (0, 1))
        return (x - m) * r * gam + bet

    got = {}
    s = stats_of(inp["part"], c.tps, inp.get("stats"))
    y = norm(inp["raw"], s, inp["gamma"], inp["beta"])
    if c.tps:
        got["stats"] = s
    if c.shortcut == "projection":
        s2 = stats_of(inp["part2"], c.tps2, inp.get("stats2"), walk=c.tps if fault == "part2_walked_with_tps" else None)
        g2, b2 = (inp["gamma"], inp["beta"]) if fault == "gamma2_beta2_replaced" else (inp["gamma2"], inp["beta2"])
        y = y + norm(inp["raw2"], s2, g2, b2)
        if c.tps:
            got["stats2"] = s2
    elif c.shortcut == "identity":
        y = y + inp["res"]
    if c.relu and fault != "relu_skipped":
        y = torch.maximum(y, torch.zeros(()))
    if "f32" in c.outs:
        got["f32"] = y.reshape(c.B * c.HW, c.C).clone()
    if "op" in c.outs:
        got["op"] = _store(y.reshape(c.B * c.HW, c.C), c.fmt, fault)
    if "halo" in c.outs:
        dt, shape, fmt = buf_spec(c, "halo")
        nbytes = math.prod(shape) * torch.empty((), dtype=dt).element_size()
        h = torch.full((nbytes,), 0xFF, dtype=torch.uint8).view(dt).reshape(shape)
        words = _store(y.reshape(c.B, c.H, c.W, c.C), fmt, fault)
        if fault == "halo_off_by_one_pixel":
            h[:, 1:-1, 2:] = words
        else:
            h[:, 1:-1, 1:-1] = words
        got["halo"] = h
    return got
