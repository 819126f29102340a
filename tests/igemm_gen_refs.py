"""The statistics (ST) and generalised-addressing (GEN) instantiations of csrc/igemm.hip: which (family, row) carries which, the descriptors that reach
each one, the smallest non-square shapes at which their addressing and their partial layout can go wrong, float64 references with a-priori bounds, the
checks on what a launch wrote, and a CPU emulation of the addressing and of the statistics epilogue into which faults are planted.
tests/test_igemm_gen_refs.py holds the table against the source text and plants the faults; tests/test_igemm_gen_gpu.py runs every row on the GPU.
Tile geometry, data sets, guards, out_f32 / copy checks and the rounding model are those of tests/igemm_refs.py and tests/fused_refs.py.

Table.  GTABLE[family][key] = the Forms (st, gen, sk, tune, how) of row `key` (geometry: row(family, key), i.e. igemm_refs.TABLE plus the f32 tile 0 that
exists with statistics only).  `how` says which descriptor reaches the instantiation.  Two Forms are `big`: the f32 128 x 128 statistics tile and the x3
128 x 128 statistics tile with generalised addressing are selected by the grid alone (>= 256 tiles of 128 x 128; tune is not consulted), so their one case
is 32768 x 128 x 32 -- the only cases beyond the size rule of 4 BM rows x (2 BN + 4) columns.  UNREACHABLE lists the instantiations that exist in the
source and that no descriptor reaches, each with the statement that shuts it out.  The weight-row-group descriptors of the training step reach the same
GEN + split-K instantiations as the row groups here; their addressing is covered by tests/test_train_layer_bwd_gpu.py.

Cases (cases(family, key)), everything non-square:
* GEN without statistics: same_s2 (3x3, stride 2, pad 0 on a halo image: timm 'SAME'; B 2, 10 x 14 -> 5 x 7, Cin = BK, bias + res1 + ReLU + haloed copy),
  pad1_s2 (Conv2d(3, 2, 1); B 3, 9 x 13 -> 5 x 7, Cin = 2 BK), gather_s2 (strided 1x1 on an un-haloed 9 x 14 image whose skipped pixels are NaN; one
  k-tile and NS + 1), s1_gen (stride 1, pad 1 with Hi / Wi given; also compared bitwise with the plain instantiation of the row), groups (3 groups of 37
  rows, ldx = K + 16 with NaN padding, grp_off = ldx so that each group's first row -- NaN -- is skipped, a NaN gap of 32 elements behind every group;
  max(1, NS - 1) and 2 NS + 1 k-tiles), readout (the same with the second A segment: seg2_k 128 of Cin 256 and 256 of 384, read from the group's first
  row, which now holds data), and for GEN + split-K one groups case in 2 splits.  N = BN + 4 throughout.  Row 21's GEN instantiation runs with a stamps
  buffer (the only descriptor that reaches it).
* ST: linear rows (ldx = K + 16, NaN padding) and the default 3x3 for the plain form, same_s2 and gather_s2 for the GEN form (f32 / x2w have one form for
  both); gn_hw = BM and 2 BM with B 2 as the non-square maps MAPS; gn_cpg 2, one of 4 / 8 / 16 / 32 and BN; N = BN + BN / 2 (a ragged last n-tile), BN
  and 2 BN; one case per form with |mean| of every group several standard deviations from zero ("dc": operands of one sign, real data only).
  No bias or residual (the forward launches none with statistics).  {mean, rstd} are requested (gn_count) where the group count divides 256, which the
  finishing launch demands.

Data sets: igemm_refs' "exact" and "real".  The exact set of a statistics case is +-1 (every sum and sum of squares of a tile stays an integer below 2^24:
check_part asserts it and then compares the partials bitwise); cases whose expected sum of squares 2 K BM cpg leaves that range, and the dc cases, run
the real set only and carry "real only" in their name.

Bounds.  out_f32: that of igemm_refs.  A partial {sum, sum of squares} of a tile and group is BM x cpg values added in f32 (the squares with one fma
each): |error| <= gamma(BM cpg) sum |v|, resp. sum v^2, against float64 sums of the launch's own out_f32.  {mean, rstd}: d mean = d a / n + u |mean|,
d var = d q / n + (2 |mean| + d mean) d mean, rstd taken at both ends of [var - d var, var + d var] (it is monotone) + 2 u rstd.
"""
from __future__ import annotations

import re
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from tests import fused_refs as R
from tests import igemm_refs as G

Form = namedtuple("Form", "st gen sk tune how stamps big")


def _f(st, gen, sk, tune, how, stamps=False, big=False):
    return Form(bool(st), bool(gen), bool(sk), tune, how, stamps, big)


def _st2(t):
    return (_f(1, 0, 0, t, f"tune {t}, gn_stats, no generalised addressing"), _f(1, 1, 0, t, f"tune {t}, gn_stats, generalised addressing"))


def _gen(t):
    return (_f(0, 1, 0, t, f"tune {t}, generalised addressing"),)


_G16 = {1: _st2(1), 4: _st2(4), 23: _st2(23),
        21: _st2(21) + (_f(0, 1, 0, 21, "tune 21 with a stamps buffer (diagnostics)", stamps=True),),
        2: _gen(2) + _st2(2),
        20: _gen(20) + _st2(20) + (_f(0, 1, 1, 20, "tune 20, splitk > 1, generalised addressing"),),
        46: (_f(0, 1, 1, 46, "tune 46, splitk > 1, generalised addressing"),)}
_BIG = "the grid alone: >= 256 tiles of 128 x 128"
GTABLE = {
    "bf16": _G16, "f16": _G16,
    "x3": {0: (_f(1, 0, 0, 0, "tune 0, gn_stats"), _f(1, 1, 0, -1, "gn_stats, generalised addressing, gn_cpg 128, " + _BIG, big=True)),
           1: _gen(1) + _st2(1), 4: _gen(4) + _st2(4),
           3: (_f(1, 0, 0, 3, "tune 3, gn_stats"),), 7: (_f(1, 0, 0, 7, "tune 7, gn_stats"),), 12: (_f(1, 0, 0, 12, "tune 12, gn_stats"),),
           "sk": (_f(0, 1, 1, -1, "splitk > 1, generalised addressing"),), "sk3": (_f(0, 1, 1, 3, "tune 3, splitk > 1, generalised addressing"),)},
    "f32": {0: (_f(1, 1, 0, -1, "gn_stats, " + _BIG, big=True),),
            1: (_f(0, 1, 0, -1, "generalised addressing"), _f(1, 1, 0, -1, "gn_stats on fewer than 256 tiles of 128 x 128, or gn_hw % 128 != 0")),
            "sk": (_f(0, 1, 1, -1, "splitk > 1, generalised addressing"),), "sk3": (_f(0, 1, 1, 3, "tune 3, splitk > 1, generalised addressing"),)},
    "x2w": {0: (_f(0, 1, 0, 0, "tune 0, generalised addressing"), _f(1, 1, 0, 0, "tune 0, gn_stats")),
            2: (_f(0, 1, 0, 2, "tune 2, generalised addressing"), _f(1, 1, 0, 2, "tune 2, gn_stats"))},
}
# (family of the source, key, st, gen, sk) that the source instantiates and no descriptor reaches -> the statements that shut it out: with need_gen the
# tune branch of pick_cfg_f32 returns 1 and 4 only, and the rules behind it return 4, 1 or 0
_X3_TUNE = ("if (d.gn_stats && (t == 0 || t == 1 || t == 3 || t == 4 || t == 7 || t == 12) && d.gn_hw % bm == 0 && bn % d.gn_cpg == 0 && "
            "!(gen && t != 1 && t != 4)) return t;")
UNREACHABLE = {("x3", 3, True, True, False): _X3_TUNE, ("x3", 7, True, True, False): _X3_TUNE}

_ROWS_EXTRA = {("f32", 0): G._r(128, 128, 32, 2, 2, 2)}   # igemm_refs.NOT_ROWS: exists with the statistics epilogue only


def row(family, key):
    return _ROWS_EXTRA.get((family, key)) or G.TABLE[family][key]


def configs():
    return [(f, k) for f in G.FAMILIES for k in GTABLE[f]]


ROUTING_LINES = {
    "16-bit: tune selects the id": "if (d.tune >= 0) return d.tune;",
    "16-bit heuristic with statistics (not relied on: every case names its row)": "return (d.gn_hw % 128 == 0 && d.gn_cpg <= 128 && t128 >= 256) ? 21 : 23;",
    "16-bit heuristic with generalised addressing": "return (d.Cin % 128 == 0 && t64 < 256) ? 20 : 2;",
    "what needs GEN": "return d.stride != 1 || d.pad != 1 || d.in_halo != 1 || d.Hi || d.Wi || d.gather1 || d.grp_rows || d.seg2_k || d.stamps || d.wt_grp_rows;",
    "launch_cfg_st: plain statistics launches skip GEN": "if (!need_gen(d)) return d.f16 ? launch_cfg_t<C, f16_t, false, false, true, false>(d, stream, err) : "
                                                         "launch_cfg_t<C, bf16_t, false, false, true, false>(d, stream, err);",
    "launch_cfg_st: otherwise ST + GEN": "return d.f16 ? launch_cfg_t<C, f16_t, false, false, true, true>(d, stream, err) : "
                                         "launch_cfg_t<C, bf16_t, false, false, true, true>(d, stream, err);",
    "launch_cfg_gen: statistics go through launch_cfg_st": "if (d.gn_stats) return launch_cfg_st<C>(d, stream, err);",
    "launch_cfg_gen: GEN alone": "return d.f16 ? launch_cfg_t<C, f16_t, false, false, false, true>(d, stream, err) : "
                                 "launch_cfg_t<C, bf16_t, false, false, false, true>(d, stream, err);",
    "row 21: GEN alone with stamps only": "if (d.stamps && !d.gn_stats)",
    "row 20: GEN + split-K": "if (d.gn_stats || (need_gen(d) && d.splitk <= 1)) return launch_cfg_gen<Cfg<32, 64, 128, 2, 2, 3>>(d, stream, err);",
    "a row without the instantiation refuses": "if (!GEN && need_gen(d)) { err =",
    "a row without statistics refuses": "if (ST != (d.gn_stats != nullptr)) { err =",
    "x3: tune is consulted with statistics / GEN": "if (d.x3 && d.tune >= 0 && d.splitk <= 1 && !d.ln_g && (d.gn_stats || need_gen(d))) {",
    "x3: tile sizes of the tuned ids": "const int bm = (t == 0 || t == 3 || t == 7) ? 128 : 64, bn = (t == 0 || t == 3) ? 128 : 64;",
    "x3: tuned statistics ids; with GEN 1 and 4 only": _X3_TUNE,
    "x3: tuned GEN ids": "if (!d.gn_stats && gen && (t == 1 || t == 4)) return t;",
    "x3: untuned plain statistics": "if (d.x3 && d.gn_stats && d.splitk <= 1 && !need_gen(d)) {",
    "x3: statistics + GEN on 64 x 64 tiles": "if (d.x3 && d.gn_stats && d.splitk <= 1 && d.gn_hw % 64 == 0 && 64 % d.gn_cpg == 0) {",
    "x3: ... 4 or 1": "return (d.N < 128 || b64 < 256) ? 4 : 1;",
    "f32 / x3: statistics otherwise: 0 on big grids, else 1": "if (d.gn_stats) return (d.gn_hw % 128 == 0 && (long)((d.M + 127) / 128) * ((d.N + 127) / 128) >= 256) ? 0 : 1;",
    "f32 / x3: GEN otherwise": "if (need_gen(d)) return 1;",
    "x3 split-K + GEN": "if (need_gen(d) && d.tune == 3) return launch_cfg_t<Cfg<128, 128, 64, 2, 4, 2>, x3_t, false, true, false, true>(d, stream, err);",
    "f32 split-K + GEN": "if (need_gen(d)) return launch_cfg_t<Cfg<64, 64, 64, 2, 2, 4>, float, false, true, false, true>(d, stream, err);",
    "x2w: Cin % 64 != 0 selects 4": "if (!k64) return 4;",
    "x2w: tune 0-2 selects the tile": "if (d.tune >= 0 && d.tune <= 2) return d.tune;",
    "x2w: tile 1 has neither": "case 1: if (gen || d.gn_stats) break;",
    "statistics preconditions": "if (!d.gn_part || !d.out_f32 || d.gn_cpg <= 0 || d.N % d.gn_cpg || C::BN % d.gn_cpg || d.gn_hw <= 0 || d.gn_hw % C::BM || d.M % d.gn_hw ||",
    "statistics preconditions (2)": "(size_t)mtiles * G * 2 > d.gn_part_floats || G > C::THREADS ||",
    "taps stay inside the image": "if (d.stride < 1 || lo < 0 || hiy >= Hi + 2 * d.in_halo || hix >= Wi + 2 * d.in_halo) { err =",
    "second segment": "if (d.seg2_k && (d.taps != 1 || d.gather1 || !d.grp_rows || d.seg2_k % 128 != 0 || d.seg2_k >= d.Cin)) { err =",
    "row groups are plain mode": "if (d.grp_rows && (d.taps != 1 || d.gather1)) { err =",
    "x3 offsets": "if (d.ldx % 16 || d.Cin % 32 || (d.out_op && !d.out_op_f32 && d.out_fmt != 1 && d.N % 16) || d.grp_off % 16 || d.seg2_off % 16 || d.grp_stride % 16) { err =",
}
# soccdpt_op_igemm (csrc/capi.cpp) refuses x3 tune 12 with a generalised descriptor, which pick_cfg_f32 would pass over for tile 4 or 1
CAPI_LINE = "if (d.x3 && d.tune == 12 && d.splitk <= 1 && !d.ln_g &&"
FINISH_LINE = "if (256 % gw) { err = \"gn_finish: the group count must divide 256\"; return 1; }"   # csrc/hybrid.hip: launch_gn_finish


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's source text
# ---------------------------------------------------------------------------------------------------------------------------------
_CALL = re.compile(r"launch_cfg_t<Cfg<([\d, ]+)>, (\w+)((?:, (?:true|false))*)>")
_FAM_OF_T = {"bf16_t": "16", "f16_t": "16", "x3_t": "x3", "float": "f32", "x2w_t": "x2w"}


def _flags(txt):
    f = [t.strip() == "true" for t in txt.split(",")[1:]]
    return f + [False] * (5 - len(f))      # LN, SK, ST, GEN, D3


def _wrapper_forms(src, name):
    """{(st, gen, sk)} with st or gen that a 16-bit wrapper `launch_cfg_<name>` can launch (a wrapper that hands on to another one inherits its forms)."""
    body = src[src.index(f"static int {name}("):]
    body = body[:body.index("\n}\n")]
    forms = set()
    for m in re.finditer(r"launch_cfg_t<C, \w+((?:, (?:true|false))*)>", body):
        ln, sk, st, gen, d3 = _flags("C" + m.group(1))
        if st or gen:
            forms.add((st, gen, sk))
    for other in re.findall(r"return (launch_cfg_\w+)<C>", body):
        if other not in ("launch_cfg", name):
            forms |= _wrapper_forms(src, other)
    return forms


def parse_instantiations(src: str):
    """{(family of the source, key, st, gen, sk)} of every igemm instantiation with ST or GEN that launch_igemm names, keyed as GTABLE is.  Anchors: those of
    igemm_refs.parse_launcher; the f32 / x3 split-K forms stand before the family's switch and are told apart by their M tile (128: "sk3", 64: "sk")."""
    body = src[src.index("int launch_igemm("):]
    i2, i3, i32, i16 = body.index("if (d.x2w) {"), body.index("if (d.x3) {"), body.index("if (d.f32) {"), body.index("const int id = pick_cfg(d);")
    out = set()

    def add(fam, key, text):
        for cfg, t, fl in _CALL.findall(text):
            ln, sk, st, gen, d3 = _flags("T" + fl)
            if (st or gen) and not ln and not d3:
                assert _FAM_OF_T[t] == fam, (fam, key, t)
                geom = G._row_of_cfg(G._cfg_args(cfg), fam)
                k = key if key is not None else ("sk3" if geom[0] == 128 else "sk")
                out.add((fam, k, st, gen, sk) + (geom,))

    def by_case(fam, text):
        parts = re.split(r"\b(case \d+|default):", text)
        add(fam, None, parts[0])
        for label, b in zip(parts[1::2], parts[2::2]):
            key = "n32" if label == "default" else int(label.split()[1])
            add(fam, key, b)
            if fam == "16":
                for name in re.findall(r"return (launch_cfg_(?:st|gen))<Cfg<[\d, ]+>>", b):
                    geom = G._row_of_cfg(G._cfg_args(re.search(r"Cfg<([\d, ]+)>", b).group(1)), fam)
                    out.update(("16", key, st, gen, sk, geom) for st, gen, sk in _wrapper_forms(src, name))

    x2w = body[i2:i3]
    sw, tail = x2w[x2w.index("switch ("):].split("default: break;")
    by_case("x2w", sw)
    add("x2w", 0, tail)
    for fam, blk in (("x3", body[i3:i32]), ("f32", body[i32:i16][:body[i32:i16].index("if (d.dot3) {")])):
        s = blk.index("switch (")
        add(fam, None, blk[:s])
        by_case(fam, blk[s + len("switch ("):])
    t16 = body[i16:]
    by_case("16", t16[t16.index("switch (id)") + len("switch (id)"):])
    return out


def table_instantiations():
    """The same set from GTABLE + UNREACHABLE."""
    out = set()
    for fam, src_fam in (("bf16", "16"), ("x3", "x3"), ("f32", "f32"), ("x2w", "x2w")):
        for key, forms in GTABLE[fam].items():
            r = row(fam, key)
            out.update((src_fam, key, f.st, f.gen, f.sk, (r.BM, r.BN, r.BK, r.WM, r.WN, r.NS, r.MF)) for f in forms)
    for (fam, key, st, gen, sk) in UNREACHABLE:
        r = row(fam, key)
        out.add((fam, key, st, gen, sk, (r.BM, r.BN, r.BK, r.WM, r.WN, r.NS, r.MF)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GCase:
    name: str
    kind: str                 # "conv" (taps 9), "gather" (taps 1, gather1), "linear"
    N: int
    Cin: int
    B: int = 0
    H: int = 0                # OUTPUT map (conv / gather)
    W: int = 0
    Hi: int = 0               # input map; 0 with gen_conv False: the default 3x3 of an H x W halo image
    Wi: int = 0
    gen_conv: bool = False    # a conv dict (stride, pad, in_halo, Hi, Wi) is passed
    stride: int = 1
    pad: int = 1
    in_halo: int = 1
    rows: int = 0             # linear: M
    ldx: int = 0
    grp_rows: int = 0
    grp_off: int = 0
    grp_stride: int = 0
    seg2_k: int = 0
    seg2_off: int = 0
    splitk: int = 1
    epi: bool = True          # bias + res1
    copy: bool = False        # ReLU + haloed operand copy
    cpg: int = 0              # statistics: channels per group, pixels per sample, {mean, rstd} requested
    hw: int = 0
    count: bool = False
    dc: bool = False
    stamps: bool = False
    tune: int = -1
    datasets: tuple = ("exact", "real")
    twin: bool = False        # also run without the conv dict and compare bitwise

    @property
    def taps(self):
        return 9 if self.kind == "conv" else 1

    @property
    def M(self):
        return self.rows if self.kind == "linear" else self.B * self.H * self.W

    @property
    def K(self):
        return self.taps * self.Cin

    @property
    def gen(self):            # need_gen of igemm.hip
        return self.gen_conv or self.kind == "gather" or bool(self.grp_rows or self.seg2_k or self.stamps)

    @property
    def st(self):
        return self.cpg > 0

    def plain(self):
        """The igemm_refs.Case with the fields check_out / check_copy read."""
        return G.Case(self.kind, self.M, self.N, self.Cin, self.taps, self.ldx, self.B, self.H, self.W, self.tune, self.splitk, 0, self.name)


MAPS = {32: (4, 8), 64: (4, 16), 128: (8, 16), 256: (8, 32), 8192: (64, 128)}   # gn_hw -> the non-square output map
MID_CPG = (4, 8, 16, 32)


def instantiation(family, key, c: GCase):
    """(st, gen, sk) of the instantiation launch_igemm runs for case c on row key: the wrappers and the switches restated."""
    sk = c.splitk > 1
    if c.st and family in ("f32", "x2w"):
        return (True, True, sk)
    if c.st and family == "x3" and key == 12:
        return (True, False, sk)
    return (c.st, c.gen, sk)


def _linear(name, M, N, nk, r, **kw):
    K = nk * r.BK
    return GCase(name, "linear", N, K, rows=M, ldx=K + 16, **kw)


def _groups(name, nk, r, seg2_k=0, Cin=0, **kw):
    """3 groups of 37 rows.  Storage per group: [first row (skipped; the second segment under seg2)] [37 rows of ldx] [32 elements of NaN]."""
    K = Cin or nk * r.BK
    ldx = (max(seg2_k, K - seg2_k) if seg2_k else K) + 16
    return GCase(name, "linear", r.BN + 4, K, rows=3 * 37, ldx=ldx, grp_rows=37, grp_off=ldx, grp_stride=38 * ldx + 32, seg2_k=seg2_k, seg2_off=0, **kw)


def _same_s2(name, B, h, w, Cin, N, **kw):
    return GCase(name, "conv", N, Cin, B=B, H=h, W=w, Hi=2 * h, Wi=2 * w, gen_conv=True, stride=2, pad=0, in_halo=1, **kw)


def _gather_s2(name, B, h, w, Cin, N, **kw):
    return GCase(name, "gather", N, Cin, B=B, H=h, W=w, Hi=2 * h - 1, Wi=2 * w, gen_conv=True, stride=2, pad=0, in_halo=0, **kw)


def _exact_ok(K, r, cpg):
    return 2 * K * r.BM * cpg < 2 ** 24


def _st_kw(r, K, cpg, hw, count=False, dc=False, **kw):
    ds = ("exact", "real") if (_exact_ok(K, r, cpg) and not dc) else ("real",)
    return dict(cpg=cpg, hw=hw, count=count, dc=dc, epi=False, datasets=ds, **kw)


def _nm(name, kw):
    return name + (" (real only)" if kw["datasets"] == ("real",) else "")


def cases(family, key):
    """The launches of one row of GTABLE, every Form of the row among them (module docstring)."""
    r = row(family, key)
    forms = GTABLE[family][key]
    out = []
    BM, BN, BK, NS = r.BM, r.BN, r.BK, r.NS
    for f in forms:
        t = dict(tune=f.tune, stamps=f.stamps)
        if f.big:      # one case: the smallest grid that selects the tile
            kw = _st_kw(r, BK, BN, 8192, **t)
            if family == "x3":
                out.append(_gather_s2("big gather_s2, gn_hw 64 x 128, cpg BN", 4, 64, 128, BK, BN, **kw))
            else:
                out.append(_linear("big linear, gn_hw 8192, cpg BN", 32768, BN, 1, r, **kw))
        elif f.gen and not f.st and not f.sk:
            out += [_same_s2("same_s2", 2, 5, 7, BK, BN + 4, copy=True, **t),
                    GCase("pad1_s2", "conv", BN + 4, 2 * BK, B=3, H=5, W=7, Hi=9, Wi=13, gen_conv=True, stride=2, pad=1, in_halo=1, copy=True, **t),
                    _gather_s2("gather_s2, 1 k-tile", 2, 5, 7, BK, BN + 4, **t),
                    _gather_s2(f"gather_s2, {NS + 1} k-tiles", 2, 5, 7, (NS + 1) * BK, BN + 4, **t),
                    GCase("s1_gen", "conv", BN + 4, BK, B=2, H=5, W=7, Hi=5, Wi=7, gen_conv=True, copy=True, twin=not f.stamps, **t),
                    _groups(f"groups, {max(1, NS - 1)} k-tile(s)", max(1, NS - 1), r, **t),
                    _groups(f"groups, {2 * NS + 1} k-tiles", 2 * NS + 1, r, **t),
                    _groups("readout, seg2_k 128 of 256", 0, r, seg2_k=128, Cin=256, **t),
                    _groups("readout, seg2_k 256 of 384", 0, r, seg2_k=256, Cin=384, **t)]
        elif f.gen and f.sk:
            out.append(_groups(f"groups, split-K 2 of {2 * NS + 1} k-tiles", 2 * NS + 1, r, splitk=2, **t))
        elif f.st:
            mid = [m for m in MID_CPG if BN % (2 * m) == 0]
            h1, w1 = MAPS[BM]
            h2, w2 = MAPS[2 * BM]
            plain_desc = not f.gen or family in ("f32", "x2w")
            gen_desc = f.gen
            if plain_desc:
                m0, m1 = mid[key % len(mid) if isinstance(key, int) else 0], mid[-1]
                kw = _st_kw(r, BK, 2, BM, **t)
                out.append(_linear(_nm("st linear, gn_hw BM, cpg 2, ragged N", kw), 2 * BM, BN + BN // 2, 1, r, **kw))
                kw = _st_kw(r, (NS + 1) * BK, BN, 2 * BM, count=True, **t)
                out.append(_linear(_nm(f"st linear, gn_hw 2 BM, cpg BN, {NS + 1} k-tiles, stats", kw), 4 * BM, BN, NS + 1, r, **kw))
                kw = _st_kw(r, 2 * BK, m0, BM, count=True, dc=True, **t)
                out.append(_linear(_nm(f"st linear dc, gn_hw BM, cpg {m0}, N 2 BN, stats", kw), 2 * BM, 2 * BN, 2, r, **kw))
                kw = _st_kw(r, 9 * BK, m1, BM, **t)
                out.append(GCase(_nm(f"st 3x3 {h1} x {w1}, cpg {m1}, ragged N", kw), "conv", BN + BN // 2, BK, B=2, H=h1, W=w1, **kw))
            if gen_desc:
                m0, m1 = mid[0], mid[(key + 1) % len(mid) if isinstance(key, int) else -1]
                kw = _st_kw(r, 9 * BK, 2, BM, **t)
                out.append(_same_s2(_nm(f"st same_s2 {h1} x {w1}, cpg 2, ragged N", kw), 2, h1, w1, BK, BN + BN // 2, **kw))
                kw = _st_kw(r, BK, BN, 2 * BM, count=True, **t)
                out.append(_gather_s2(_nm(f"st gather_s2 {h2} x {w2}, cpg BN, stats", kw), 2, h2, w2, BK, BN, **kw))
                kw = _st_kw(r, 2 * BK, m1, BM, count=True, dc=True, **t)
                out.append(_gather_s2(_nm(f"st gather_s2 dc {h1} x {w1}, cpg {m1}, N 2 BN, stats", kw), 2, h1, w1, 2 * BK, 2 * BN, **kw))
                kw = _st_kw(r, 9 * BK, m0, 2 * BM, **t)
                out.append(_same_s2(_nm(f"st same_s2 {h2} x {w2}, cpg {m0}, 2 tiles per sample", kw), 2, h2, w2, BK, BN, **kw))
    return out


def _cdiv(a, b):
    return -(-a // b)


def x3_pick(c: GCase):
    """pick_cfg_f32 for an unsplit x3 launch with statistics or generalised addressing."""
    t, gen, st = c.tune, c.gen, c.st
    if t >= 0:
        bm, bn = (128 if t in (0, 3, 7) else 64), (128 if t in (0, 3) else 64)
        if st and t in (0, 1, 3, 4, 7, 12) and c.hw % bm == 0 and bn % c.cpg == 0 and not (gen and t not in (1, 4)):
            return t
        if not st and gen and t in (1, 4):
            return t
    b64 = _cdiv(c.M, 64) * _cdiv(c.N, 64)
    if st and not gen:
        if c.taps == 1 and c.Cin <= 256 and b64 > 256 and c.hw % 64 == 0 and 64 % c.cpg == 0 and t < 0:
            return 12
        if c.hw % 128 == 0 and 128 % c.cpg == 0 and c.N >= 256 and c.M >= 32768:
            return 3
        if c.hw % 64 == 0 and 64 % c.cpg == 0 and not (c.taps == 9 and 256 <= b64 < 512):
            return 4
    if st and c.hw % 64 == 0 and 64 % c.cpg == 0:
        return 4 if (c.N < 128 or b64 < 256) else 1
    if st:
        return 0 if (c.hw % 128 == 0 and _cdiv(c.M, 128) * _cdiv(c.N, 128) >= 256) else 1
    return 1


def precondition_errors(family, key, c: GCase):
    """launch_igemm's preconditions (and launch_gn_finish's, where {mean, rstd} are requested) that case c violates on row key, and the conditions under
    which it would run another row or instantiation: none, for a generated case."""
    r = row(family, key)
    bad = []
    esz = G.ELEM_BYTES[family]
    if c.N % 4: bad.append("N % 4")
    if c.Cin % 32: bad.append("Cin % 32")
    if c.Cin % r.cin_div: bad.append(f"Cin % {r.cin_div}")
    if c.taps not in (1, 9): bad.append("taps")
    if c.kind != "linear":
        if c.H <= 0 or c.W <= 0 or c.M % (c.H * c.W): bad.append("conv geometry")
        Hi, Wi, k = c.Hi or c.H, c.Wi or c.W, 3 if c.taps == 9 else 1
        stride, pad, halo = (c.stride, c.pad, c.in_halo) if c.gen_conv else (1, 1, 1)
        lo = halo - pad
        if stride < 1 or lo < 0 or (c.H - 1) * stride + k - 1 + lo >= Hi + 2 * halo or (c.W - 1) * stride + k - 1 + lo >= Wi + 2 * halo:
            bad.append("taps leave the input image")
        if not c.gen_conv and (c.Hi or c.Wi or c.kind == "gather"): bad.append("a generalised convolution needs the conv dict")
    if c.seg2_k and (c.kind != "linear" or not c.grp_rows or c.seg2_k % 128 or c.seg2_k >= c.Cin): bad.append("second segment")
    if c.grp_rows and c.kind != "linear": bad.append("row groups are plain mode")
    if c.kind == "linear":
        if family != "x3" and c.ldx * esz % 16: bad.append("ldx: 16 bytes")
        if not c.grp_rows and not c.seg2_k and c.ldx < c.Cin: bad.append("ldx < Cin")
        if c.grp_rows and c.M % c.grp_rows: bad.append("the cases hold whole groups")
    if family == "x3" and (c.ldx % 16 or c.grp_off % 16 or c.seg2_off % 16 or c.grp_stride % 16): bad.append("x3: multiples of 16 elements")
    if family in ("bf16", "f16", "x2w") and c.N <= 32 and c.Cin % 64: bad.append("N <= 32 needs Cin % 64 == 0")
    nk = c.K // r.BK
    if c.splitk > nk: bad.append("splits > nk")
    if c.splitk > 1 and (c.st or family == "x2w"): bad.append("no split-K with statistics / x2w")
    if c.st:
        Gn = c.N // c.cpg if c.cpg else 0
        if c.N % c.cpg or r.BN % c.cpg or c.hw <= 0 or c.hw % r.BM or c.M % c.hw or Gn > 64 * r.WM * r.WN: bad.append("statistics descriptor")
        if (2 * r.WM * r.BN + 4) * 4 + 64 * r.WM * r.WN * 16 > r.NS * (r.BM + r.BN * (2 if family == "x2w" else 1)) * r.BK * esz: bad.append("statistics scratch exceeds the ring")
        if c.count and (Gn > 256 or 256 % Gn): bad.append("gn_finish: the group count must divide 256")
        if c.epi or c.copy: bad.append("statistics launches carry no bias / residual here")
    elif c.count or c.dc: bad.append("statistics fields without statistics")
    if c.stamps and c.st: bad.append("stamps with statistics do not reach the GEN-only instantiation")
    # routing: the row and the instantiation
    inst = instantiation(family, key, c)
    form = [f for f in GTABLE[family][key] if (f.st, f.gen, f.sk) == inst]
    if not form: bad.append(f"row {key} has no instantiation {inst}")
    if family in ("bf16", "f16"):
        if c.tune != key: bad.append("16-bit rows are named by tune")
        if (key == 21 and inst == (False, True, False)) != c.stamps: bad.append("row 21 runs GEN alone with stamps, and only then")
        if key == 46 and c.splitk <= 1: bad.append("46 is the split-K form")
    elif family == "x2w":
        if c.tune != key or c.Cin % 64: bad.append("x2w rows 0-2: tune and Cin % 64 == 0")
    elif c.splitk > 1:
        if key != ("sk3" if c.tune == 3 else "sk"): bad.append("split-K tile is chosen by tune == 3")
    elif family == "x3":
        if x3_pick(c) != key: bad.append(f"x3 launch runs {x3_pick(c)}")
    else:
        big = c.st and c.hw % 128 == 0 and _cdiv(c.M, 128) * _cdiv(c.N, 128) >= 256
        if key != (0 if big else 1): bad.append("f32 tile is chosen by the grid")
    if form and not form[0].big and (c.M > 4 * r.BM or c.N > 2 * r.BN + 4): bad.append("case larger than 4 BM rows x (2 BN + 4) columns")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# data: the flat operand storage as the kernel reads it, and the im2col rows taken from the LOGICAL tensors (no index arithmetic of the kernel's)
# ---------------------------------------------------------------------------------------------------------------------------------
def storage_elems(c: GCase):
    if c.kind == "linear":
        n = 3 * c.grp_stride if c.grp_rows else c.M * c.ldx
    else:
        halo = c.in_halo if c.gen_conv else 1
        n = c.B * ((c.Hi or c.H) + 2 * halo) * ((c.Wi or c.W) + 2 * halo) * c.Cin
    return _cdiv(n, 16) * 16


def make_data(c: GCase, family, dataset, seed=0):
    """dict(X_src: the f32 flat storage (NaN where nothing may be read), store: the same as read (float64), cols [M][K], Wt_src, Wt, bias, res1)."""
    g = torch.Generator().manual_seed(seed * 7919 + c.M * 31 + c.N * 17 + c.Cin + len(c.name) * 101 + (1 if dataset == "real" else 0))
    mag = 1 if c.st else 4

    def draw(*shape):
        if c.dc:
            return torch.randn(shape, generator=g).abs() + 0.25
        return G.draw_values(g, dataset, shape, mag)
    nan = float("nan")
    n = storage_elems(c)
    if c.kind == "linear":
        flat = torch.full((n,), nan)
        if c.grp_rows:
            v = flat[:3 * c.grp_stride].view(3, c.grp_stride)
            k1 = c.seg2_k or c.K
            v[:, c.ldx:38 * c.ldx].view(3, 37, c.ldx)[:, :, :k1] = draw(3 * 37, k1).view(3, 37, k1)
            if c.seg2_k:
                v[:, :c.K - c.seg2_k] = draw(3, c.K - c.seg2_k)
        else:
            flat[:c.M * c.ldx].view(c.M, c.ldx)[:, :c.K] = draw(c.M, c.K)
    else:
        halo = c.in_halo if c.gen_conv else 1
        Hi, Wi = c.Hi or c.H, c.Wi or c.W
        flat = torch.zeros(n)
        img = flat[:c.B * (Hi + 2 * halo) * (Wi + 2 * halo) * c.Cin].view(c.B, Hi + 2 * halo, Wi + 2 * halo, c.Cin)
        L = draw(c.B * Hi * Wi, c.Cin).view(c.B, Hi, Wi, c.Cin)
        if c.kind == "gather":        # every pixel a stride-2 gather must skip
            L[:, 1::2] = nan
            L[:, :, 1::2] = nan
        img[:, halo:halo + Hi, halo:halo + Wi] = L
    store = G._as_read(flat.view(1, -1), G.x_fmt(family)).view(-1)
    d = dict(X_src=flat, store=store)
    # ---- the rows of the product, from the logical tensors ----
    if c.kind == "linear":
        if c.grp_rows:
            v = store[:3 * c.grp_stride].view(3, c.grp_stride)
            k1 = c.seg2_k or c.K
            cols = v[:, c.ldx:38 * c.ldx].reshape(3, 37, c.ldx)[:, :, :k1]
            if c.seg2_k:
                cols = torch.cat([cols, v[:, None, :c.K - c.seg2_k].expand(3, 37, c.K - c.seg2_k)], dim=2)
            cols = cols.reshape(c.M, c.K)
        else:
            cols = store[:c.M * c.ldx].view(c.M, c.ldx)[:, :c.K]
    else:
        simg = store[:img.numel()].view(img.shape)
        L = simg[:, halo:halo + Hi, halo:halo + Wi]
        stride, pad = (c.stride, c.pad) if c.gen_conv else (1, 1)
        k = 3 if c.taps == 9 else 1
        need_h, need_w = (c.H - 1) * stride + k - pad - Hi, (c.W - 1) * stride + k - pad - Wi     # zero rows / columns behind the image
        Lp = F.pad(L, (0, 0, pad, max(0, need_w), pad, max(0, need_h)))
        cols = torch.cat([Lp[:, ky:ky + (c.H - 1) * stride + 1:stride, kx:kx + (c.W - 1) * stride + 1:stride] for ky in range(k) for kx in range(k)], dim=3)
        cols = cols.reshape(c.M, c.K)
    assert not bool(cols.isnan().any())
    d["cols"] = cols.contiguous()
    d["Wt_src"] = draw(c.N, c.K)
    d["Wt"] = G._as_read(d["Wt_src"], G.w_fmt(family))
    if c.epi:
        if dataset == "exact":
            d["bias"], d["res1"] = torch.randint(-4, 5, (c.N,), generator=g).double(), torch.randint(-4, 5, (c.M, c.N), generator=g).double()
        else:
            d["bias"], d["res1"] = torch.randn(c.N, generator=g).double(), torch.randn(c.M, c.N, generator=g).double()
    else:
        d["bias"], d["res1"] = torch.zeros(c.N, dtype=torch.float64), torch.zeros(c.M, c.N, dtype=torch.float64)
    return d


def reference(c: GCase, family, key, d, dev="cpu"):
    """As igemm_refs.reference: v = acc + bias + res1 (float64), its bound, the split-K partial products."""
    r = row(family, key)
    cols, Wt, bias, res1 = d["cols"].to(dev), d["Wt"].to(dev), d["bias"].to(dev), d["res1"].to(dev)
    S = max(1, c.splitk)
    parts = [cols[:, lo:hi] @ Wt[:, lo:hi].t() for lo, hi in G.split_ranges(c.K // r.BK, S, r.BK)]
    acc = parts[0].clone()
    for p in parts[1:]:
        acc += p
    bound = R.gemm_gamma(family, c.K, r.MF) * (cols.abs() @ Wt.abs().t()) + R.gamma(2) * (acc.abs() + bias.abs() + res1.abs())
    if S > 1:
        bound = bound + R.gamma(S - 1) * sum(p.abs() for p in parts)
    return dict(v=acc + bias + res1, bound=bound, parts=parts, bias=bias, res1=res1)


# ---------------------------------------------------------------------------------------------------------------------------------
# checks on what a launch wrote
# ---------------------------------------------------------------------------------------------------------------------------------
PART_SLACK = 8     # floats behind the last used entry of gn_part that the launch is given and must leave alone
U32 = 2.0 ** -24


def part_floats(c: GCase, r):
    return (c.M // r.BM) * (c.N // c.cpg) * 2


def _is_ff(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def check_part(c: GCase, r, dataset, out_f32, part, what):
    """gn_part (f32, part_floats + PART_SLACK of them) read as [M tile][N / cpg][2] against float64 sums of the launch's own out_f32 over each tile's rows
    and each group's channels.  Returns (worst error / bound of the sums, of the sums of squares)."""
    out, part = out_f32.detach().cpu().float(), part.detach().cpu()
    mt, Gn = c.M // r.BM, c.N // c.cpg
    used = mt * Gn * 2
    assert part.numel() == used + PART_SLACK
    if not _is_ff(part[used:]):
        raise AssertionError(f"{what}: floats behind the last partial were written")
    P = part[:used].view(mt, Gn, 2)
    V = out.double().view(mt, r.BM, Gn, c.cpg)
    s, q, sa = V.sum((1, 3)), (V * V).sum((1, 3)), V.abs().sum((1, 3))
    gm = R.gamma(r.BM * c.cpg)
    if dataset == "exact":
        assert bool((V == V.round()).all()) and float(q.max()) < 2 ** 24 and float(sa.max()) < 2 ** 24, f"{what}: the exact data set left the integers of f32"
        exp = torch.stack([s, q], dim=2).float()
        same = (P.view(torch.int32) == exp.view(torch.int32)) | ((P == 0) & (exp == 0))
        if not bool(same.all()):
            t = tuple((~same).nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int((~same).sum())} of {same.numel()} partials differ from the exact sums; first at (tile, group, which) {t}: "
                                 f"got {float(P[t])!r}, expected {float(exp[t])!r}")
        return 0.0, 0.0
    return (R.check_bound(P[..., 0], s, gm * sa, what + ": partial sums"), R.check_bound(P[..., 1], q, gm * q, what + ": partial sums of squares"))


def stats_formula(a, q, n, eps=1e-5):
    """{mean, 1 / sqrt(var + eps)} with biased variance, float64."""
    mean = a / n
    var = (q / n - mean * mean).clamp(min=0.0)
    return mean, 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))


def check_stats(c: GCase, r, out_f32, part, stats, what):
    """gn_stats [B][N / cpg][2] = {mean, rstd}: (1) against float64 statistics of out_f32 within the bound propagated from the partials' bound, (2) against the
    same formula in float64 on the device's own partials within two f32 roundings.  Returns the worst error / bound of (1) for mean and rstd."""
    out, part, stats = out_f32.detach().cpu().float(), part.detach().cpu(), stats.detach().cpu().double()
    B, Gn, n = c.M // c.hw, c.N // c.cpg, c.hw * c.cpg
    V = out.double().view(B, c.hw, Gn, c.cpg)
    a, q, sa = V.sum((1, 3)), (V * V).sum((1, 3)), V.abs().sum((1, 3))
    mean, rstd = stats_formula(a, q, n)
    gm = R.gamma(r.BM * c.cpg)
    dmean = gm * sa / n + U32 * mean.abs()
    dvar = gm * q / n + (2 * mean.abs() + dmean) * dmean
    var = (q / n - mean * mean).clamp(min=0.0)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))
    drstd = torch.maximum(1.0 / torch.sqrt((var - dvar).clamp(min=0.0) + eps) - rstd, rstd - 1.0 / torch.sqrt(var + dvar + eps)) + 2 * U32 * rstd
    r1 = R.check_bound(stats[..., 0], mean, dmean, what + ": mean")
    r2 = R.check_bound(stats[..., 1], rstd, drstd, what + ": rstd")
    P = part[:part_floats(c, r)].double().view(B, c.hw // r.BM, Gn, 2).sum(1)
    pm, pr = stats_formula(P[..., 0], P[..., 1], n)
    R.check_bound(stats[..., 0], pm, 2 * U32 * pm.abs(), what + ": mean against the formula on the device's partials")
    R.check_bound(stats[..., 1], pr, 2 * U32 * pr, what + ": rstd against the formula on the device's partials")
    return r1, r2


def check_dc(c: GCase, out_f32):
    """A dc case is one only if every group's |mean| is several standard deviations from zero."""
    V = out_f32.detach().cpu().double().view(c.M // c.hw, c.hw, c.N // c.cpg, c.cpg)
    mean, std = V.mean((1, 3)), V.permute(0, 2, 1, 3).reshape(V.shape[0], V.shape[2], -1).std(-1)
    assert bool((mean.abs() >= 4 * std).all()), "dc case: a group's mean is less than 4 standard deviations from zero"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU emulation: the kernel's addressing on the flat storage, f32 accumulation in its order, the statistics epilogue's layout -- and planted faults
# ---------------------------------------------------------------------------------------------------------------------------------
ADDR_FAULTS = ("pitch_hw_swapped", "pitch_from_output", "stride_one_axis", "halo_minus_pad_dropped", "grp_off_dropped", "group_is_m_div_bm", "seg2_one_ktile_late")
STAT_FAULTS = ("part_pitch_is_bn", "ragged_groups_stored", "wave_row_left_out", "squares_miss_last_channel")


def fault_applies(fault, c: GCase, r):
    conv_gen = c.kind != "linear" and c.gen_conv
    ntiles = _cdiv(c.N, r.BN)
    return {"pitch_hw_swapped": c.kind != "linear" and (c.taps == 9 or c.B * c.H > 1),
            "pitch_from_output": conv_gen and bool(c.Wi) and c.Wi != c.W,
            "stride_one_axis": conv_gen and c.stride != 1,
            "halo_minus_pad_dropped": conv_gen and c.in_halo != c.pad,
            "grp_off_dropped": bool(c.grp_rows and c.grp_off),
            "group_is_m_div_bm": bool(c.grp_rows) and c.M > r.BM and c.grp_rows != r.BM,
            "seg2_one_ktile_late": bool(c.seg2_k),
            "part_pitch_is_bn": c.st and ntiles > 1 and c.M > r.BM,
            "ragged_groups_stored": c.st and c.N % r.BN != 0,
            "wave_row_left_out": c.st,
            "squares_miss_last_channel": c.st}[fault]


def kernel_index(c: GCase, r, fault=None):
    """[M][K] element offsets into the flat storage, by the arithmetic of igemm_kernel.h (x_off / stage), with one addressing fault planted."""
    m = torch.arange(c.M)[:, None]
    k = torch.arange(c.K)[None, :]
    if c.kind != "linear":
        stride, pad, halo = (c.stride, c.pad, c.in_halo) if c.gen_conv else (1, 1, 1)
        Hpi, Wpi = (c.Hi or c.H) + 2 * halo, (c.Wi or c.W) + 2 * halo
        if fault == "pitch_from_output":
            Wpi = c.W + 2 * halo
        hw = c.H * c.W
        b, rem = m // hw, m % hw
        y, x = rem // c.W, rem % c.W
        lo = 0 if fault == "halo_minus_pad_dropped" else halo - pad
        sx = 1 if fault == "stride_one_axis" else stride
        tap, ci = k // c.Cin, k % c.Cin
        ky, kx = (tap // 3, tap % 3) if c.taps == 9 else (0 * tap, 0 * tap)
        if fault == "pitch_hw_swapped":
            return ((b * Wpi + y * stride + lo) * Hpi + x * sx + lo) * c.Cin + (ky * Hpi + kx) * c.Cin + ci
        return ((b * Hpi + y * stride + lo) * Wpi + x * sx + lo) * c.Cin + (ky * Wpi + kx) * c.Cin + ci
    if c.grp_rows:
        g = m // r.BM if fault == "group_is_m_div_bm" else m // c.grp_rows
        rr = m - g * c.grp_rows
        base = g * c.grp_stride + (0 if fault == "grp_off_dropped" else c.grp_off) + rr * c.ldx
        if not c.seg2_k:
            return base + k
        wk = (k // r.BK) * r.BK                                       # the k-tile decides, as in the kernel
        in2 = wk >= c.seg2_k + (r.BK if fault == "seg2_one_ktile_late" else 0)
        return torch.where(in2, g * c.grp_stride + c.seg2_off + (k - c.seg2_k), base + k)
    return m * c.ldx + k


def _f32_product(cols, Wt, ranges):
    """sum_k cols Wt^T accumulated in f32 one 32-element k-step after the other (the MFMA chain), per split; the splits added in order in f32."""
    total = None
    for lo, hi in ranges:
        acc = torch.zeros(cols.shape[0], Wt.shape[0], dtype=torch.float32)
        for s in range(lo, hi, 32):
            acc = (acc.double() + cols[:, s:s + 32] @ Wt[:, s:s + 32].t()).float()
        total = acc if total is None else total + acc
    return total


def emulate_out(c: GCase, family, key, d, fault=None):
    """out_f32 of an f32-accumulating kernel that addresses the storage as igemm_kernel.h does (fault: one of ADDR_FAULTS).  Returns (out, changed):
    changed = the fault moved an address (the self-test asserts it)."""
    r = row(family, key)
    idx = kernel_index(c, r, fault)
    good = kernel_index(c, r) if fault else idx
    changed = not bool((idx == good).all())
    cols = d["store"][idx.clamp(0, d["store"].numel() - 1)]
    acc = _f32_product(cols, d["Wt"], G.split_ranges(c.K // r.BK, max(1, c.splitk), r.BK))
    return (acc + d["bias"].float()) + d["res1"].float(), changed


def emulate_part(c: GCase, r, out_f32, fault=None):
    """gn_part as the statistics epilogue leaves it (0xFF where it writes nothing), from out_f32 in the kernel's order of f32 additions: per lane over its m-tiles,
    a butterfly over the 16 lanes of a channel, then per group its channels and, per channel, the WM wave rows.  fault: one of STAT_FAULTS."""
    BM, BN, WM, cpg = r.BM, r.BN, r.WM, c.cpg
    mt, nt, Gn, gpt = c.M // BM, _cdiv(c.N, BN), c.N // cpg, BN // cpg
    Np = nt * BN
    V = torch.zeros(c.M, Np)
    V[:, :c.N] = out_f32.float()
    TM = BM // WM // 16
    V = V.view(mt, WM, TM, 16, Np)
    a = torch.zeros(mt, WM, 16, Np)
    q = torch.zeros(mt, WM, 16, Np)
    for j in range(TM):
        v = V[:, :, j]
        a = a + v
        q = (v.double() * v.double() + q.double()).float()
    for o in (1, 2, 4, 8):
        perm = torch.arange(16) ^ o
        a, q = a + a[:, :, perm], q + q[:, :, perm]
    ra, rq = a[:, :, 0].view(mt, WM, nt * gpt, cpg), q[:, :, 0].view(mt, WM, nt * gpt, cpg)
    sa, sq = torch.zeros(mt, nt * gpt), torch.zeros(mt, nt * gpt)
    for ch in range(cpg):
        for w in range(WM):
            if fault == "wave_row_left_out" and w == WM - 1 and WM > 1:
                continue
            sa = sa + ra[:, w, :, ch]
            if not (fault == "squares_miss_last_channel" and ch == cpg - 1):
                sq = sq + rq[:, w, :, ch]
    if fault == "wave_row_left_out" and WM == 1:      # a one-row layout: its only wave row
        sa, sq = sa * 0, sq * 0
    buf = torch.full(((mt * Gn * 2 + PART_SLACK) * 4,), 0xFF, dtype=torch.uint8).view(torch.float32)
    pitch = gpt if fault == "part_pitch_is_bn" else Gn
    for t in range(mt):
        for g in range(nt * gpt):
            if g * cpg >= c.N and fault != "ragged_groups_stored":
                continue
            i = (t * pitch + g) * 2
            if i + 1 < buf.numel():
                buf[i], buf[i + 1] = sa[t, g], sq[t, g]
    return buf


def emulate_stats(c: GCase, r, part):
    """launch_gn_finish: the tiles of a sample added in f64, {mean, rstd} rounded to f32."""
    B, Gn = c.M // c.hw, c.N // c.cpg
    P = part[:part_floats(c, r)].double().view(B, c.hw // r.BM, Gn, 2).sum(1)
    mean, rstd = stats_formula(P[..., 0], P[..., 1], c.hw * c.cpg)
    return torch.stack([mean, rstd], dim=2).float()
