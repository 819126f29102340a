"""The tile configurations of csrc/igemm.hip, the shapes that exercise each one's ring and tile edges, float64 references with a-priori bounds, and the
checks on what a launch wrote.  tests/test_igemm_refs.py holds the table against the source text and plants faults into a CPU emulation;
tests/test_igemm_tiles_gpu.py runs every configuration's cases on the GPU.

Table.  TABLE[family][key] = Row(BM, BN, BK, WM, WN, NS, MF, cin_div, sk): the tile in output rows x output channels x k-tile depth IN ELEMENTS OF THE
FAMILY (a Cfg's third argument counts bf16 elements: f32 / x3 rows hold half as many; x2w counts the fp16 activations), the wave layout, the ring depth,
the MFMA shape, the divisor of Cin the launcher demands for the row, and whether the row has a split-K form ("no", "also", "only").  Keys are the tune
ids; "n32" is the tile the f32 / x3 launcher takes for N <= 32 whatever tune says, "sk" / "sk3" / "sk8" are the split-K forms of f32 and x3 (default,
tune 3, tune 8).  Not rows: conv8p (ids 30-39, own launcher and test), and the ids that exist only with an epilogue this module does not drive (NOT_ROWS).

How a row is reached (launch_igemm):
* bf16 / f16: tune = id, any shape.  N <= 32 is refused unless Cin % 64 == 0 (the default tile for such N needs it), so the 32-deep rows run N = 4 with
  two k-tiles and the one-k-tile case with N = 36.
* x3: tune = id needs N > 32 (N <= 32 always takes the 128 x 32 tile, which is also id 2): the smallest N of the other rows is 36.  Ids 8-10 need
  Cin % 64 == 0 (their k-tile), else the launcher runs id 1.
* f32 ignores tune outside split-K: N <= 32 takes "n32", cdiv(M, 128) cdiv(N, 128) >= 384 takes 3, everything else 1.
* x2w: tune 0-2 with Cin % 64 == 0; 4 is what Cin % 64 != 0 selects, so its k-tile counts are odd and N <= 32 (refused with such Cin) does not occur.

Cases (cases(family, key)): per row, Linear launches with ldx = K + 16 and NaN in the 16 padding
columns at (M, N, k-tiles) = (1, 4, 1), (BM + 1, BN + 4, NS - 1), (BM - 1, BN - 4, NS), (2 BM + 17, BN + BN / 2, 2 NS + 1) without duplicates; 3 x 3
convolutions over zero-halo images (2, 5, 7) and (3, 9, 11) with Cin = BK and 2 BK and Cout = BN + 4; split-K forms with 6 k-tiles and 2, 4 and 6 splits
(eager with bias and residual, deferred without) and one convolution with 9 k-tiles in 4 splits.

Data sets: "exact" -- nonzero integers of magnitude <= 4 (x3 / x2w pairs with lo = 0): every partial sum is an integer below 2^24, so out_f32 must equal
the float64 result bitwise in every configuration; "real" -- randn with a power-of-two scale 2^-3 .. 2^3 per row, rounded (or x3-encoded and decoded)
exactly as the kernel reads it.

Bound of the real data set, per element: fused_refs.gemm_gamma(fmt, K, MF) sum |w| |x|  (the MFMA chains)  +  gamma(2) (|acc| + |bias| + |res1|)  (the
two epilogue additions)  +  gamma(S - 1) sum |partials|  (the in-order sum of S split-K partials).  No element is excluded.
"""
from __future__ import annotations

import re
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import fused_refs as R

Row = namedtuple("Row", "BM BN BK WM WN NS MF cin_div sk")
Case = namedtuple("Case", "kind M N Cin taps ldx B H W tune splitk sk_defer what")

FAMILIES = ("bf16", "f16", "f32", "x3", "x2w")
PREC = {"bf16": 0, "f32": 1, "f16": 2, "x3": 3, "x2w": 5}   # SOCCDPT_PREC_* of the launch


def _r(BM, BN, BK, WM, WN, NS, MF=16, sk="no", cin_div=None):
    return Row(BM, BN, BK, WM, WN, NS, MF, cin_div or BK, sk)


_T16 = {
    0: _r(128, 128, 64, 2, 2, 4), 1: _r(128, 128, 64, 2, 2, 2), 2: _r(64, 64, 64, 2, 2, 4), 3: _r(128, 128, 32, 2, 2, 4), 4: _r(64, 64, 32, 2, 2, 4),
    5: _r(128, 32, 64, 4, 1, 4), 6: _r(256, 128, 64, 4, 2, 2), 7: _r(256, 128, 64, 4, 2, 3), 8: _r(256, 256, 64, 2, 4, 2), 9: _r(128, 128, 32, 2, 2, 3),
    10: _r(128, 256, 64, 2, 4, 2), 11: _r(64, 64, 64, 2, 2, 6), 12: _r(64, 64, 64, 2, 2, 8), 13: _r(64, 128, 64, 2, 2, 4),
    14: _r(32, 64, 64, 2, 2, 6, sk="also"), 15: _r(128, 256, 32, 2, 4, 3), 16: _r(256, 128, 32, 4, 2, 3), 17: _r(128, 256, 32, 2, 4, 4),
    18: _r(256, 256, 32, 2, 4, 3), 19: _r(64, 128, 32, 2, 2, 4), 20: _r(32, 64, 128, 2, 2, 3, sk="also"), 21: _r(128, 128, 64, 2, 4, 2),
    22: _r(32, 64, 128, 2, 4, 3), 23: _r(64, 64, 64, 2, 4, 4), 24: _r(128, 128, 32, 2, 4, 3),
    40: _r(128, 128, 64, 2, 2, 2, 32), 41: _r(128, 128, 64, 2, 4, 2, 32), 42: _r(256, 128, 64, 4, 2, 2, 32), 43: _r(128, 256, 64, 2, 4, 2, 32),
    44: _r(256, 256, 64, 2, 4, 2, 32), 45: _r(128, 128, 64, 2, 2, 3, 32), 46: _r(128, 128, 64, 2, 4, 2, sk="only"),
    47: _r(256, 256, 64, 4, 4, 2), 48: _r(256, 256, 32, 4, 4, 4), 49: _r(512, 128, 64, 8, 2, 2), 50: _r(256, 128, 64, 4, 4, 2),
    51: _r(128, 256, 64, 2, 8, 2), 52: _r(128, 256, 64, 4, 4, 2),
}
_T4 = {   # the 4-byte families: a 128-byte tile row is 32 elements
    "x3": {0: _r(128, 128, 32, 2, 2, 2), 1: _r(64, 64, 32, 2, 2, 4), 2: _r(128, 32, 32, 4, 1, 4), 3: _r(128, 128, 32, 2, 4, 2), 4: _r(64, 64, 32, 2, 4, 4),
           5: _r(128, 128, 32, 2, 4, 3), 6: _r(128, 128, 32, 2, 4, 4), 7: _r(128, 64, 32, 2, 2, 3), 8: _r(128, 128, 64, 2, 4, 2), 9: _r(64, 64, 64, 2, 2, 3),
           10: _r(32, 64, 64, 2, 4, 3), 11: _r(64, 128, 32, 2, 2, 3), 12: _r(64, 64, 32, 2, 4, 2), "n32": _r(128, 32, 32, 4, 1, 4),
           "sk": _r(64, 64, 32, 2, 2, 4, sk="only"), "sk3": _r(128, 128, 32, 2, 4, 2, sk="only"), "sk8": _r(128, 128, 64, 2, 4, 2, sk="only")},
    "f32": {1: _r(64, 64, 32, 2, 2, 4), 3: _r(128, 128, 32, 2, 4, 2), "n32": _r(128, 32, 32, 4, 1, 4),
            "sk": _r(64, 64, 32, 2, 2, 4, sk="only"), "sk3": _r(128, 128, 32, 2, 4, 2, sk="only")},
}
TABLE = {"bf16": _T16, "f16": _T16, "x3": _T4["x3"], "f32": _T4["f32"],
         "x2w": {0: _r(64, 64, 64, 2, 4, 3), 1: _r(32, 64, 64, 2, 2, 4), 2: _r(128, 128, 64, 2, 4, 2), 4: _r(64, 64, 32, 2, 2, 4)}}
# `case` labels of the launcher's switches that are no rows, and why
NOT_ROWS = {"x2w": {3: "fused-LayerNorm tile: reached with ln_g only"}, "f32": {0: "reached with the LayerNorm or GroupNorm-statistics epilogue only"},
            "x3": {}, "16": {}}

ELEM_BYTES = {"bf16": 2, "f16": 2, "x2w": 2, "f32": 4, "x3": 4}   # of an X element as ldx counts it (x3: the pair occupies 4 bytes)
CHUNK_ELEMS = {"bf16": 8, "f16": 8, "x2w": 8, "f32": 4, "x3": 8}   # elements of a row that one 16-byte LDS-DMA piece moves together (x3: 8 hi or 8 lo values)


def configs():
    """Every (family, key) of the table, in a fixed order."""
    return [(f, k) for f in FAMILIES for k in TABLE[f]]


def config_id(fk):
    return f"{fk[0]}-{fk[1]}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the launcher's source text
# ---------------------------------------------------------------------------------------------------------------------------------
def _cfg_args(txt):
    a = [int(v) for v in txt.split(",")]
    return a + [16] if len(a) == 6 else a


def _row_of_cfg(a, family):
    """Cfg<BM, BN, BK in bf16 elements, WM, WN, NS[, MF]> -> the table's geometry tuple (BM, BN, BK in elements of the family, WM, WN, NS, MF)."""
    bk = a[2] // 2 if family in ("f32", "x3") else a[2]
    return (a[0], a[1], bk, a[3], a[4], a[5], a[6])


def _switch_cases(block, family):
    """{label: geometry} of a `switch` body: the first Cfg<> after every `case N:` / `default:` label."""
    out = {}
    parts = re.split(r"\b(case \d+|default):", block)
    for label, body in zip(parts[1::2], parts[2::2]):
        m = re.search(r"Cfg<([\d, ]+)>", body)
        if m:
            out["default" if label == "default" else int(label.split()[1])] = _row_of_cfg(_cfg_args(m.group(1)), family)
    return out


# The routing statements of igemm.hip that cases() and precondition_errors() restate in Python (what sends a launch to the row it was generated for).
# tests/test_igemm_refs.py asserts that each still stands in the source, whitespace aside: a changed rule fails there instead of quietly running
# a row's cases on another tile.
ROUTING_LINES = {
    "16-bit: tune selects the id": "if (d.tune >= 0) return d.tune;",
    "16-bit / x2w: N <= 32 refused unless Cin % 64 == 0": "if (d.N <= 32 && d.Cin % 64 != 0 && !d.f32 && !d.x3) { err =",
    "f32 / x3: tune is honoured for N > 32, unsplit, plain launches only": "const bool tunable = !d.gn_stats && !need_gen(d) && !d.ln_g && d.N > 32 && d.splitk <= 1;",
    "x3: tune in 0 .. 12": "if (d.x3 && d.tune >= 0 && d.tune < kNumCfgX3 && tunable) {",
    "x3: ids 8-10 fall back to 1 unless Cin % 64 == 0": "if (d.tune >= 8 && d.tune <= 10 && d.Cin % 64) return 1;",
    "f32 / x3: N <= 32 takes the 128 x 32 tile": "if (d.N <= 32) return 2;",
    "f32: the grid chooses between 3 and 1": "return b128 >= 384 ? 3 : 1;",
    "x3 split-K: tune 8 needs Cin % 64 == 0": "if (d.tune == 8 && d.Cin % 64 == 0) return launch_cfg_t<Cfg<128, 128, 128, 2, 4, 2>, x3_t, false, true>",
    "x2w: Cin % 64 != 0 selects 4": "if (!k64) return 4;",
    "x2w: tune 0-2 selects the tile": "if (d.tune >= 0 && d.tune <= 2) return d.tune;",
    "x2w has no split-K": "if (d.f32 || d.x3 || d.dot3 || d.out_dot || d.splitk > 1 || d.wt_grp_rows) { err =",
}


def parse_launcher(src: str):
    """What launch_igemm's switches say: {"16": {id: geometry}, "x3": {...}, "f32": {...}, "x2w": {...}} with the keys of TABLE ("default" of the f32 / x3
    switches is the 128 x 32 tile; x2w's code after the switch is id 0), plus "k64" / "k128": the ids the launcher refuses unless Cin % 64 / 128 == 0, and
    "sk_also" / "sk_only": the 16-bit ids that also carry, or only are, a split-K instantiation."""
    # Anchors in the source text this parser relies on (a change to any of them fails loudly here, not silently): the opening lines `if (d.x2w) {`,
    # `if (d.x3) {`, `if (d.f32) {` and `const int id = pick_cfg(d);` that separate the families; `default: break;` closing the x2w switch; the plain
    # split-K returns `Cfg<...>, x3_t | float, false, true>(` in the order tune 8, tune 3, default (x3) and tune 3, default (f32); the words
    # "needs Cin % 64 == 0" / "needs Cin % 128 == 0" on the lines that list the ids, "launch_cfg_sk<" and "is the split-K form" inside a case.
    body = src[src.index("int launch_igemm("):]
    i2, i3, i32, i16 = body.index("if (d.x2w) {"), body.index("if (d.x3) {"), body.index("if (d.f32) {"), body.index("const int id = pick_cfg(d);")
    out = {}
    x2w = body[i2:i3]
    sw, tail = x2w[x2w.index("switch ("):].split("default: break;")
    out["x2w"] = {k: v for k, v in _switch_cases(sw, "x2w").items()}
    out["x2w"][0] = _row_of_cfg(_cfg_args(re.search(r"Cfg<([\d, ]+)>", tail).group(1)), "x2w")
    for fam, blk, tag in (("x3", body[i3:i32], "x3_t"), ("f32", body[i32:i16], "float")):
        s = blk.index("switch (")
        rows = _switch_cases(blk[s:], fam)
        rows["n32"] = rows.pop("default")
        if fam == "x3":
            rows[2] = rows["n32"]   # no label of its own: tune 2 falls to the default
        plain_sk = [_row_of_cfg(_cfg_args(m), fam) for m in re.findall(r"Cfg<([\d, ]+)>, %s, false, true>\(" % tag, blk[:s])]
        names = ("sk8", "sk3", "sk") if fam == "x3" else ("sk3", "sk")
        assert len(plain_sk) == len(names), (fam, plain_sk)
        rows.update(zip(names, plain_sk))
        out[fam] = rows
    t16 = body[i16:]
    out["16"] = {k: v for k, v in _switch_cases(t16[t16.index("switch (id)"):], "16").items() if k != "default"}

    def ids_of(line):
        ids = {int(v) for v in re.findall(r"id == (\d+)", line)}
        for lo, hi in re.findall(r"id >= (\d+) && id <= (\d+)", line):
            ids |= set(range(int(lo), int(hi) + 1))
        return ids
    l64 = next(ln for ln in t16.splitlines() if "needs Cin % 64 == 0" in ln)
    l128 = next(ln for ln in t16.splitlines() if "needs Cin % 128 == 0" in ln)
    out["k64"], out["k128"] = ids_of(l64), ids_of(l128)
    parts = re.split(r"\bcase (\d+):", t16[t16.index("switch (id)"):])
    out["sk_also"] = {int(k) for k, b in zip(parts[1::2], parts[2::2]) if "launch_cfg_sk<" in b}
    out["sk_only"] = {int(k) for k, b in zip(parts[1::2], parts[2::2]) if "is the split-K form" in b}
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _tune(family, key):
    if family == "f32":
        return 3 if key == "sk3" else -1
    if family == "x2w":
        return -1 if key == 4 else key
    if isinstance(key, int):
        return key
    return {"n32": -1, "sk": -1, "sk3": 3, "sk8": 8}[key]


def _lin(M, N, nk, r, tune, what, splitk=1, defer=0):
    K = nk * r.BK
    return Case("linear", M, N, K, 1, K + 16, 0, 0, 0, tune, splitk, defer, what)


def _conv(B, H, W, Cin, N, tune, what, splitk=1):
    return Case("conv", B * H * W, N, Cin, 9, 0, B, H, W, tune, splitk, 0, what)


def cases(family, key):
    """The launches of one table row (see the module docstring)."""
    r = TABLE[family][key]
    tune = _tune(family, key)
    odd = family == "x2w" and key == 4                     # Cin must stay an odd multiple of 32
    kt = lambda n: n + 1 if odd and n % 2 == 0 else n
    if family == "f32" and key == 3:                          # selected by shape: 192 x 2 tiles of 128 x 128, M one short of a multiple of 128
        return [_lin(192 * 128 - 1, 132, nk, r, tune, f"384 tiles, ragged M, {nk} k-tile(s)") for nk in (1, 2)]
    out = []
    if r.sk != "only":
        n32 = key == "n32"
        tuned4 = family in ("x3", "f32") and not n32 and key != 2     # N <= 32 would run the 128 x 32 tile instead of this row
        small_needs_k64 = family in ("bf16", "f16", "x2w") and r.BK % 64 != 0
        if tuned4:
            out.append(_lin(1, 36, 1, r, tune, "M = 1: every staged row clamped, one k-tile (N = 36: smaller N leaves the row)"))
        elif small_needs_k64:
            if not odd:
                out.append(_lin(1, 4, 2, r, tune, "M = 1, N = 4 (two k-tiles: N <= 32 needs Cin % 64 == 0)"))
            out.append(_lin(1, 36, 1, r, tune, "M = 1, one k-tile (N = 36: N <= 32 needs Cin % 64 == 0)"))
        else:
            out.append(_lin(1, 4, 1, r, tune, "M = 1, N = 4: every staged row clamped, one k-tile"))
        ns = (32, 28, 20) if n32 else (r.BN + 4, r.BN - 4, r.BN + r.BN // 2)
        shapes = [(r.BM + 1, ns[0], kt(max(1, r.NS - 1)), "prologue fills the ring; last tiles hold one row / four columns"),
                  (r.BM - 1, ns[1], kt(r.NS), "first steady-state stage"),
                  (2 * r.BM + 17, ns[2], kt(2 * r.NS + 1), "every ring slot reused twice")]
        seen = {(c.M, c.N, c.Cin) for c in out}
        for M, N, nk, what in shapes:
            if (M, N, nk * r.BK) not in seen:
                seen.add((M, N, nk * r.BK))
                out.append(_lin(M, N, nk, r, tune, what))
        cout = 20 if n32 else r.BN + 4
        for B, H, W in ((2, 5, 7), (3, 9, 11)):
            for kpt in (1, 3 if odd else 2):
                out.append(_conv(B, H, W, kpt * r.BK, cout, tune, f"3x3 conv {B}x{H}x{W}, kpt {kpt}"))
    if r.sk != "no":
        for S in (2, 4, 6):
            out.append(_lin(r.BM + 1, r.BN + 4, 6, r, tune, f"split-K {S} of 6 k-tiles, eager", S, 0))
            out.append(_lin(r.BM + 1, r.BN + 4, 6, r, tune, f"split-K {S} of 6 k-tiles, deferred", S, 1))
        out.append(_conv(2, 5, 7, r.BK, r.BN + 4, tune, "split-K 4 of 9 k-tiles, 3x3 conv", 4))
    return out


def precondition_errors(family, key, c: Case):
    """The launcher preconditions a case violates (none, for a generated one), and the conditions under which it would run another row."""
    r = TABLE[family][key]
    bad = []
    K = c.taps * c.Cin
    nk = K // r.BK
    if c.N % 4: bad.append("N % 4")
    if c.Cin % 32: bad.append("Cin % 32")
    if c.Cin % r.cin_div: bad.append(f"Cin % {r.cin_div}")
    if c.taps == 9 and c.M != c.B * c.H * c.W: bad.append("conv geometry")
    if c.taps == 1 and (c.ldx < c.Cin or c.ldx * ELEM_BYTES[family] % 16): bad.append("ldx")
    if family == "x3" and c.ldx % 16: bad.append("x3 ldx % 16")
    if c.splitk > nk: bad.append("splits > nk")
    if c.splitk > 1 and r.sk == "no": bad.append("no split-K form")
    if c.splitk <= 1 and r.sk == "only": bad.append("split-K only")
    if family in ("bf16", "f16", "x2w") and c.N <= 32 and c.Cin % 64: bad.append("N <= 32 needs Cin % 64 == 0")
    if family == "x2w" and (c.Cin % 64 == 0) != (key != 4): bad.append("x2w: Cin % 64 selects another tile")
    if family == "x2w" and c.splitk > 1: bad.append("x2w has no split-K")
    b128 = -(-c.M // 128) * -(-c.N // 128)
    if family in ("x3", "f32") and c.splitk <= 1:
        if c.N <= 32 and key not in ("n32", 2): bad.append("N <= 32 selects the 128 x 32 tile")
        if c.N > 32 and key == "n32": bad.append("N > 32 leaves the N <= 32 tile")
        if family == "f32" and key != "n32" and (b128 >= 384) != (key == 3): bad.append("f32 tile is chosen by the grid")
    if c.sk_defer and c.splitk <= 1: bad.append("deferred without splits")
    return bad


# ---------------------------------------------------------------------------------------------------------------------------------
# data: float64 tensors holding exactly the values the kernel reads
# ---------------------------------------------------------------------------------------------------------------------------------
def x3_roundtrip(t):
    from soccdpt_amd.lib import x3_decode, x3_encode
    return x3_decode(x3_encode(t.float()), t.shape)


def _as_read(t, fmt):
    """f32 values -> what an operand of format fmt holds, as float64."""
    if fmt in ("bf16", "f16"):
        return R.round16(t.double(), fmt)
    if fmt == "x3":
        return x3_roundtrip(t)
    return t.float().double()


def device_operand(src, fmt, dev):
    """The f32 source of an operand -> the tensor a launch of format fmt reads (the counterpart of _as_read)."""
    if fmt in ("bf16", "f16"):
        return src.to(R.DT16[fmt]).to(dev)
    if fmt == "x3":
        from soccdpt_amd.lib import x3_encode
        return x3_encode(src.float()).to(dev)
    return src.float().to(dev)


def x_fmt(family):
    return "f16" if family == "x2w" else family


def w_fmt(family):
    return "x3" if family == "x2w" else family


def draw_values(g, dataset, shape, mag=4):
    """The two data sets (module docstring): "exact" -- nonzero integers of magnitude <= mag; "real" -- randn with a power-of-two scale per row."""
    if dataset == "exact":
        v = torch.randint(1, mag + 1, shape, generator=g).float()
        return v * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    scale = 2.0 ** torch.randint(-3, 4, (shape[0],) + (1,) * (len(shape) - 1), generator=g).float()
    return torch.randn(shape, generator=g) * scale


def make_data(c: Case, family, dataset, seed=0):
    """dict(X | xh, Wt, bias, res1) of float64 CPU tensors.  Linear: X is [M][ldx] with NaN in the 16 padding columns; conv: xh is the zero-halo NHWC image.
    X_src / Wt_src: the f32 tensors the operands were rounded or encoded from (device_operand makes the launch's operand from them the same way)."""
    g = torch.Generator().manual_seed(seed * 7919 + c.M * 31 + c.N * 17 + c.Cin + (1 if dataset == "real" else 0))
    K = c.taps * c.Cin
    draw = lambda *shape: draw_values(g, dataset, shape)
    d = {}
    if c.kind == "linear":
        x = torch.full((c.M, c.ldx), float("nan"))
        x[:, :K] = draw(c.M, K)
        d["X"], d["X_src"] = _as_read(x, x_fmt(family)), x
        assert bool(d["X"][:, K:].isnan().all())
    else:
        x = torch.zeros(c.B, c.H + 2, c.W + 2, c.Cin)
        x[:, 1:-1, 1:-1] = draw(c.B * c.H * c.W, c.Cin).reshape(c.B, c.H, c.W, c.Cin)
        d["xh"], d["X_src"] = _as_read(x, x_fmt(family)), x
    d["Wt_src"] = draw(c.N, K)
    d["Wt"] = _as_read(d["Wt_src"], w_fmt(family))
    if dataset == "exact":
        d["bias"] = torch.randint(-4, 5, (c.N,), generator=g).double()
        d["res1"] = torch.randint(-4, 5, (c.M, c.N), generator=g).double()
    else:
        d["bias"] = torch.randn(c.N, generator=g).double()
        d["res1"] = torch.randn(c.M, c.N, generator=g).double()
    if c.sk_defer:   # the deferred form writes the bare product
        d["bias"], d["res1"] = torch.zeros(c.N, dtype=torch.float64), torch.zeros(c.M, c.N, dtype=torch.float64)
    return d


def im2col(xh, c: Case, swap_taps=False):
    """[M][9 Cin] rows (tap-major, tap = 3 ky + kx) of every output pixel; swap_taps walks (kx, ky) instead (a planted fault)."""
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    if swap_taps:
        taps = [(kx, ky) for ky, kx in taps]
    # a swapped walk reads ky * Wp + kx with the roles exchanged: the pixel (y + kx, x + ky) -- possible only inside the halo image
    Hp, Wp = c.H + 2, c.W + 2
    flat = xh.reshape(c.B, Hp * Wp, c.Cin)
    y = torch.arange(c.H, device=xh.device)[:, None]
    x = torch.arange(c.W, device=xh.device)[None, :]
    cols = []
    for ky, kx in taps:
        idx = ((y + ky) * Wp + (x + kx)).reshape(-1)
        cols.append(flat[:, idx])
    return torch.cat(cols, dim=2).reshape(c.M, 9 * c.Cin)


def split_ranges(nk, S, BK):
    """Element ranges [lo, hi) of the K axis that split s of S accumulates (igemm_kernel.h: kbase = s nk / S)."""
    return [((s * nk // S) * BK, ((s + 1) * nk // S) * BK) for s in range(S)]


def reference(c: Case, family, key, d, dev="cpu"):
    """dict: cols [M][K], Wt, v = acc + bias + res1 (float64, before the activation), bound, partials (the S split-K partial products), all on dev."""
    r = TABLE[family][key]
    K = c.taps * c.Cin
    Wt = d["Wt"].to(dev)
    cols = d["X"][:, :K].to(dev) if c.kind == "linear" else im2col(d["xh"].to(dev), c)
    bias, res1 = d["bias"].to(dev), d["res1"].to(dev)
    S = max(1, c.splitk)
    parts = [cols[:, lo:hi] @ Wt[:, lo:hi].t() for lo, hi in split_ranges(K // r.BK, S, r.BK)]
    acc = parts[0].clone()
    for p in parts[1:]:
        acc += p
    mag = cols.abs() @ Wt.abs().t()
    bound = R.gemm_gamma(family, K, r.MF) * mag + R.gamma(2) * (acc.abs() + bias.abs() + res1.abs())
    if S > 1:
        bound = bound + R.gamma(S - 1) * sum(p.abs() for p in parts)
    return dict(cols=cols, Wt=Wt, v=acc + bias + res1, bound=bound, parts=parts, bias=bias, res1=res1)


# ---------------------------------------------------------------------------------------------------------------------------------
# checks on what a launch wrote
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def guarded(nbytes, dev):
    """(whole, payload): a 0xFF-filled byte buffer with GUARD bytes either side of `nbytes` payload bytes."""
    whole = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + nbytes]


def check_guards(whole, what):
    n = whole.numel()
    if not (bool((whole[:GUARD] == 0xFF).all()) and bool((whole[n - GUARD:] == 0xFF).all())):
        raise AssertionError(f"{what}: a guard region beside the buffer was written")


def check_out(c: Case, dataset, ref, out_f32, what):
    """out_f32 [M][N] against the reference: bitwise for the exact data set, element-wise within the bound otherwise.  Returns the worst error / bound."""
    got = out_f32.detach().cpu()
    v = ref["v"].cpu()
    if dataset == "exact":
        exp = v.float()
        assert bool((exp.double() == v).all()), "the exact data set left the integers of f32"
        same = (got.view(torch.int32) == exp.view(torch.int32)) | ((got == 0) & (exp == 0))
        if not bool(same.all()):
            t = tuple((~same).nonzero()[0].tolist())
            raise AssertionError(f"{what}: {int((~same).sum())} of {same.numel()} elements differ from the exact result; first at {t}: got {float(got[t])!r}, "
                                 f"expected {float(exp[t])!r}")
        return 0.0
    return R.check_bound(got, v, ref["bound"].cpu(), what)


def check_copy(c: Case, family, out_f32, copy, what):
    """The haloed operand copy [B][H+2][W+2][N] (as raw storage of its element type) against the launch's own f32 output: interior = RN16(relu(out_f32))
    bitwise (f32 launches copy relu(out_f32) itself), ring untouched (still 0xFF bytes)."""
    got = copy.detach().cpu().reshape(c.B, c.H + 2, c.W + 2, c.N)
    a = out_f32.detach().cpu().float().clamp(min=0).reshape(c.B, c.H, c.W, c.N)
    ring = torch.ones(c.H + 2, c.W + 2, dtype=torch.bool)
    ring[1:-1, 1:-1] = False
    raw = got.view(torch.uint8).reshape(c.B, c.H + 2, c.W + 2, -1)
    if not bool((raw[:, ring] == 0xFF).all()):
        raise AssertionError(f"{what}: the halo ring of the operand copy was written")
    inner = got[:, 1:-1, 1:-1]
    if family == "f32":
        same = (inner.view(torch.int32) == a.view(torch.int32)) | ((inner == 0) & (a == 0))
        if not bool(same.all()):
            raise AssertionError(f"{what}: {int((~same).sum())} words of the f32 copy differ from relu(out_f32)")
    else:
        R.check_copy16(inner, a, "bf16" if family == "bf16" else "f16", what)


def copy_dtype(family):
    return {"bf16": torch.bfloat16, "f32": torch.float32}.get(family, torch.float16)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU emulation with planted faults (tests/test_igemm_refs.py)
# ---------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("skip_last_ktile", "stale_slot", "swap_chunks", "clamped_neighbour", "cols_not_stored", "tap_swap", "read_past_k", "split_missing")


def fault_applies(fault, c: Case, family, key):
    r = TABLE[family][key]
    nk = c.taps * c.Cin // r.BK
    S = max(1, c.splitk)
    return {"skip_last_ktile": True,
            "stale_slot": S == 1 and nk > r.NS,
            "swap_chunks": True,
            "clamped_neighbour": c.M >= 2,
            "cols_not_stored": True,
            "tap_swap": c.kind == "conv",
            "read_past_k": c.kind == "linear",
            "split_missing": S > 1}[fault]


def emulate(c: Case, family, key, d, ref, fault=None):
    """What an exact-arithmetic kernel would leave in out_f32 (rounded to f32), with one fault planted.  Returns (out_f32, changed): changed says whether
    the fault moved any value of the float64 result (the self-test asserts it, so that no fault hides behind operands that happen to cancel)."""
    r = TABLE[family][key]
    cols, Wt, v = ref["cols"], ref["Wt"], ref["v"].clone()
    K, BK = c.taps * c.Cin, r.BK
    nk = K // BK
    if fault == "skip_last_ktile":
        v -= cols[:, K - BK:] @ Wt[:, K - BK:].t()
    elif fault == "stale_slot":      # k-tile nk - 1 served from ring slot contents NS tiles old
        a, b = (nk - 1) * BK, (nk - 1 - r.NS) * BK
        v += cols[:, b:b + BK] @ Wt[:, b:b + BK].t() - cols[:, a:a + BK] @ Wt[:, a:a + BK].t()
    elif fault == "swap_chunks":     # the first two 16-byte pieces of weight row 0 exchanged
        e = CHUNK_ELEMS[w_fmt(family)]
        w0 = Wt[0, :2 * e]
        assert bool((w0 != 0).all()) and bool((w0[:e] != w0[e:]).any()), "planted position holds no distinguishable operands"
        sw = torch.cat([w0[e:], w0[:e]])
        v[:, 0] += cols[:, :2 * e] @ (sw - w0)
    elif fault == "clamped_neighbour":
        assert bool((cols[c.M - 2] != cols[c.M - 1]).any())
        v[c.M - 1] = cols[c.M - 2] @ Wt.t() + ref["bias"] + ref["res1"][c.M - 1]
    elif fault == "tap_swap":
        v = im2col(d["xh"].to(cols.device), c, swap_taps=True) @ Wt.t() + ref["bias"] + ref["res1"]
    elif fault == "read_past_k":     # element K - 1 of row 0 taken one element further on: the first padding column
        past = d["X"][0, K].to(cols.device)
        assert bool(Wt[:, K - 1].ne(0).all())
        v[0] += (past - cols[0, K - 1]) * Wt[:, K - 1]
    elif fault == "split_missing":
        v -= ref["parts"][1]
    out = v.float()
    if fault == "cols_not_stored":
        out[:, c.N - 4:] = float("nan")
    changed = fault == "cols_not_stored" or not bool((v == ref["v"]).all())   # NaN counts as changed
    return out, changed


def torch_f32(c: Case, d):
    """The same launch with torch's f32 matmul / conv2d on the CPU (the operands are exact in f32)."""
    K = c.taps * c.Cin
    if c.kind == "linear":
        acc = d["X"][:, :K].float() @ d["Wt"].float().t()
    else:
        x = d["xh"][:, 1:-1, 1:-1].float().permute(0, 3, 1, 2)
        w = d["Wt"].float().reshape(c.N, 3, 3, c.Cin).permute(0, 3, 1, 2)
        acc = F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(c.M, c.N)
    return acc + d["bias"].float() + d["res1"].float()
