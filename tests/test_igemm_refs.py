"""CPU: tests/igemm_refs.py against the launcher's source text and against itself.

* the table's rows are the Cfg<> of the `case` labels of launch_igemm's switches, and no label lacks a row (a configuration added later fails here);
* every generated case satisfies the launcher's preconditions and lands on the row it was generated for;
* a CPU emulation of the launch with one fault planted -- a skipped k-tile, a stale ring slot, two exchanged 16-byte pieces, a clamped neighbour row, four
  columns not stored, a transposed tap walk, a read past K, a missing split-K partial -- is rejected by the checker at every generated shape where the
  fault can occur, in both data sets, and the unfaulted emulation passes;
* torch's own f32 matmul / conv2d of the same operands lies inside every bound.

The emulation depends on the tile geometry only, so rows of equal (BM, BN, BK, NS, MF, split-K form) share one run; bf16 and f16 alternate over them."""
import os

import pytest
import torch

from tests import igemm_refs as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source():
    return open(os.path.join(REPO, "soccdpt_amd", "csrc", "igemm.hip")).read()


def _geom(r):
    return (r.BM, r.BN, r.BK, r.WM, r.WN, r.NS, r.MF)


def test_table_agrees_with_the_launcher_source():
    p = G.parse_launcher(_source())
    for fam, tab in (("16", G.TABLE["bf16"]), ("x3", G.TABLE["x3"]), ("f32", G.TABLE["f32"]), ("x2w", G.TABLE["x2w"])):
        src = dict(p[fam])
        for k, why in G.NOT_ROWS[fam].items():
            assert k in src, (fam, k, "listed as no row, but the launcher has no such case")
            del src[k]
        assert set(src) == set(tab), (fam, "cases without a row", set(src) - set(tab), "rows without a case", set(tab) - set(src))
        for k, geom in src.items():
            assert _geom(tab[k]) == geom, (fam, k, _geom(tab[k]), geom)
    assert G.TABLE["f16"] is G.TABLE["bf16"]
    # the Cin divisibility the launcher demands per 16-bit id
    t16 = G.TABLE["bf16"]
    assert p["k64"] | p["k128"] <= set(t16)
    for k, r in t16.items():
        assert r.cin_div == r.BK
        assert (k in p["k128"]) == (r.cin_div == 128), k
        assert (k in p["k64"]) or r.cin_div != 64, k
        assert not (k in p["k64"] and r.cin_div == 32), k
    assert {k for k, r in t16.items() if r.sk == "also"} == p["sk_also"] and {k for k, r in t16.items() if r.sk == "only"} == p["sk_only"]


def test_routing_rules_the_generator_restates_stand_in_the_source():
    flat = " ".join(_source().split())
    for what, line in G.ROUTING_LINES.items():
        assert " ".join(line.split()) in flat, f"igemm.hip no longer holds the routing rule the case generator relies on: {what}: `{line}`"


def test_a_configuration_without_a_row_is_noticed():
    src = _source().replace("case 52: return launch_cfg<Cfg<128, 256, 64, 4, 4, 2>>", "case 52: return launch_cfg<Cfg<128, 256, 64, 4, 4, 2>>(d, stream, err);\n"
                            "        case 53: return launch_cfg<Cfg<64, 256, 64, 2, 4, 2>>")
    p = G.parse_launcher(src)
    assert 53 in p["16"] and 53 not in G.TABLE["bf16"]
    p = G.parse_launcher(_source().replace("case 12: return launch_cfg<Cfg<64, 64, 64, 2, 2, 8>>", "case 12: return launch_cfg<Cfg<64, 64, 64, 2, 2, 7>>"))
    assert p["16"][12] != _geom(G.TABLE["bf16"][12])


@pytest.mark.parametrize("fk", G.configs(), ids=G.config_id)
def test_cases_satisfy_the_launcher_preconditions(fk):
    family, key = fk
    r = G.TABLE[family][key]
    cs = G.cases(family, key)
    assert cs and len({(c.kind, c.M, c.N, c.Cin, c.B, c.splitk, c.sk_defer) for c in cs}) == len(cs), "duplicate cases"
    for c in cs:
        assert G.precondition_errors(family, key, c) == [], c
        assert (c.M <= 1100 and c.N <= 400 and c.taps * c.Cin <= 2400) or (family, key) == ("f32", 3)   # a launch and its float64 reference stay small
    if r.sk != "only" and (family, key) != ("f32", 3):
        nks = {c.Cin // r.BK for c in cs if c.kind == "linear" and c.splitk == 1}
        assert 2 * r.NS + 1 in nks or 2 * r.NS + 2 in nks
        assert any(n <= r.NS - 1 for n in nks) and any(c.M == 1 for c in cs)
        assert {(c.B, c.H, c.W) for c in cs if c.kind == "conv" and c.splitk == 1} == {(2, 5, 7), (3, 9, 11)}
    if r.sk != "no":
        assert {c.splitk for c in cs if c.splitk > 1 and c.kind == "linear"} == {2, 4, 6}
        assert any(c.sk_defer for c in cs)


def _geometry_classes():
    """One (family, key) per distinct (4-byte / 2-byte / x2w class, geometry that the emulation sees, split form); 16-bit classes alternate bf16 / f16."""
    seen, out = set(), []
    for family, key in G.configs():
        if family == "f16":
            continue
        r = G.TABLE[family][key]
        sig = (family, r.BM, r.BN, r.BK, r.NS, r.MF, r.sk, key == "n32", (family, key) == ("f32", 3))
        if sig in seen:
            continue
        seen.add(sig)
        if family == "bf16" and len(out) % 2:
            family = "f16"
        out.append((family, key))
    return out


@pytest.mark.parametrize("fk", _geometry_classes(), ids=G.config_id)
def test_planted_faults_are_rejected_and_torch_f32_is_inside_the_bounds(fk):
    family, key = fk
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for c in G.cases(family, key):
        for dataset in ("exact", "real"):
            d = G.make_data(c, family, dataset)
            ref = G.reference(c, family, key, d)
            what = f"{family}-{key} {c.what} [{dataset}]"
            clean, changed = G.emulate(c, family, key, d, ref)
            assert not changed
            G.check_out(c, dataset, ref, clean, what)
            G.check_out(c, dataset, ref, G.torch_f32(c, d), what + " torch f32")
            for fault in G.FAULTS:
                if not G.fault_applies(fault, c, family, key):
                    continue
                out, changed = G.emulate(c, family, key, d, ref, fault)
                assert changed, (what, fault, "the planted fault moved no value")
                with pytest.raises(AssertionError):
                    G.check_out(c, dataset, ref, out, what + " " + fault)


def test_every_fault_occurs_somewhere_in_every_family():
    for family in G.FAMILIES:
        hit = set()
        for key in G.TABLE[family]:
            for c in G.cases(family, key):
                hit |= {f for f in G.FAULTS if G.fault_applies(f, c, family, key)}
        assert hit == set(G.FAULTS) - ({"split_missing"} if family == "x2w" else set()), (family, set(G.FAULTS) - hit)


def test_copy_and_guard_checks_reject_what_they_should():
    c = G.Case("conv", 70, 8, 32, 9, 0, 2, 5, 7, -1, 1, 0, "")
    out = torch.randn(70, 8)
    for family in ("bf16", "f16", "f32", "x3", "x2w"):
        dt = G.copy_dtype(family)
        es = torch.empty((), dtype=dt).element_size()
        whole, payload = G.guarded(2 * 7 * 9 * 8 * es, "cpu")
        copy = payload.view(dt).reshape(2, 7, 9, 8)
        copy[:, 1:-1, 1:-1] = out.clamp(min=0).reshape(2, 5, 7, 8).to(dt)
        G.check_copy(c, family, out, copy, family)
        G.check_guards(whole, family)
        bad = copy.clone()
        bad[1, 0, 3, 2] = 0.0                      # a write into the ring
        with pytest.raises(AssertionError):
            G.check_copy(c, family, out, bad, family)
        bad = copy.clone()
        bad[0, 2, 2, 1] = out[9 * 0 + 7 + 1, 1].abs() * 1.01 + 1e-3   # not the rounding of the f32 value
        with pytest.raises(AssertionError):
            G.check_copy(c, family, out, bad, family)
        whole[G.GUARD - 1] = 0
        with pytest.raises(AssertionError):
            G.check_guards(whole, family)


def test_mfma32_bound_follows_the_stated_rule():
    from tests.fused_refs import gamma, gemm_gamma
    assert gemm_gamma("bf16", 64, 32) == gamma(5 * 4) and gemm_gamma("f16", 17, 32) == gamma(5 * 2)
    assert gemm_gamma("bf16", 64) == gamma(6 * 2)
    with pytest.raises(ValueError):
        gemm_gamma("x3", 64, 32)
