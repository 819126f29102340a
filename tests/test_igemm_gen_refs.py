"""CPU: tests/igemm_gen_refs.py against the launcher's source text and against itself.

* the instantiations with ST or GEN that launch_igemm names are the table's Forms plus the listed unreachable ones, with the table's tile geometry, and
  every routing statement the case generator restates still stands in the source;
* every generated case satisfies the Python restatement of launch_igemm's preconditions and reaches the row and instantiation it was generated for, and
  every Form of every row has a case;
* a CPU emulation that addresses the flat operand storage as igemm_kernel.h does, accumulates in f32 in the kernel's order and lays the statistics
  partials out as the epilogue does passes every check of every case of every row; with one fault planted -- H and W exchanged in the input pitch, the
  pitch taken from the output width, the stride on one axis only, in_halo - pad dropped, grp_off dropped, the group taken as m / BM, the second segment
  one k-tile late; a partial stored with the n-tile's group count as pitch, the groups of a ragged n-tile beyond N stored, a wave row left out, the
  squares without a group's last channel -- every addressing fault is rejected by every case where it can occur, every statistics fault by every such
  case's exact data set and by at least one case of the row (under the real data set a channel of small scale can hide inside the a-priori bound), and
  every fault occurs in every family.
"""
import os

import pytest
import torch

from tests import igemm_gen_refs as T
from tests import igemm_refs as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(name="igemm.hip"):
    return open(os.path.join(REPO, "soccdpt_amd", "csrc", name)).read()


def test_table_is_the_set_of_instantiations_in_the_source():
    src, tab = T.parse_instantiations(_source()), T.table_instantiations()
    assert src == tab, ("in the source, not in the table", sorted(map(str, src - tab)), "in the table, not in the source", sorted(map(str, tab - src)))
    assert T.GTABLE["f16"] is T.GTABLE["bf16"]
    for key in T.UNREACHABLE:
        assert key[1] in T.GTABLE[key[0]] and not any((f.st, f.gen, f.sk) == key[2:] for f in T.GTABLE[key[0]][key[1]])


def test_an_instantiation_without_a_form_is_noticed():
    src = _source().replace("case 5: return launch_cfg_t<Cfg<128, 128, 64, 2, 4, 3>, x3_t>(d, stream, err);",
                            "case 5: return launch_cfg_t<Cfg<128, 128, 64, 2, 4, 3>, x3_t, false, false, true, false>(d, stream, err);")
    assert ("x3", 5, True, False, False, (128, 128, 32, 2, 4, 3, 16)) in T.parse_instantiations(src) - T.table_instantiations()
    src = _source().replace("case 0: return launch_cfg<Cfg<128, 128, 64, 2, 2, 4>>", "case 0: return launch_cfg_st<Cfg<128, 128, 64, 2, 2, 4>>")
    assert {k[:5] for k in T.parse_instantiations(src) - T.table_instantiations()} == {("16", 0, True, False, False), ("16", 0, True, True, False)}


def test_routing_rules_the_generator_restates_stand_in_the_source():
    flat = " ".join((_source() + _source("hybrid.hip") + _source("capi.cpp")).split())
    for what, line in list(T.ROUTING_LINES.items()) + [("gn_finish", T.FINISH_LINE), ("op_igemm", T.CAPI_LINE)] + [(str(k), v) for k, v in T.UNREACHABLE.items()]:
        assert " ".join(line.split()) in flat, f"the source no longer holds the rule the case generator relies on: {what}: `{line}`"


def test_unreachable_instantiations_are_unreachable_by_the_restated_routing():
    """x3 statistics + generalised addressing on tiles 3 and 7: whatever tune, shape and group width, the restated pick_cfg_f32 never returns them."""
    for tune in range(-1, 13):
        for hw, cpg, N, B in ((64, 2, 64, 2), (128, 8, 128, 2), (128, 128, 128, 2), (8192, 128, 128, 4), (8192, 64, 256, 8), (4096, 32, 512, 16)):
            h, w = (64, 128) if hw == 8192 else ((64, 64) if hw == 4096 else T.MAPS[hw])
            c = T._gather_s2("", B, h, w, 32, N, cpg=cpg, hw=hw, epi=False, tune=tune)
            assert T.x3_pick(c) in (0, 1, 4, 12), (tune, hw, cpg, T.x3_pick(c))
            c = T._same_s2("", B, h, w, 32, N, cpg=cpg, hw=hw, epi=False, tune=tune)
            assert T.x3_pick(c) in (0, 1, 4, 12)


@pytest.mark.parametrize("fk", T.configs(), ids=G.config_id)
def test_cases_satisfy_the_launcher_preconditions(fk):
    family, key = fk
    cs = T.cases(family, key)
    assert cs and len({c.name for c in cs}) == len(cs), "duplicate case names"
    for c in cs:
        assert T.precondition_errors(family, key, c) == [], c
        assert ("real only" in c.name) == (c.datasets == ("real",))
        assert c.kind == "linear" or (c.H != c.W and (c.Hi or c.H) != (c.Wi or c.W)), "everything is non-square"
    hit = {T.instantiation(family, key, c) for c in cs}
    assert hit == {(f.st, f.gen, f.sk) for f in T.GTABLE[family][key]}, "a Form of the row has no case"
    forms = T.GTABLE[family][key]
    r = T.row(family, key)
    if any(f.gen and not f.st and not f.sk for f in forms):
        names = " | ".join(c.name for c in cs)
        for what in ("same_s2", "pad1_s2", "gather_s2, 1 k-tile", "s1_gen", "groups", "readout, seg2_k 128 of 256", "readout, seg2_k 256 of 384"):
            assert what in names, what
        nks = {c.K // r.BK for c in cs if c.grp_rows and not c.seg2_k and c.splitk == 1}
        assert nks == {max(1, r.NS - 1), 2 * r.NS + 1}
    if any(f.gen and f.sk for f in forms):
        assert any(c.splitk == 2 and c.grp_rows for c in cs)
    for f in forms:
        if f.st and not f.big:
            mine = [c for c in cs if c.st and T.instantiation(family, key, c) == (f.st, f.gen, f.sk)]
            assert {c.hw for c in mine} == {r.BM, 2 * r.BM} and all(c.M == 2 * c.hw for c in mine)
            cpgs = {c.cpg for c in mine}
            assert 2 in cpgs and r.BN in cpgs and cpgs & set(T.MID_CPG)
            assert any(c.N == r.BN + r.BN // 2 for c in mine) and any(c.dc for c in mine) and any(c.count for c in mine) and any("exact" in c.datasets for c in mine)


def test_a_moved_precondition_is_noticed():
    c = T.cases("bf16", 2)[0]
    from dataclasses import replace
    assert T.precondition_errors("bf16", 2, replace(c, Hi=8)) == ["taps leave the input image"]
    assert "row 3 has no instantiation (False, True, False)" in T.precondition_errors("x3", 3, replace(c, tune=3))[0]
    g = next(c for c in T.cases("x3", 1) if c.seg2_k)
    assert "second segment" in T.precondition_errors("x3", 1, replace(g, seg2_k=64))
    assert "x3: multiples of 16 elements" in T.precondition_errors("x3", 1, replace(g, grp_off=g.grp_off + 8))
    s = next(c for c in T.cases("f16", 23) if c.st)
    assert "statistics descriptor" in T.precondition_errors("f16", 23, replace(s, hw=s.hw // 2))
    assert "statistics descriptor" in T.precondition_errors("f16", 23, replace(s, cpg=3))


def _run_checks(family, key, c, dataset, d, ref, out, part, what):
    """Every check the GPU test applies to a launch's out_f32 and partials."""
    r = T.row(family, key)
    G.check_out(c.plain(), dataset, ref, out, what)
    if c.st:
        T.check_part(c, r, dataset, out, part, what)


@pytest.mark.parametrize("fk", T.configs(), ids=G.config_id)
def test_emulation_passes_and_planted_faults_are_rejected(fk):
    family, key = fk
    r = T.row(family, key)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    applied, caught = set(), set()
    for c in T.cases(family, key):
        for dataset in c.datasets:
            d = T.make_data(c, family, dataset)
            ref = T.reference(c, family, key, d)
            what = f"{family}-{key} {c.name} [{dataset}]"
            out, changed = T.emulate_out(c, family, key, d)
            assert not changed
            part = T.emulate_part(c, r, out) if c.st else None
            _run_checks(family, key, c, dataset, d, ref, out, part, what)
            if c.dc:
                T.check_dc(c, out)
            if c.count:
                T.check_stats(c, r, out, part, T.emulate_stats(c, r, part), what)
                off = T.emulate_stats(c, r, part)
                off[0, 0, 1] *= 1 + 2.0 ** -20
                with pytest.raises(AssertionError):
                    T.check_stats(c, r, out, part, off, what + " rstd off by 8 ulp")
            for fault in T.ADDR_FAULTS:
                if T.fault_applies(fault, c, r):
                    bad, changed = T.emulate_out(c, family, key, d, fault)
                    assert changed, (what, fault, "the planted fault moved no address")
                    with pytest.raises(AssertionError):
                        G.check_out(c.plain(), dataset, ref, bad, what + " " + fault)
            for fault in T.STAT_FAULTS:      # the exact data set must catch each; under the real one a channel of small scale may hide inside the a-priori bound
                if T.fault_applies(fault, c, r):
                    applied.add(fault)
                    try:
                        T.check_part(c, r, dataset, out, T.emulate_part(c, r, out, fault), what + " " + fault)
                    except AssertionError:
                        caught.add(fault)
                    else:
                        assert dataset == "real", (what, fault, "not caught by the exact data set")
    assert caught == applied, (family, key, "planted statistics faults no case caught", applied - caught)


def test_every_fault_occurs_somewhere_in_every_family():
    for family in G.FAMILIES:
        hit = set()
        for key in T.GTABLE[family]:
            r = T.row(family, key)
            for c in T.cases(family, key):
                hit |= {f for f in T.ADDR_FAULTS + T.STAT_FAULTS if T.fault_applies(f, c, r)}
        assert hit == set(T.ADDR_FAULTS + T.STAT_FAULTS), (family, set(T.ADDR_FAULTS + T.STAT_FAULTS) - hit)
