"""CPU: tests/gn_refs.py against itself -- no GPU, no built library.

* the launcher rules it restates stand in the text of csrc/hybrid.hip / csrc/capi.cpp, and the restated Python agrees with them on the case table;
* the case table reaches every (OUT, U) instantiation of gn_apply_kernel, every statistics mode, every tile count and projection pair of the thresholds;
* the data sets keep their promises (neighbouring groups and samples apart, the clamp decides, +-0 and tiny pre-ReLU values exist);
* an f32 emulation of the kernels (partial sums in f64, the rest in f32, the store formats) passes every bound at every case;
* every planted fault leaves a bound at one named case or more."""
import os

import pytest
import torch

from tests import gn_refs as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in T.CASES if c.B * c.HW * c.C < T.LARGE]
LARGE = [c for c in T.CASES if c.B * c.HW * c.C >= T.LARGE]


def _flat(*names):
    return " ".join(" ".join(open(os.path.join(REPO, "soccdpt_amd", "csrc", n)).read().split()) for n in names)


def test_restated_rules_stand_in_the_source():
    flat = _flat("hybrid.hip", "capi.cpp")
    for what, line in T.SRC.items():
        assert " ".join(line.split()) in flat, f"the source no longer holds the rule gn_refs restates: {what}: `{line}`"
    assert (T.K_DIRECT, T.K_COOP) == (12, 64)
    # a moved rule is noticed
    assert "tmax < kGnDirectTps" not in flat and T.SRC["mode"].replace("<=", "<") not in flat


def test_restated_rules_at_the_thresholds():
    assert [T.stats_mode(t, 0, False) for t in (0, 1, 12, 13, 64, 65, 144)] == [(0, False), (1, False), (1, False), (2, False), (2, False), (0, True), (0, True)]
    assert T.stats_mode(9, 36, True) == T.stats_mode(36, 9, True) == T.stats_mode(12, 13, True) == (2, False)
    assert T.stats_mode(64, 65, True) == T.stats_mode(65, 64, True) == (0, True) and T.stats_mode(12, 9, True) == (1, False)
    assert T.stats_mode(36, 0, False, groups=96) == (0, True)                  # a group count that does not divide 256 never shares the walk
    assert T.pixels_per_thread(2, 48 * 48, 1024) == 4 and T.pixels_per_thread(1, 48 * 48, 1024) == 2 and T.pixels_per_thread(3, 160, 64) == 1
    assert T.finish_gw(32, 9) == (32, None) and T.finish_gw(32, 65) == (16, None) and T.finish_gw(32, 144) == (4, None) and T.finish_gw(32, 577) == (1, None)
    assert T.finish_gw(1, 577) == (1, None)
    for G_, msg in T.FINISH_REFUSED.items():
        assert T.finish_gw(G_, 64)[1] == msg
    for tps in T.FINISH_TPS:
        for G_ in T.FINISH_G:
            gw, err = T.finish_gw(G_, tps)
            assert err is None and 256 % gw == 0 and G_ % gw == 0 and (gw == G_ or 256 // (2 * gw) < tps // 4)


def test_cases_are_legal_and_cover_the_table():
    assert len(T.CASE) == len(T.CASES)
    for c in T.CASES:
        assert c.C in (64, 128, 256, 512, 1024) and (c.HW * c.C // 4) % 256 == 0 and c.tps <= c.HW and c.tps2 <= c.HW, c
        assert T.apply_refusal(c.B, c.HW, c.W, c.C, c.cpg, c.tps, c.tps2, c.shortcut == "projection", c.shortcut == "identity") is None, c
        assert (c.shortcut == "projection" and c.tps > 0) == (c.tps2 > 0), c
    triples = {c.triple for c in T.CASES}
    assert {t[:2] for t in triples} == {(o, u) for o in range(4) for u in (1, 2, 4)}, "an (OUT, U) instantiation is never launched"
    assert {t[2] for t in triples} == {"0s", "0f", 1, 2}
    assert [c.name for c in T.CASES if c.triple[1] != 1] == [c.name for c in LARGE] and len(LARGE) == 8, "U = 4 and U = 2 once per format are the only large cases"
    plain = [c for c in T.CASES if c.shortcut != "projection"]
    assert {c.tps for c in plain} >= {1, 9, 12, 13, 36, 64, 65, 144}
    assert {(c.tps, c.tps2) for c in T.CASES if c.shortcut == "projection"} >= {(9, 36), (36, 9), (12, 13), (64, 65), (65, 64), (144, 144)}
    assert {c.shortcut for c in T.CASES} == {"none", "identity", "projection"} and {c.relu for c in T.CASES} == {0, 1} and {c.B for c in SMALL} >= {1, 3}
    assert {c.cpg for c in T.CASES} >= {2, 4, 8, 32} and {c.data for c in T.CASES} == {"a", "b", "c", "d"}
    assert {c.outs for c in T.CASES} >= {("f32",), ("op",), ("halo",), ("f32", "op"), ("f32", "op", "halo"), ("op", "halo")}
    assert {(c.fmt, c.halo_fmt) for c in T.CASES if c.halo_fmt is not None} == {(T.HF, T.X3), (T.HF, T.BF), (T.HF, T.F3), (T.BF, T.HF)}
    for m in (1, 2, "0f"):               # the clamp decides and cpg == 2 in every mode that adds partials up
        assert any(c.data == "c" and c.triple[2] == m and c.cpg == 2 for c in T.CASES), m


def test_tiles_are_uneven_and_partials_add_up():
    c = T.CASE["t13_c64_b3"]
    inp = T.build(c.name)
    assert int(inp["sizes"].sum()) == c.HW and int(inp["sizes"].min()) >= 1 and len(set(inp["sizes"].tolist())) > 1
    x = inp["raw"].double().reshape(c.B, c.HW, T.G, c.cpg)
    tot = inp["part"].double().reshape(c.B, c.tps, T.G, 2).sum(1)
    torch.testing.assert_close(tot[..., 0], x.sum((1, 3)), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(tot[..., 1], (x * x).sum((1, 3)), rtol=1e-6, atol=1e-6)


def test_data_sets_keep_their_promises():
    c = T.CASE["t13_c64_b3"]                                           # (a)
    st = T.stats_ref(T.build(c.name)["part"], c.B, c.tps, c.n)
    mean, sd = st["mean"].abs(), 1.0 / st["rstd"]
    for a, b in ((mean[:, 1:], mean[:, :-1]), (mean[1:], mean[:-1])):
        assert float(torch.minimum(a / b, b / a).max()) < 1 / 8, "neighbouring groups / samples differ by ~10x in mean"
    for a, b in ((sd[:, 1:], sd[:, :-1]), (sd[1:], sd[:-1])):
        assert float(torch.minimum(a / b, b / a).max()) < 1 / 3, "neighbouring groups / samples differ by ~4x in spread"
    c = T.CASE["t12_c64_b3_b"]                                         # (b)
    st = T.stats_ref(T.build(c.name)["part"], c.B, c.tps, c.n)
    assert float((st["mean"] * st["rstd"]).min()) > 20 and float((st["mean"] * st["rstd"]).max()) > 400
    for name in ("t9_c64_b3_c", "t13_c64_b3_c", "t144_c64_b1_c"):      # (c)
        c = T.CASE[name]
        p = T.build(name)["part"].double().reshape(c.B, c.tps, T.G, 2).sum(1) / c.n
        var = p[..., 1] - p[..., 0] ** 2
        assert bool((var[:, 0] == 0).all()) and bool((var[:, 1] < 0).all()) and bool((var[:, 1] > -2e-6).all()), "group 0 constant, group 1 below zero by an f32 ulp of mean^2"
    c = T.CASE["t12_c64_b3_norelu_d"]                                  # (d)
    inp = T.build(c.name)
    y = T.emulate(c, inp)["f32"].reshape(c.B, c.HW, c.C)[:, :3, ::3]
    assert bool((y[:, 0] == 0).all()) and bool((torch.signbit(y[:, 0])).any()) and bool((~torch.signbit(y[:, 0])).any()), "+0 and -0 before the ReLU"
    assert float(y[:, 1:].abs().max()) < 1e-4 and bool((y[:, 1:] > 0).any()) and bool((y[:, 1:] < 0).any())
    assert bool((inp["gamma"] == 0).any()) and bool((inp["gamma"] < 0).any())


@pytest.mark.parametrize("c", T.CASES, ids=lambda c: c.name)
def test_emulation_stays_inside_every_bound(c):
    inp = T.build(c.name)
    ratios = T.check_outputs(c, T.reference(c, inp), T.emulate(c, inp))
    print(f"{c.name}: worst error / bound {ratios}")
    assert ratios and max(ratios.values()) <= 1.0


def test_finish_emulation_stays_inside_its_bound():
    worst = 0.0
    for tps in T.FINISH_TPS:
        for G_ in T.FINISH_G:
            part, hw, cpg = T.build_finish(tps, G_)
            worst = max(worst, T.check_stats(T.emulate_stats(part, 2, tps, hw * cpg), T.stats_ref(part, 2, tps, hw * cpg), f"finish {tps} x {G_}"))
    print(f"gn_finish emulation: worst error / bound {worst:.3g}")
    assert 0 < worst <= 1.0


# fault -> the cases that must catch it (each is caught wherever it applies among the small cases; these are the named ones)
NAMED = {
    "s0_s1_swapped": ["t13_c64_b3", "t9_c64_b3_c", "p64_65_c64_b3", "s_c64_b3"],
    "sample0_statistics": ["t9_c1024_b3_id", "t65_c128_b3_op", "p12_13_c1024_b3", "s_c64_b3"],
    "last_tile_dropped": ["t1_c64_b1", "t13_c64_b3", "t144_c256_b3_id_all", "p9_36_c64_b3"],
    "clamped_tile_twice": ["t13_c64_b3", "t65_c128_b3_op", "t65_c64_b3_halo_x3", "p12_13_c1024_b3", "p64_65_c64_b3", "p65_64_c256_b1_d"],
    "clamp_omitted": ["t9_c64_b3_c", "t13_c64_b3_c", "t144_c64_b1_c", "p9_12_c128_b3_c"],
    "unbiased_variance": ["t1_c64_b1", "t12_c64_b3_norelu_d", "t13_c64_b3"],
    "eps_dropped": ["t9_c64_b3_c", "t13_c64_b3_c", "t144_c64_b1_c"],
    "gamma2_beta2_replaced": ["p9_36_c64_b3", "p36_9_c128_b1_norelu", "p64_65_c64_b3", "s_c512_b1_proj", "h_f16_f32_t65"],
    "part2_walked_with_tps": ["p9_36_c64_b3", "p36_9_c128_b1_norelu", "p12_13_c1024_b3", "p64_65_c64_b3", "p65_64_c256_b1_d", "p12_9_c64_b3"],
    "halo_off_by_one_pixel": ["t64_c128_b3_halo", "t65_c64_b3_halo_x3", "t144_c256_b3_id_all", "h_f16_x3_t9", "h_f16_bf16_t13", "h_f16_f32_t65", "h_bf16_f16_s"],
    "relu_skipped": ["t1_c64_b1", "t65_c128_b3_op", "t64_c128_b3_halo", "p9_36_c64_b3", "s_c64_b3"],
    "store16_truncated": ["t1_c64_b1", "t9_c1024_b3_id", "t64_c128_b3_halo", "t65_c128_b3_op", "h_f16_bf16_t13", "h_bf16_f16_s"],
}


@pytest.mark.parametrize("fault", T.FAULTS)
def test_planted_fault_is_caught_by_name(fault):
    assert set(NAMED) == set(T.FAULTS) and NAMED[fault]
    for name in NAMED[fault]:
        c = T.CASE[name]
        assert T.fault_applies(fault, c), (fault, name)
        inp = T.build(name)
        with pytest.raises(AssertionError):
            T.check_outputs(c, T.reference(c, inp), T.emulate(c, inp, fault))
