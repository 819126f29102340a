"""CPU: the selection core of soccdpt_prec_calibrate (soccdpt_amd/csrc/calib_select.cpp) without a GPU.

tests/calib_select_main.cpp links only the core, is built here with the host compiler under the address and undefined-behaviour sanitizers and run as
a child process.  Its measure callback is a synthetic additive error model (per group and quantity a variance in fp16, a smaller one as x2w, none in
x3, over a floor; hold-out errors 1.05 x the calibration errors) with a non-additivity factor and a call that can be made to fail, so the paths the
GPU tests cannot reach -- tightened attempts, the fall-back after six of them, a failure in the middle -- are reached here.  Every scenario prints
the maps it handed to measure, in order ('0' fp16, '1' x2w, '2' x3 per group, 'p' appended when the per-pixel figures were asked for)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUDGET, HEADROOM = 5e-4, 0.85


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or "/opt/rocm/llvm/bin/clang++"
    out = str(tmp_path_factory.mktemp("calib_select") / "calib_select_main")
    src = [os.path.join(REPO, "tests", "calib_select_main.cpp"), os.path.join(REPO, "soccdpt_amd", "csrc", "calib_select.cpp")]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *src, "-o", out]
    # gcc links the sanitizer runtimes as shared libraries unless told otherwise; linked into the program they need nothing from the loader.  Where the
    # static archives are not installed, the default link does
    is_clang = "clang" in subprocess.run([cxx, "--version"], capture_output=True, text=True, check=True).stdout
    if is_clang or subprocess.run([*cmd, "-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr     # a sanitizer report goes to stderr and ends the program with a non-zero status
    return json.loads(r.stdout)


def _select(exe, **kw):
    return _run(exe, "select", *[f"{k}={v}" for k, v in kw.items()])


def _n_first_candidate(d):
    """calls before the first candidate: all-x3, all-fp16, shipped, then per group one-out in fp16 and, where it may, in x2w"""
    return 3 + d["G"] + d["x2w_ok"].count("1")


def _check_prefix(d):
    """the fixed part of the sequence, map for map"""
    G, ok, calls = d["G"], d["x2w_ok"], d["calls"]
    want = ["2" * G + "p", "0" * G + "p", d["shipped"]]
    for i in range(G):
        want.append("2" * i + "0" + "2" * (G - i - 1))
        if ok[i] == "1":
            want.append("2" * i + "1" + "2" * (G - i - 1))
    assert calls[:len(want)] == want
    assert len(want) == _n_first_candidate(d)


def _check_accepted(d):
    assert d["rc"] == 0
    assert d["final_worst"] <= HEADROOM * BUDGET and d["final_holdout"] <= BUDGET
    assert all(s != "1" or o == "1" for call in d["calls"] for s, o in zip(call, d["x2w_ok"]))     # no group that cannot take x2w is ever asked to
    assert d["calls"][-1] == d["chosen"] + "p"      # the last measured run is the chosen map: what the handle stays prepared for
    assert d["worst_x3"] < HEADROOM * BUDGET < d["worst_f16"]


@pytest.mark.parametrize("G,seed", [(12, 4), (66, 1)])
def test_additive_model(exe, G, seed):
    d = _select(exe, G=G, seed=seed)
    _check_prefix(d)
    _check_accepted(d)
    n0 = _n_first_candidate(d)
    cand = d["calls"][n0]
    print(f"G = {G}: {len(d['calls'])} calls, candidate {cand}, chosen {d['chosen']}, worst {d['final_worst']:.3e}, cost {d['cost_chosen']:.1f} us (all x3: {d['cost_shipped']:.1f})")
    assert n0 + 2 <= len(d["calls"]) <= n0 + 2 + 5 + sum(c != "0" for c in cand)
    assert d["shipped"] == "2" * G and d["cost_chosen"] < d["cost_shipped"]      # an all-x3 shipped map passes the rule but costs more: not chosen
    assert "1" in d["chosen"] and "0" in d["chosen"]


def test_no_group_may_take_x2w_is_the_two_format_selection(exe):
    d = _select(exe, G=12, seed=4, no_x2w=1)
    _check_prefix(d)
    _check_accepted(d)
    assert d["x2w_ok"] == "0" * 12 and _n_first_candidate(d) == 3 + 12
    assert not any("1" in call for call in d["calls"]) and "1" not in d["chosen"]
    assert len(d["calls"]) >= 3 + 12 + 2


@pytest.mark.parametrize("G,seed", [(12, 4), (66, 1)])
def test_optimistic_prediction_is_tightened(exe, G, seed):
    """errors 1.15 x what the additive model predicts as soon as two groups are below x3: the first candidate misses, a tightened one is accepted"""
    base = _select(exe, G=G, seed=seed)
    d = _select(exe, G=G, seed=seed, factor=1.15)
    _check_prefix(d)
    _check_accepted(d)
    assert len(d["calls"]) > len(base["calls"])
    assert d["cost_chosen"] >= base["cost_chosen"]


@pytest.mark.parametrize("G,seed", [(12, 4), (66, 1)])
def test_six_failed_attempts_fall_back_to_pruning_all_x3(exe, G, seed):
    """errors 3 x the prediction: 0.97 x 0.9^5 of the target is still not enough, so the selection starts again from every group in x3 and keeps the
    single-level demotions that measure under the target"""
    d = _select(exe, G=G, seed=seed, factor=3)
    _check_prefix(d)
    _check_accepted(d)
    n0 = _n_first_candidate(d)
    assert len(d["calls"]) == n0 + 6 + G + 1        # six candidates, one demotion tried per group (every saving is above 1 us), the final run
    first_demotion = d["calls"][n0 + 6]
    assert sorted(first_demotion) == sorted("2" * (G - 1) + ("1" if "1" in first_demotion else "0"))
    assert d["chosen"] != "2" * G and d["chosen"].count("2") >= G - 2


def test_floor_above_the_target_selects_nothing(exe):
    d = _select(exe, G=12, seed=4, floor=4.5e-4)
    assert d["rc"] == 0 and d["worst_x3"] > HEADROOM * BUDGET
    assert d["calls"] == ["2" * 12 + "p", "0" * 12 + "p", d["shipped"], "2" * 12 + "p"]
    assert d["chosen"] == "2" * 12


def test_shipped_map_wins_at_no_higher_cost(exe):
    """the cheapest map the model accepts (exhaustive search in the driver) as the shipped map: the greedy result on this draw costs more, so the
    shipped map is the one chosen"""
    greedy = _select(exe, G=12, seed=4)
    d = _select(exe, G=12, seed=4, shipped="best")
    _check_prefix(d)
    _check_accepted(d)
    assert d["calls"][:-1] == greedy["calls"][:2] + [d["shipped"]] + greedy["calls"][3:-1]     # the same selection up to the last rule
    assert d["shipped"] != greedy["chosen"] and d["cost_shipped"] <= greedy["cost_chosen"] and d["worst_shipped"] <= HEADROOM * BUDGET
    assert d["chosen"] == d["shipped"]


@pytest.mark.parametrize("k", [0, 9])
def test_failing_measure_ends_the_selection_at_once(exe, k):
    """k = 9 is inside the one-group-out loop (calls 3 .. 3 + G + n_ok - 1)"""
    d = _select(exe, G=12, seed=4, fail_at=k)
    assert 3 <= 9 < _n_first_candidate(d)
    assert d["rc"] != 0 and len(d["calls"]) == k + 1


def _per_pixel_numpy(ref, got):
    n = ref.size
    if n == 0:
        return 0.0, 0.0
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), np.float32(1e-6))
    assert e.dtype == np.float32
    e = np.sort(np.where(np.isnan(e), np.float32(3.0e38), e))
    k = min(n - 1, max(0, int(0.999 * n) - 1))
    return float(e[k]), float(e[-1])


@pytest.mark.parametrize("case", ["n0", "n1", "n2000", "nan", "ref0"])
def test_per_pixel_equals_numpy(exe, tmp_path, case):
    rng = np.random.default_rng(7)
    n = {"n0": 0, "n1": 1}.get(case, 2000)
    ref = (rng.standard_normal(n) * 0.3 + 1.0).astype(np.float32)
    got = (ref * (1.0 + 1e-3 * rng.standard_normal(n))).astype(np.float32)
    if case == "nan":
        got[1234] = np.nan
    if case == "ref0":
        ref[::97] = 0.0         # the 1e-6 floor of the denominator
        ref[5] = np.float32(3e-7)
    path = tmp_path / "pixels.f32"
    with open(path, "wb") as f:
        f.write(ref.tobytes())
        f.write(got.tobytes())
    d = _run(exe, "pixels", str(path), str(n))
    p999, pmax = _per_pixel_numpy(ref, got)
    assert (d["p999"], d["pmax"]) == (p999, pmax)
    if case == "nan":
        assert pmax == float(np.float32(3.0e38)) and p999 < 1.0
    if case == "ref0":
        assert pmax > 1.0e3
