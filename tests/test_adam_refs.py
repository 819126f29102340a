"""CPU: the bounds of tests/adam_refs.py admit float32 evaluations of one Adam step (op by op like torch, with the kernel's fmas, with and without the two
contractions the compiler may add) at every case of the tables, and refuse each named defect on at least one case."""
import pytest
import torch

from tests import adam_refs as R


def _steps(h, step, n=R.HYPER_N, seed=1):
    """(inputs, Scalars, step) of a launch at `step` and of the one after it, which starts from what the first evaluation wrote."""
    inp = R.build(n, seed, step)
    return inp, R.scalars(h, step)


VARIANTS = [("kernel", True), ("kernel", False), ("plain", False), ("torch", False)]


def test_scalars_are_cast_once_from_float64():
    s = R.scalars(R.DEFAULT, 1)
    assert s.omb2 == R.f32(1.0 - 0.999) and s.omb2 != float(torch.tensor(1.0) - torch.tensor(0.999))
    assert abs(s.omb2 / float(torch.tensor(1.0) - torch.tensor(0.999)) - 1) > 1e-5      # the trap: 1.3e-5 relative
    assert s.ss == R.f32(1e-3 / (1 - 0.9)) and s.ibs == R.f32(1 / (1 - 0.999) ** 0.5)
    s = R.scalars(R.Hyper(1.0, 0.9, 0.0, 1e-3, 0.0), 100000)
    assert s.ibs == 1.0 and s.ss == 1.0 and s.b2 == 0.0 and s.omb2 == 1.0


@pytest.mark.parametrize("h", R.HYPERS, ids=lambda h: f"lr{h.lr}-b{h.b1}-{h.b2}-eps{h.eps}-wd{h.wd}")
def test_emulations_are_admitted(h):
    for step in R.STEPS:
        for style, contract in VARIANTS:
            inp, s = _steps(h, step)
            got = R.emulate(inp["p"], inp["g"], inp["m"], inp["v"], h, step, style, contract)
            R.check_step(got, inp, s, f"{style} contract {contract} step {step}")
            nxt = dict(got, g=R.build(R.HYPER_N, 2, step + 1)["g"])            # the next step starts from what this one wrote
            got2 = R.emulate(nxt["p"], nxt["g"], nxt["m"], nxt["v"], h, step + 1, style, contract)
            R.check_step(got2, nxt, R.scalars(h, step + 1), f"{style} contract {contract} step {step + 1}")


def test_torch_style_is_torch():
    """The op-by-op emulation is torch.optim.Adam's single-tensor path, bit for bit, over three steps."""
    h = R.DEFAULT
    inp = R.build(500, 3, 1, gexp=(-6.0, 3.0))
    p = torch.nn.Parameter(inp["p"].clone())
    opt = torch.optim.Adam([p], lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd, foreach=False)
    cur = {k: inp[k].clone() for k in ("p", "m", "v")}
    for step in (1, 2, 3):
        g = R.build(500, 3 + step, 2, gexp=(-6.0, 3.0))["g"]
        p.grad = g.clone()
        opt.step()
        cur = R.emulate(cur["p"], g, cur["m"], cur["v"], h, step, "torch", False)
        assert torch.equal(cur["p"], p.detach()) and torch.equal(cur["m"], opt.state[p]["exp_avg"]) and torch.equal(cur["v"], opt.state[p]["exp_avg_sq"]), step


@pytest.mark.parametrize("defect", R.ELEMENT_DEFECTS)
def test_element_defects_are_refused(defect):
    refused = []
    for h in R.HYPERS:
        for step in R.STEPS + [s + 1 for s in R.STEPS]:
            inp, s = _steps(h, step)
            got = R.emulate(inp["p"], inp["g"], inp["m"], inp["v"], h, step, "kernel", True, defect=defect)
            try:
                R.check_step(got, inp, s, defect)
            except AssertionError:
                refused.append((h, step))
    assert refused, f"no case refuses: {defect}"
    print(f"{defect}: refused at {len(refused)} of {len(R.HYPERS) * 2 * len(R.STEPS)} (hyper-parameters, step) pairs")


def _table_cases():
    yield "131073", [R.build(R.SIZES[5], 9, 2)]
    yield "mixed chunk", [R.build(n, 20 + i, 2) for i, n in enumerate(R.MIXED_CHUNK)]
    for n in R.COUNTS:
        yield f"{n} tensors", R.count_case(n)


def test_table_emulation_is_admitted_and_defects_refused():
    h, step = R.DEFAULT, 2
    s = R.scalars(h, step)
    refused = {d: [] for d in R.TABLE_DEFECTS}
    for label, tensors in _table_cases():
        inp = R.cat_all(tensors)
        got = R.emulate_launches(tensors, h, step)
        if tensors:
            R.check_step(R.cat_all(got, "pmv"), inp, s, label)
        for d in R.TABLE_DEFECTS:
            bad = R.emulate_launches(tensors, h, step, defect=d)
            try:
                if tensors:
                    R.check_step(R.cat_all(bad, "pmv"), inp, s, label)
            except AssertionError:
                refused[d].append(label)
    assert refused[R.TABLE_DEFECTS[0]] == ["131073", "mixed chunk"], refused          # only past the 512-block cap
    assert "49 tensors" in refused[R.TABLE_DEFECTS[2]] and "48 tensors" not in refused[R.TABLE_DEFECTS[2]], refused
    assert {"mixed chunk", "48 tensors", "97 tensors"} <= set(refused[R.TABLE_DEFECTS[1]]) and "1 tensors" not in refused[R.TABLE_DEFECTS[1]], refused


@pytest.mark.parametrize("kind", R.SPECIAL)
def test_special_values(kind):
    h = R.SPECIAL_HYPER
    inp = R.special(kind)
    s = R.scalars(h, 1)
    for style, contract in VARIANTS:
        got = R.emulate(inp["p"], inp["g"], inp["m"], inp["v"], h, 1, style, contract)
        R.check_special(kind, got, inp, s)
    if kind != "zero":          # and the checks see a change: a v' that is merely tiny / merely large is refused
        got = R.emulate(inp["p"], inp["g"], inp["m"], inp["v"], h, 1)
        got["v"] = torch.full_like(got["v"], 1e-45 if kind == "underflow" else 3e38)
        with pytest.raises(AssertionError):
            R.check_special(kind, got, inp, s)


def test_inputs_cover_what_the_issue_names():
    inp = R.build(R.HYPER_N, 1, 1000)
    g = inp["g"].double().abs()
    assert float(g.min()) < 1e-17 and float(g.max()) > 1e17
    gg = inp["g"] * inp["g"]
    assert bool(torch.isfinite(gg).all()) and bool((gg > 0).all()), "g^2 stays finite and non-zero in float32"
    assert bool((R.build(5, 1, 1)["m"] == 0).all())
    assert R.SIZES[4] == 131072 and R.SIZES[5] == 131073 and R.SIZES[6] > 589000
    sizes = [R.COUNT_SIZES[i % len(R.COUNT_SIZES)] for i in range(97)]
    assert all(a != b for a, b in zip(sizes, sizes[1:]))
    assert len(R.HYPERS) == 16
