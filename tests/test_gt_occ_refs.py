"""CPU: the ground-truth occupancy references of tests/gt_occ_refs.py.  The numpy restatement of the reference's expressions equals oracle/gt_occ_ref.c bit
for bit (depth, all points, counts, grid) on every table row, general rotation angles included; the C oracle equals the goldens recorded from the reference's
own process_frame at three further geometries; the 64-lane emulation of the kernel's run aggregation gives np.add.at's counts; every edge the table is meant
to reach occurs in some row; and each named defect changes at least one output bit of at least one row."""
import os

import numpy as np
import pytest

from tests import gt_occ_refs as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "gt_occupancy_geoms.npz"))


@pytest.fixture(scope="module")
def rows():
    out = {}
    for name in R.BY_NAME:
        g, disp, seg = R.inputs(name)
        out[name] = (g, disp, seg, R.c_oracle(g, disp, seg))
    return out


@pytest.fixture(scope="module")
def refs(rows):
    return {name: R.numpy_ref(disp, seg, g) for name, (g, disp, seg, _) in rows.items()}


@pytest.mark.parametrize("name", list(R.BY_NAME))
def test_numpy_reference_equals_c_oracle(rows, refs, name):
    g, disp, seg, c = rows[name]
    n = refs[name]
    for k in ("depth", "points", "counts", "grid"):
        assert R.same_bits(n[k], c[k]), f"{name}: {k} differs between the numpy restatement and the C oracle"
    assert np.array_equal(R.aggregate(n["cells"], g), c["counts"]), f"{name}: the 64-lane aggregation does not add up to np.add.at's counts"


@pytest.mark.parametrize("g", R.GOLDEN, ids=lambda g: g.name)
def test_c_oracle_equals_reference_goldens(rows, g):
    c = rows[g.name][3]
    key = g.name.replace(" ", "_")
    shape = tuple(G[key + "/grid_shape"])
    assert shape == (*g.grid, g.C)
    grid = np.unpackbits(G[key + "/grid_bits"])[: int(np.prod(shape))].reshape(shape).astype(bool)
    assert np.array_equal(c["grid"][0], grid) and grid.any()
    assert R.same_bits(c["depth"][0], G[key + "/depth"])
    assert R.same_bits(c["points"][0], G[key + "/points"])


def test_table_contains_what_it_must():
    T = R.TABLE
    frames = {(g.H, g.W) for g in T}
    assert {(2, 1), (3, 5), (7, 63), (8, 65), (16, 64), (37, 53)} <= frames
    assert any(g.B == 3 and (g.H, g.W) == (8, 65) for g in T) and any(g.B * g.H * g.W > R.GRID_CAP * R.BLOCK for g in T)
    assert {(256, 256, 32), (33, 21, 7), (2, 2, 2), (1, 1, 1)} <= {g.grid for g in T}
    assert {1, 3, 5} <= {g.C for g in T} and {10, 0, 0.5, -1} <= {g.threshold for g in T}
    assert {(7.0, 3.0, -2.0), (5.0, -4.0, 9.0)} <= {g.angles for g in T} and any(min(g.pc_scale) < 0 for g in T)
    assert any(g.H % 2 for g in R.GOLDEN) and all(g.angles == (7.0, 0.0, 0.0) for g in R.GOLDEN)
    vals, ids = set(), set()
    for name in R.BY_NAME:
        g, disp, seg = R.inputs(name)
        vis = disp[:, g.H // 2:]
        for label, hit in (("+0", (vis == 0) & ~np.signbit(vis)), ("-0", (vis == 0) & np.signbit(vis)), ("nan", np.isnan(vis)), ("+inf", vis == np.inf),
                           ("-inf", vis == -np.inf), ("denormal", (np.abs(vis) > 0) & (np.abs(vis) < np.finfo(np.float32).tiny)), ("negative", vis == np.float32(-0.3)),
                           ("tiny", vis == np.float32(1e-30))):
            if hit.any():
                vals.add(label)
        ids |= set(np.unique(seg).tolist()) - set(range(g.C))
    assert vals == {"+0", "-0", "nan", "+inf", "-inf", "denormal", "negative", "tiny"}, vals
    assert {-1, 255, R.INT32_MIN} <= ids and any(g.C in set(np.unique(R.inputs(g.name)[2]).tolist()) for g in T)


def test_every_edge_is_reached(rows, refs):
    found, at_threshold, last, past, guard = set(), [], [], [], []
    for name, (g, disp, seg, c) in rows.items():
        found |= R.patterns(refs[name]["cells"], g)
        if (c["counts"].astype(np.float32) == np.float32(g.threshold)).any() and g.threshold > 0:
            at_threshold.append(name)
        idx, usable, guarded = R.voxel_of_points(c["points"], g)
        if (idx[usable] == np.array(g.grid) - 1).any() and max(g.grid) > 2:
            last.append(name)
        if (idx[usable] == np.array(g.grid)).any():
            past.append(name)
        if guarded.any():
            guard.append(name)
        if name in R.NO_OCCUPIED:
            assert not c["counts"].any() and not c["grid"].any(), name
        else:
            assert c["counts"].any() and c["grid"].any(), f"{name}: no occupied cell"
            assert all(c["counts"][b].any() for b in range(g.B)), f"{name}: a batch row without a counted pixel"
    assert found == R.ALL_PATTERNS, R.ALL_PATTERNS - found
    assert at_threshold and last and past and guard, (at_threshold, last, past, guard)
    g, disp, seg, c = rows["2x1 grid 2"]
    assert c["counts"].sum() == 1 and c["counts"][0, 1, 1, 1, 0] == 1 and c["grid"].all()          # only index 1 is valid; every count exceeds -1
    print("count == threshold:", at_threshold, "\nidx == grid - 1:", last, "\nidx == grid:", past, "\nguard path:", guard)


def test_processor_row_is_not_trivial():
    """The row of the GPU test through OccupancyProcessor.process: a grid and a C other than the defaults, the numpy restatement equal to the C oracle at its
    angles, and in every frame a point list of more than 10 entries with several class ids (cells at count >= threshold, class-major)."""
    g, disp, seg = R.processor_case()
    assert g.C not in (1, 3) and g.grid != (256, 256, 32) and g.B == 2
    c, n = R.c_oracle(g, disp, seg), R.numpy_ref(disp, seg, g)
    assert all(R.same_bits(n[k], c[k]) for k in ("depth", "points", "counts", "grid"))
    for b in range(g.B):
        pts = R.occupancy_points_ref(c["counts"][b], g)
        assert pts.dtype == np.float64 and pts.shape[1] == 4 and len(pts) > 10 and len(set(pts[:, 3].tolist())) > 2
        assert (np.diff(pts[:, 3]) >= 0).all(), "class-major"
        assert len(pts) == int((c["counts"][b].astype(np.float32) >= g.threshold).sum())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_defects_change_an_output_bit(rows, refs, defect):
    changed = []
    for name in R.SMALL:
        g, disp, seg, c = rows[name]
        if defect in R.DEFECTS[:4]:
            bad = R.numpy_ref(disp, seg, g, defect)
            same = all(R.same_bits(bad[k], c[k]) for k in ("depth", "points", "counts", "grid"))
        else:
            counts = R.aggregate(refs[name]["cells"], g, defect)
            same = np.array_equal(counts, c["counts"]) and np.array_equal(counts.astype(np.float32) > np.float32(g.threshold), c["grid"])
        if not same:
            changed.append(name)
    assert changed, f"no row notices: {defect}"
    print(f"{defect}: noticed by {changed}")
