"""CPU: the reference side of tests/test_projection_geometry_gpu.py.  The two projection oracles (the C restatement the GPU tests compare with,
and the torch CPU ops the reference itself runs) agree bit for bit at every geometry of tests/projection_geometries.py; the host rotation
matrices the library is configured with are the reference's; the table reaches all five forms of launch_project; and the inputs are worth
comparing on (they set enough voxels, in every frame, without flooding the grid)."""
import numpy as np
import pytest

from oracle import cref, soccdpt_ref as R
from tests import projection_geometries as PG


@pytest.mark.parametrize("case_id", PG.CASE_IDS + ("D0",))
def test_oracles_agree(case_id):
    geo, inv, seg = PG.case_inputs(case_id)
    c = PG.case_oracle(case_id)
    inv_up, seg_up, pts, occ = R.project(inv, seg, geo.cam, geo.cfg)
    W, H = geo.cam_size
    assert PG.same(c["inv_up"], inv_up.numpy())
    assert PG.same(c["seg_up"], seg_up.numpy().reshape(geo.B, 3, H, W))     # (the torch oracle keeps the reference's B == 1 squeeze)
    assert PG.same(c["points"], pts.numpy())
    for b in range(geo.B):                                                   # the union over the batch in every row
        assert np.array_equal(occ[b].numpy(), PG.unpack(c["occ_bits"], geo))
    assert np.array_equal(cref.pack_occ(occ[0]), c["occ_bits"])              # ... and no padding bit set
    print(f"{case_id}: {PG.form_of(geo)}, {PG.popcount(c['occ_bits'])} bits set, C oracle == torch oracle")


ANGLES = sorted({g.angles for g in PG.GEOMETRIES.values()}) + [(0.0, 0.0, 0.0), (-7.0, -3.0, 2.0), (95.0, 120.0, -135.0), (180.0, 90.0, 270.0),
                                                                (0.5, -0.25, 359.0), (-181.0, 45.0, 1e-3)]


@pytest.mark.parametrize("angles", ANGLES)
def test_host_rotations_are_the_references(angles):
    from soccdpt_amd.lib import host_rotation_matrices
    got, want = host_rotation_matrices(angles), cref.rot_matrices(angles)
    assert got.dtype == np.float32 and got.shape == (27,)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if angles[1] != 0 or angles[2] != 0:      # b and c really are rotations here: not the identity the rest of the suite runs
        eye = np.eye(3, dtype=np.float32).reshape(-1)
        assert not (np.array_equal(got[9:18], eye) and np.array_equal(got[18:], eye))


def test_table_covers_every_form():
    labels = {g.id: PG.form_of(g) for g in PG.TABLE}
    print(labels)
    for g in PG.TABLE + (PG.G3PC, PG.D0):
        assert PG.form_of(g) == g.form, (g.id, PG.form_of(g), g.form)
    assert PG.eight_row_condition(PG.G3.cam_size[1], PG.G3.map_hw[0]) and PG.eight_row_condition(PG.D0.cam_size[1], PG.D0.map_hw[0])
    for g in (PG.G3, PG.D0):
        assert PG.form_of(g, rows8=True) == PG.ROWS8 and PG.form_of(g, rows1=True) == PG.ROWS1 and PG.form_of(g, rows8=True, rows1=True) == PG.ROWS1
    assert set(labels.values()) | {PG.form_of(PG.G3, rows8=True)} == set(PG.FORMS)
    # what each row is in the table for
    assert PG.G1.cam_size[0] > 1024 and PG.G1.cam_size[0] - 1024 == 4 and PG.G1.cam_size[1] % 4 == 1      # two segments, the second 4 pixels; u > ulast tail
    assert PG.G3.cam_size[1] % 4 == 2 and PG.G3.cam_size[1] % 8 == 2
    assert PG.G5.cam_size[0] % 4 != 0 and PG.G5.ncell % 32 != 0 and PG.G5.ncell % 4 == 0
    assert PG.G6.ncell % 2 == 1 and PG.G6.map_hw[0] > PG.G6.cam_size[1] and PG.G6.map_hw[1] > PG.G6.cam_size[0]   # down-sampling
    assert all(any(a != 0 for a in g.angles[1:]) for g in (PG.G2, PG.G3, PG.G6, PG.G7))                     # rot_bc_identity == 0
    assert any(g.map_hw[0] != g.map_hw[1] for g in PG.TABLE)


@pytest.mark.parametrize("case_id", PG.CASE_IDS)
def test_inputs_are_worth_comparing_on(case_id):
    geo = PG.case_inputs(case_id)[0]
    union = PG.case_oracle(case_id)["occ_bits"]
    rows = PG.case_oracle_frames(case_id)
    n = PG.popcount(union)
    per_frame = [PG.popcount(r) for r in rows]
    print(f"{case_id}: {n} of {geo.ncell} cells set, per frame {per_frame}")
    assert n >= 300
    assert min(per_frame) >= 1
    assert n <= 0.25 * geo.ncell
    assert np.array_equal(np.bitwise_or.reduce(rows, axis=0), union)


@pytest.mark.parametrize("case_id", [c for c in PG.CASE_IDS if c.endswith("plateau")])
def test_plateau_inputs_repeat_voxels(case_id):
    """The plateau inputs are there for the run-length de-duplication: many camera pixels per voxel.  In-grid pixels, recomputed in numpy from
    the oracle's points and the rotation matrices, are at least 8 x the voxels the oracle sets."""
    geo, inv, seg = PG.case_inputs(case_id)
    c = PG.case_oracle(case_id)
    rot = cref.rot_matrices(geo.angles).reshape(3, 3, 3)
    p = c["points"].reshape(-1, 3).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((p @ rot[0]) @ rot[1]) @ rot[2]
        f = q / geo.cfg.occupancy_shape() * np.array(geo.grid, np.float32)
    ok = np.isfinite(q).all(axis=1) & (np.abs(np.nan_to_num(f, nan=1e9, posinf=1e9, neginf=-1e9)) < 65536).all(axis=1)
    ijk = np.trunc(f[ok]).astype(np.int64)
    in_grid = int(((ijk > 0) & (ijk < np.array(geo.grid))).all(axis=1).sum())
    voxels = int(PG.unpack(c["occ_bits"], geo).any(axis=-1).sum())
    print(f"{case_id}: {in_grid} in-grid pixels, {voxels} voxels set ({in_grid / max(voxels, 1):.1f} pixels per voxel)")
    assert voxels > 0 and in_grid >= 8 * voxels
    # the class sets really change inside the constant-depth runs: neighbouring map pixels differ in their non-zero classes, both ways
    nz = (seg != 0)
    assert bool((nz[..., :, 1:] != nz[..., :, :-1]).any(dim=1).float().mean() > 0.5) and bool((nz[..., 1:, :] != nz[..., :-1, :]).any(dim=1).float().mean() > 0.5)
    assert bool((inv[..., :, 1:] == inv[..., :, :-1]).float().mean() > 0.9)
