"""References, geometries, inputs and the wave-aggregation emulation for the ground-truth occupancy generator (csrc/gt_occ.hip through
soccdpt_gt_occupancy).  Everything here is bit for bit: there are no tolerances.

Three statements of the same frame -> (depth, points, counts, grid) function:
  * `numpy_ref`: a vectorised numpy restatement written from the reference's own numpy expressions (OccupancyProcessor.process_frame and
    transform_points_to_occupancy_grid_vect of datasets/bdd_helper.py): np.reciprocal on float32, the float64 product rounded to float32 once, the hidden
    upper half `depth.shape[0] // 2`, (V - cx) * Z / fx in float64, separate scale and shift, three np.dot with the transposed rotations (the angles are a
    parameter), `(points / occupancy_shape * grid_size).astype(int)`, the strict bounds, np.add.at, `> threshold`.  It shares no line with
  * oracle/gt_occ_ref.c, the scalar C program the kernel was written against (explicit fma() in dgemm's K = 3 order), and
  * the kernel, which adds the wave-wide run aggregation (`aggregate`: the 64-lane emulation of it).
tests/test_gt_occ_refs.py holds the first two to each other and to goldens recorded from the reference's own process_frame; tests/test_gt_occupancy_gpu.py
holds the kernel to the C oracle and the goldens.

The class-id contract (gt_occ.hip's header): an id outside [0, C) contributes nothing.  The reference's np.add.at would wrap -1 to the last class and raise
IndexError on an id >= C; its rgb_seg_to_class never produces either.  `numpy_ref` follows the contract unless told otherwise (DEFECTS).

The one place the restatements do not follow numpy is a voxel coordinate beyond +-9e18, where `astype(int)` is undefined in C (numpy gives INT64_MIN on
x86-64, which fails `0 < idx`): all three reject the pixel explicitly.
"""
import math
from collections import namedtuple

import numpy as np

Geom = namedtuple("Geom", "name B H W C grid extent pc_scale pc_shift threshold angles f build")
WAVE = 64
BLOCK = 256
GRID_CAP = 8192
INT32_MIN = -2 ** 31
DEFAULT_EXTENT = (128.0, 128.0, 32 / 0.666)          # metres covered by the reference's grid (256, 256, 32) at scale (2, 2, 0.666)


def scale_of(g):
    """voxels per metre such that the grid covers g.extent: a smaller grid at the default scale holds nothing of the scene."""
    return tuple(g.grid[k] / g.extent[k] for k in range(3))


def intrinsics(g):
    """A camera for an H x W frame: the principal point off-centre and off-integer, fx != fy."""
    return np.array([[g.f, 0.0, g.W / 2.0 - 0.3], [0.0, g.f * 1.01, g.H / 2.0 + 0.2], [0.0, 0.0, 1.0]])


def rot_matrices(angles):
    """The three matrices of rotate_points (math.cos / math.sin of math.radians), untransposed."""
    a, b, c = [math.radians(v) for v in angles]
    return (np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]]),
            np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]]),
            np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]]))


DEFECTS = (">= at the threshold", "H / 2 rounded up", "<= at the grid bound", "class -1 wrapped to the last class", "runs merged across a rejected pixel",
           "a run cut at lane 63 and lost", "idle tail lanes excluded from the ballot", "counts not cleared per batch row")


def frame_cells(disp, seg, g, defect=None):
    """One frame -> (depth f32 [H, W], points f64 [H * W, 3], cell int64 [H * W]): the flat (voxel, class) counter index of every pixel, -1 where it
    contributes nothing."""
    H, W = disp.shape
    K = intrinsics(g)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    baseline, focal = 1.0 * 10 ** -2, (fx + fy) / 2.0
    with np.errstate(all="ignore"):
        depth = (baseline * focal * np.reciprocal(disp.astype(np.float32)).astype(np.float64)).astype(np.float32)
        hide = np.zeros((H, W), dtype=bool)
        hide[0: ((H + 1) // 2 if defect == DEFECTS[1] else H // 2)] = True
        depth[hide] = float("inf")
        depth[np.isinf(depth)] = 0
        depth[np.isnan(depth)] = 0
        U, V = np.ix_(np.arange(H), np.arange(W))
        Z = depth.copy()
        X = ((V - cx) * Z / fx).flatten()
        Y = ((U - cy) * Z / fy).flatten()
        points = np.array([X, Y, Z.flatten()]).T
        for k in range(3):
            points[:, k] = points[:, k] * g.pc_scale[k] + g.pc_shift[k]
        for M in rot_matrices(g.angles):
            points = np.dot(points, M.T)
        finite = ~np.isinf(points).any(axis=1) & ~np.isnan(points).any(axis=1)
        occupancy_shape = np.array([float(g.grid[k] / scale_of(g)[k]) for k in range(3)], dtype=np.float32)
        f = points / occupancy_shape * np.array(g.grid)
        inside = finite & (np.abs(np.where(finite[:, None], f, 0.0)) < 9.0e18).all(axis=1)
        ijk = np.where(inside[:, None], f, 0.0).astype(np.int64)
    hi = (ijk <= np.array(g.grid)) if defect == DEFECTS[2] else (ijk < np.array(g.grid))
    ok = inside & ((0 < ijk) & hi).all(axis=1)
    c = seg.reshape(-1).astype(np.int64)
    if defect == DEFECTS[3]:
        c = np.where(c == -1, g.C - 1, c)
    ok &= (0 <= c) & (c < g.C)
    flat = ((ijk[:, 0] * g.grid[1] + ijk[:, 1]) * g.grid[2] + ijk[:, 2]) * g.C + c
    return depth, points, np.where(ok, flat, -1)


def ncell(g):
    return g.grid[0] * g.grid[1] * g.grid[2] * g.C


def numpy_ref(disp, seg, g, defect=None):
    """disp f32 [B, H, W], seg int [B, H, W] -> dict(depth [B, H, W], points [B, H * W, 3], counts uint32 [B, g0, g1, g2, C], grid bool): np.add.at per frame."""
    assert defect is None or defect in DEFECTS[:4], defect
    out = dict(depth=[], points=[], counts=[], cells=[])
    n = ncell(g)
    for b in range(disp.shape[0]):
        depth, points, cell = frame_cells(disp[b], seg[b], g, defect)
        counts = np.zeros(n + (g.grid[1] * g.grid[2] * g.C + g.grid[2] * g.C + g.C if defect == DEFECTS[2] else 0), dtype=np.float32)
        np.add.at(counts, cell[cell >= 0], 1)
        out["depth"].append(depth)
        out["points"].append(points)
        out["counts"].append(counts[:n].astype(np.uint32).reshape(*g.grid, g.C))
        out["cells"].append(cell)
    out = {k: np.stack(v) for k, v in out.items()}
    thr = np.float32(g.threshold)
    out["grid"] = (out["counts"].astype(np.float32) >= thr) if defect == DEFECTS[0] else (out["counts"].astype(np.float32) > thr)
    return out


# ---------------- the kernel's 64-lane run aggregation ----------------
def lanes(cells, g):
    """cells int64 [B, H * W] (per frame, -1 = nothing) -> (cell [n_waves, 64] with the batch row's offset added, idle [n_waves, 64]): the threads of
    gt_points_count_kernel in launch order.  The grid is capped and the loop bound rounded up to whole waves; every wave is 64 consecutive pixels of the
    flattened batch whatever the round, the lanes past the end are idle (cell -1) and still take part in the ballot."""
    B, npix = cells.shape
    total = B * npix
    flat = np.where(cells >= 0, cells + (np.arange(B) * ncell(g))[:, None], -1).reshape(-1)
    padded = -np.ones((total + WAVE - 1) // WAVE * WAVE, dtype=np.int64)
    padded[:total] = flat
    idle = np.arange(padded.size) >= total
    return padded.reshape(-1, WAVE), idle.reshape(-1, WAVE)


def run_heads(cell, idle, defect=None):
    """-> (head bool [n_waves, 64], run int [n_waves, 64]): `head = lane == 0 || left != cell`, run = distance to the next head, or to the wave's end."""
    cell = cell.copy()
    if defect == DEFECTS[4]:          # a rejected pixel does not end the run around it
        for lane in range(1, WAVE):
            cell[:, lane] = np.where((cell[:, lane] < 0) & ~idle[:, lane], cell[:, lane - 1], cell[:, lane])
    head = np.ones_like(cell, dtype=bool)
    head[:, 1:] = cell[:, 1:] != cell[:, :-1]
    if defect == DEFECTS[5]:          # lane 0 compares with lane 63 of the wave before: the second part of a run that spans two waves is lost
        head[1:, 0] = cell[1:, 0] != cell[:-1, WAVE - 1]
    ballot = head & ~idle if defect == DEFECTS[6] else head
    nxt = np.full(cell.shape[0], WAVE)
    run = np.zeros_like(cell)
    for lane in range(WAVE - 1, -1, -1):
        run[:, lane] = nxt - lane
        nxt = np.where(ballot[:, lane], lane, nxt)
    return head, run


def aggregate(cells, g, defect=None):
    """The counts the kernel's atomics add up to: uint32 [B, g0, g1, g2, C]."""
    assert defect is None or defect in DEFECTS[4:], defect
    B = cells.shape[0]
    cell, idle = lanes(cells, g)
    head, run = run_heads(cell, idle, defect)
    counts = np.zeros(B * ncell(g), dtype=np.int64)
    sel = head & (cell >= 0)
    np.add.at(counts, cell[sel], run[sel])
    counts = counts.reshape(B, -1)
    if defect == DEFECTS[7]:
        counts = np.cumsum(counts, axis=0)
    return counts.astype(np.uint32).reshape(B, *g.grid, g.C)


def patterns(cells, g):
    """Which of the run patterns the issue names occur among the waves of a row -> set of names."""
    cell, idle = lanes(cells, g)
    head, run = run_heads(cell, idle)
    live = cell >= 0
    found = set()
    if ((run[:, 0] == WAVE) & live[:, 0]).any():
        found.add("a run of exactly 64 aligned to a wave")
    ends63 = live[:, WAVE - 1] & ~head[:, WAVE - 1] & (run[:, 0] < WAVE)
    if ends63.any():
        found.add("a run ending at lane 63")
    if (live[1:, 0] & (cell[1:, 0] == cell[:-1, WAVE - 1])).any():
        found.add("a run spanning two waves")
    if (head & live).all(axis=1).any():
        found.add("every lane a head")
    for lane in range(WAVE - 5):
        w = cell[:, lane: lane + 6]
        if ((w[:, 0] >= 0) & (w[:, 0] == w[:, 1]) & (w[:, 2] < 0) & (w[:, 3] < 0) & (w[:, 4] == w[:, 0]) & (w[:, 5] == w[:, 0]) & ~idle[:, lane + 5]).any():
            found.add("A A x x A A")
    B, npix = cells.shape
    for b in range(1, B):
        t = b * npix
        if t % WAVE and cells[b - 1, -1] >= 0 and cells[b - 1, -1] == cells[b, 0]:
            found.add("the same voxel on either side of a batch boundary inside a wave")
    if idle.any() and live[-1].any():
        found.add("idle tail lanes behind live ones")
    if B * npix > GRID_CAP * BLOCK:
        found.add("a second round of the loop")
    return found


ALL_PATTERNS = {"a run of exactly 64 aligned to a wave", "a run ending at lane 63", "a run spanning two waves", "every lane a head", "A A x x A A",
                "the same voxel on either side of a batch boundary inside a wave", "idle tail lanes behind live ones", "a second round of the loop"}


# ---------------- inputs ----------------
def scene(g, seed):
    """A smooth depth of 0.02 .. 0.1 (the reference's scene after pc_scale = (500, 2500, 200)) as a float32 disparity, and a blocky class map in [0, C)."""
    rng = np.random.RandomState(seed)
    B, H, W = g.B, g.H, g.W
    gh, gw = max(2, H // 6 + 1), max(2, W // 6 + 1)
    coarse = rng.rand(B, gh, gw)
    yi, xi = np.minimum(np.arange(H) * gh // max(H, 1), gh - 1), np.minimum(np.arange(W) * gw // max(W, 1), gw - 1)
    ramp = np.linspace(0.0, 1.0, H)[None, :, None] * 0.5
    depth = 0.02 + 0.08 * np.clip(0.5 * coarse[:, yi][:, :, xi] + ramp + 0.02 * rng.rand(B, H, W), 0, 1)
    K = intrinsics(g)
    disp = (0.01 * (K[0, 0] + K[1, 1]) / 2.0 / depth).astype(np.float32)
    seg = rng.randint(0, g.C, size=(B, max(1, H // 3 + 1), max(1, W // 5 + 1)))[:, np.arange(H) // 3][:, :, np.arange(W) // 5].astype(np.int32)
    return disp, seg


def _plain(g):
    return scene(g, 1)


def _degenerate(g):
    """Special disparities in the visible half (+0, -0, NaN, +-inf, a denormal, a negative, one so small that the voxel coordinate passes 9e18) and class ids
    outside [0, C) among valid ones."""
    disp, seg = scene(g, 2)
    vals = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-40, -0.3, 1e-30, -1e-30], dtype=np.float32)
    u = g.H // 2 + (g.H - g.H // 2) // 2
    for b in range(g.B):
        n = min(len(vals), g.W)
        disp[b, u, :n] = vals[:n]
        disp[b, g.H - 1, g.W - n:] = vals[:n][::-1]
        bad = np.array([-1, g.C, 255, INT32_MIN], dtype=np.int32)
        seg[b, g.H - 1, : min(4, g.W)] = bad[: min(4, g.W)]
        seg[b, 0, : min(4, g.W)] = bad[: min(4, g.W)][::-1]
    return disp, seg


def _batch_edges(g):
    """B frames whose pixel count is no multiple of 64: the last pixels of a frame (disparity +inf: depth 0, the voxel of pc_shift) and the first, hidden,
    pixels of the next share a voxel and a class across the batch boundary inside a wave; bad class ids in between."""
    disp, seg = _degenerate(g)
    disp[:, g.H - 1, g.W - 12:] = np.inf
    seg[:, g.H - 1, g.W - 12:] = 0
    seg[:, 0, :12] = 0
    return disp, seg


def _runs(g):
    """W = 64: every camera row is one wave.  The hidden rows (depth 0) all fall into the voxel of pc_shift, so their cells differ by class only."""
    assert g.W == WAVE and g.H >= 12 and g.C >= 2
    disp, seg = scene(g, 3)
    seg[:, 0] = 0                                   # a run of exactly 64 equal cells aligned to a wave
    seg[:, 1, :40], seg[:, 1, 40:] = 1, 0           # a run ending at lane 63 ...
    seg[:, 2, :10], seg[:, 2, 10:] = 0, 1           # ... that continues in the next wave: a run spanning two waves
    seg[:, 3] = np.arange(WAVE) % 2                 # every lane a head
    seg[:, 4] = np.tile(np.array([0, 0, -1, -1, 0, 0, 1, 1], dtype=np.int32), 8)          # A A x x A A
    seg[:, 5, :10], seg[:, 5, 10:] = 1, 0           # exactly 10 + 40 + 54 + 32 + 16 + 10 pixels of class 1 in the hidden voxel
    return disp, seg


def _threshold_hit(g):
    """Class C - 1 occurs at exactly `threshold` hidden pixels and nowhere else: a count equal to its threshold."""
    disp, seg = _degenerate(g)
    seg = np.where(seg == g.C - 1, 0, seg)
    n = int(g.threshold)
    assert 0 < n <= g.W and g.H >= 4
    seg[:, 1, :n] = g.C - 1
    return disp, seg


D = dict(extent=DEFAULT_EXTENT, pc_scale=(500.0, 2500.0, 200.0), pc_shift=(100.0, 40.0, 0.0), angles=(7.0, 0.0, 0.0), f=60.0)


def _g(name, B, H, W, C, grid, threshold, build, **kw):
    a = dict(D, **kw)
    return Geom(name, B, H, W, C, grid, a["extent"], a["pc_scale"], a["pc_shift"], threshold, a["angles"], a["f"], build)


TABLE = [
    _g("2x1 grid 2", 1, 2, 1, 1, (2, 2, 2), -1, _plain, extent=(150.0, 70.0, 9.0), f=2.0),
    _g("3x5 odd H", 2, 3, 5, 3, (33, 21, 7), 0, _degenerate, angles=(7.0, 3.0, -2.0), pc_shift=(100.0, 40.0, 12.0), f=6.0),
    _g("7x63 below a wave row", 1, 7, 63, 5, (256, 256, 32), 0.5, _degenerate, angles=(5.0, -4.0, 9.0), pc_scale=(-500.0, 2500.0, 200.0)),
    _g("8x65 B 3", 3, 8, 65, 3, (33, 21, 7), 0, _batch_edges, angles=(7.0, 3.0, -2.0), extent=(128.0, 100.0, 32 / 0.666), pc_shift=(100.0, 40.0, 12.0), f=30.0),
    _g("16x64 runs", 2, 16, 64, 3, (33, 21, 7), 10, _runs, extent=(128.0, 100.0, 32 / 0.666), pc_shift=(100.0, 40.0, 5.0), f=20.0),
    _g("37x53 threshold", 2, 37, 53, 3, (256, 256, 32), 10, _threshold_hit, angles=(5.0, -4.0, 9.0), pc_shift=(90.0, 35.0, 2.0)),
    _g("3x5 grid 1", 1, 3, 5, 3, (1, 1, 1), 0, _plain, f=6.0),
    _g("1040x2048 second round", 1, 1040, 2048, 3, (256, 256, 32), 10, _plain, f=1300.0),
]
# the rows recorded from the reference's own process_frame (rotation (7, 0, 0), which it hard-codes; class ids in [0, C) only, which is all its
# rgb_seg_to_class produces): other cameras (one with odd H), grids, scales, pc_scale / pc_shift, thresholds and C
GOLDEN = [
    _g("golden 9x20", 1, 9, 20, 5, (33, 21, 7), 0.5, _plain, f=25.0),
    _g("golden 12x31", 1, 12, 31, 1, (256, 256, 32), 0, _plain, pc_scale=(-500.0, 2500.0, 200.0), pc_shift=(120.0, 30.0, 1.0), f=40.0),
    _g("golden 16x64", 1, 16, 64, 3, (40, 50, 9), 2, _plain, extent=(128.0, 100.0, 40.0), pc_shift=(100.0, 40.0, 0.5)),
]
BY_NAME = {g.name: g for g in TABLE + GOLDEN}
SMALL = [g.name for g in TABLE if g.H * g.W < 100000] + [g.name for g in GOLDEN]
NO_OCCUPIED = {"3x5 grid 1"}


def inputs(name):
    g = BY_NAME[name]
    disp, seg = g.build(g)
    return g, np.ascontiguousarray(disp, dtype=np.float32), np.ascontiguousarray(seg, dtype=np.int32)


def processor_case():
    """The row of the OccupancyProcessor.process test: "golden 9x20" (grid (33, 21, 7), C = 5, threshold 0.5) with two frames and general correction angles."""
    g = BY_NAME["golden 9x20"]._replace(name="processor", B=2, angles=(5.0, -4.0, 9.0))
    disp, seg = g.build(g)
    return g, np.ascontiguousarray(disp, dtype=np.float32), np.ascontiguousarray(seg, dtype=np.int32)


def c_oracle(g, disp, seg):
    """oracle/gt_occ_ref.c per frame -> the same dict as numpy_ref."""
    from oracle import cref
    K = intrinsics(g)
    P = cref.gt_params(g.H, g.W, g.C, K[0, 0], K[1, 1], K[0, 2], K[1, 2], grid_size=g.grid, scale=scale_of(g), pc_scale=g.pc_scale, pc_shift=g.pc_shift,
                       threshold=g.threshold, angles=g.angles)
    frames = [cref.gt_occupancy(disp[b], seg[b], P) for b in range(g.B)]
    return {k: np.stack([f[k] for f in frames]) for k in ("depth", "points", "counts", "grid")}


def voxel_of_points(points, g):
    """points f64 [..., 3] as an implementation returned them -> (idx int64 [N, 3], usable bool [N], guarded bool [N]): the voxel index of every finite point
    whose coordinate is inside +-9e18, and which finite points took the guard path."""
    pts = points.reshape(-1, 3)
    shape = np.array([np.float32(g.grid[k] / scale_of(g)[k]) for k in range(3)], dtype=np.float32)
    with np.errstate(all="ignore"):
        f = pts / shape * np.array(g.grid)
        finite = np.isfinite(pts).all(axis=1)
        usable = finite & (np.abs(np.where(finite[:, None], f, 0.0)) < 9.0e18).all(axis=1)
        idx = np.where(usable[:, None], f, 0.0).astype(np.int64)
    return idx, usable, finite & ~usable


def occupancy_points_ref(counts, g):
    """transform_points_to_occupancy_grid_vect's `occupancy_points` from one frame's counts, in the reference's own expressions: float64 [N, 4]."""
    grid_size = tuple(g.grid)
    occupancy_shape = np.array([float(g.grid[k] / scale_of(g)[k]) for k in range(3)], dtype=np.float32)
    occupancy_points_indices = np.argwhere(counts.astype(np.float32) >= g.threshold)
    occupancy_points = []
    for class_id in range(g.C):
        class_indices = occupancy_points_indices[occupancy_points_indices[:, 3] == class_id][:, :3]
        class_points = (class_indices / grid_size[:3] * occupancy_shape[:3]).astype(np.float32)
        occupancy_points.append(np.concatenate([class_points, np.full((class_points.shape[0], 1), class_id)], axis=1))
    return np.concatenate(occupancy_points, axis=0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
