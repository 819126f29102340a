"""A scalar float64 restatement of soccdpt_occ_rays_observed, written from the comment of include/soccdpt_occ_rays.h (TEST INFRASTRUCTURE ONLY), the
exact-arithmetic bounds it is sandwiched between, a numpy statement of soccdpt_occ_iou_counts_masked, and the case table every occ_rays test uses.

`cast_ray` follows the header line by line in numpy float64 scalars: every operation is one IEEE operation, rounded on its own.  It shares no text
with csrc/occ_rays_core.h.  `exact_voxels` knows nothing of traversal: from the float64 segment ends it lists, in fractions.Fraction, the voxels
whose cube, grown or shrunk by eps, meets the segment.

DEFECTS are planted into the restatement one at a time; tests/test_occ_rays_cpu.py checks that the case table refuses each of them."""
import math
from fractions import Fraction

import numpy as np

from soccdpt_amd.utils.occupancy_rays import camera_to_voxel      # the table's model and processor geometries go through the product's own inverse

F = np.float64
EPS = Fraction(1, 2 ** 30)

DEFECTS = ("end voxel dropped", "entry voxel after clipping dropped", "tie stepped on the higher axis only", "row offset lost",
           "bits lost when the word changes", "step / 2 offset dropped", "<= for < at z_near")


def nvox_of(g):
    return int(g[0]) * int(g[1]) * int(g[2])


def nvw_of(g):
    return (nvox_of(g) + 31) // 32


def cast_pixels(n, step, defect=None):
    """u = step / 2 + a step (C integer division) inside [0, n)."""
    first = 0 if defect == DEFECTS[5] else step // 2
    return list(range(first, n, step))


def _finite(x):
    return bool(np.isfinite(x))


def _clamp_floor(x, n):
    f = np.floor(x)
    if not f >= 0.0:
        return 0
    if f > F(n - 1):
        return n - 1
    return int(f)


def segment(N, K, z_near, max_depth, u, v, depth, defect=None):
    """-> (S, D, E) as lists of three float64, or None when the header skips the ray before clipping."""
    fx, fy, cx, cy = (F(x) for x in K)
    z_near, max_depth = F(z_near), F(max_depth)
    N = [F(x) for x in np.asarray(N, dtype=np.float64).reshape(-1)]
    Z = F(np.float32(depth))
    if not _finite(Z):
        return None
    if defect == DEFECTS[6]:
        if not Z >= z_near:
            return None
    elif not Z > z_near:
        return None
    if max_depth > 0.0 and Z > max_depth:
        Z = max_depth
    dx = (F(u) - cx) / fx
    dy = (F(v) - cy) / fy
    A = (dx * z_near, dy * z_near, z_near)
    B = (dx * Z, dy * Z, Z)
    S, D, E = [], [], []
    for a in range(3):
        n0, n1, n2, n3 = N[4 * a: 4 * a + 4]
        s = ((n0 * A[0] + n1 * A[1]) + n2 * A[2]) + n3
        e = ((n0 * B[0] + n1 * B[1]) + n2 * B[2]) + n3
        d = e - s
        if not (_finite(s) and _finite(d)):
            return None
        S.append(s)
        D.append(d)
        E.append(e)
    return S, D, E


def cast_ray(N, K, g, z_near, max_depth, u, v, depth, defect=None):
    """The voxels (flat index m) one ray marks, in the order it enters them."""
    with np.errstate(all="ignore"):
        sd = segment(N, K, z_near, max_depth, u, v, depth, defect)
        if sd is None:
            return []
        S, D, _ = sd
        t0, t1 = F(0.0), F(1.0)
        for a in range(3):
            ga = F(g[a])
            if D[a] == 0.0:
                if not (S[a] >= 0.0 and S[a] < ga):
                    return []
            else:
                p, q = (F(0.0) - S[a]) / D[a], (ga - S[a]) / D[a]
                t0 = max(t0, min(p, q))
                t1 = min(t1, max(p, q))
            if not t0 <= t1:
                return []
        i = [_clamp_floor(S[a] + t0 * D[a], g[a]) for a in range(3)]
        e = [_clamp_floor(S[a] + t1 * D[a], g[a]) for a in range(3)]
        out = []
        for trip in range(g[0] + g[1] + g[2] + 3):
            if not all(0 <= i[a] < g[a] for a in range(3)):
                break
            at_end = i == e
            dropped = (defect == DEFECTS[0] and at_end) or (defect == DEFECTS[1] and trip == 0 and t0 > 0.0)
            if not dropped:
                out.append((i[0] * g[1] + i[1]) * g[2] + i[2])
            if at_end:
                break
            k, ck = -1, F(0.0)
            for a in range(3):
                if D[a] == 0.0:
                    continue
                b = F(i[a] + 1) if D[a] > 0.0 else F(i[a])
                c = (b - S[a]) / D[a]
                if k < 0 or c < ck or (defect == DEFECTS[2] and c == ck):
                    k, ck = a, c
            if k < 0 or not ck <= t1:
                break
            i[k] += 1 if D[k] > 0.0 else -1
        return out


def observed_ref(case, defect=None):
    """The mask soccdpt_occ_rays_observed leaves for a case: uint32 [rows, nvw]."""
    g, rows, H, W = case["g"], case["rows"], case["H"], case["W"]
    out = np.zeros((rows, nvw_of(g)), dtype=np.uint32) if case["init"] is None else case["init"].copy()
    for r in range(rows):
        for v in cast_pixels(H, case["step"], defect):
            for u in cast_pixels(W, case["step"], defect):
                ms = cast_ray(case["N"], case["K"], g, case["z_near"], case["max_depth"], u, v, case["depth"][r, v, u], defect)
                if defect == DEFECTS[4] and ms:      # a lane that drops its register when it moves on keeps only the last word's bits
                    ms = [m for m in ms if m >> 5 == ms[-1] >> 5]
                for m in ms:
                    out[0 if defect == DEFECTS[3] else r, m >> 5] |= np.uint32(1 << (m & 31))
    return out


def mask_to_set(words):
    """One row of a mask -> the set of voxel indices."""
    w = np.asarray(words, dtype=np.uint32)
    return set(np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little")).tolist())


# ---------------- exact arithmetic ----------------
def _slab(s, d, lo, hi, t0, t1):
    """{t in [t0, t1]: lo <= s + t d <= hi} as a closed interval, or None."""
    if d == 0:
        return (t0, t1) if lo <= s <= hi else None
    p, q = (lo - s) / d, (hi - s) / d
    if p > q:
        p, q = q, p
    t0, t1 = max(t0, p), min(t1, q)
    return (t0, t1) if t0 <= t1 else None


def exact_voxels(S, E, g, eps):
    """The voxels whose cube [i - eps, i + 1 + eps]^3 (eps < 0: shrunk) meets the segment from S to E, in exact arithmetic on the float64 ends."""
    S = [Fraction(float(x)) for x in S]
    E = [Fraction(float(x)) for x in E]
    D = [E[a] - S[a] for a in range(3)]
    found = set()

    def descend(a, t0, t1, idx):
        if a == 3:
            found.add((idx[0] * g[1] + idx[1]) * g[2] + idx[2])
            return
        x0, x1 = S[a] + t0 * D[a], S[a] + t1 * D[a]
        lo, hi = min(x0, x1), max(x0, x1)
        for i in range(max(0, math.floor(lo - abs(eps)) - 1), min(g[a] - 1, math.floor(hi + abs(eps)) + 1) + 1):
            iv = _slab(S[a], D[a], i - eps, i + 1 + eps, t0, t1)
            if iv is not None:
                descend(a + 1, iv[0], iv[1], idx + [i])

    descend(0, Fraction(0), Fraction(1), [])
    return found


def sandwich(case):
    """For every cast ray of the case -> list of (row, u, v, missing from the restatement, beyond the upper bound); empty when it holds."""
    bad = []
    g = case["g"]
    with np.errstate(all="ignore"):
        for r in range(case["rows"]):
            for v in cast_pixels(case["H"], case["step"]):
                for u in cast_pixels(case["W"], case["step"]):
                    d = case["depth"][r, v, u]
                    got = set(cast_ray(case["N"], case["K"], g, case["z_near"], case["max_depth"], u, v, d))
                    sd = segment(case["N"], case["K"], case["z_near"], case["max_depth"], u, v, d)
                    if sd is None:
                        assert not got
                        continue
                    S, _, E = sd
                    lower, upper = exact_voxels(S, E, g, -EPS), exact_voxels(S, E, g, EPS)
                    if not (lower <= got <= upper):
                        bad.append((r, u, v, sorted(lower - got), sorted(got - upper)))
    return bad


# ---------------- masked IoU ----------------
def unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)


def iou_masked_ref(pred, gt, mask, nvox, C, include_gt):
    """pred [pred_rows, nwords], gt [rows, nwords], mask [mask_rows, nvw] uint32 -> (counts int64 [rows, C, 4], observed int64 [rows])."""
    rows = gt.shape[0]
    counts, observed = np.zeros((rows, C, 4), dtype=np.int64), np.zeros(rows, dtype=np.int64)
    for r in range(rows):
        p = unpack(pred[r if pred.shape[0] > 1 else 0], nvox * C).reshape(nvox, C)
        q = unpack(gt[r], nvox * C).reshape(nvox, C)
        m = unpack(mask[r if mask.shape[0] > 1 else 0], nvox)
        if include_gt:
            m = m | q.any(axis=1)
        observed[r] = m.sum()
        p, q = p & m[:, None], q & m[:, None]
        counts[r] = np.stack([(p & q).sum(0), (p | q).sum(0), p.sum(0), q.sum(0)], axis=1)
    return counts, observed


# ---------------- geometries ----------------
def invert(M):
    """voxel-centre -> camera (3 x 4) to camera -> continuous voxel coordinate (3 x 4): what utils/occupancy_rays.camera_to_voxel must return."""
    M = np.asarray(M, dtype=np.float64)
    Li = np.linalg.inv(M[:, :3])
    return np.concatenate([Li, -(Li @ M[:, 3]).reshape(3, 1)], axis=1)


def axis_aligned(origin, cell=1.0):
    """Camera X, Y, Z along grid axes 0, 1, 2; the camera centre sits at the voxel coordinate `origin`; one voxel is `cell` metres.  With cell a power
    of two, integer intrinsics and origin on a half or whole number, rays run exactly along grid lines and through voxel corners."""
    N = np.zeros((3, 4))
    for a in range(3):
        N[a, a] = 1.0 / cell
        N[a, 3] = origin[a]
    return N


def model_matrix(g, extent, angles):
    """SOccDPT.voxel_to_camera() for grid g covering `extent` metres with correction_angle `angles`, inverted."""
    from soccdpt_amd.lib import host_rotation_matrices
    from soccdpt_amd.utils.occupancy_views import model_voxel_to_camera
    return camera_to_voxel(model_voxel_to_camera(g, np.array(extent, dtype=np.float32), host_rotation_matrices(angles)))


def processor_matrix(g, extent, pc_scale, pc_shift, angles):
    """OccupancyProcessor.voxel_to_camera() for the same, inverted."""
    from tests.gt_occ_refs import rot_matrices
    from soccdpt_amd.utils.occupancy_views import processor_voxel_to_camera
    rot_t = np.concatenate([m.T.reshape(-1) for m in rot_matrices(angles)])
    return camera_to_voxel(processor_voxel_to_camera(g, np.array(extent, dtype=np.float32), pc_scale, pc_shift, rot_t))


SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0], dtype=np.float32)


def _depth(rows, H, W, lo, hi, seed, specials=True):
    rng = np.random.RandomState(seed)
    d = (lo + (hi - lo) * rng.rand(rows, H, W)).astype(np.float32)
    if specials:
        flat = d.reshape(rows, -1)
        n = flat.shape[1]
        for r in range(rows):
            for k, s in enumerate(SPECIALS):
                if n > len(SPECIALS) + 2:
                    flat[r, (3 * k + r) % n] = s
    return d


def _case(name, g, W, H, rows, step, N, K, depth, z_near=0.0, max_depth=0.0, preset=None):
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    assert depth.shape == (rows, H, W), (name, depth.shape)
    init = None
    if preset is not None:
        init = np.random.RandomState(preset).randint(0, 2 ** 32, size=(rows, nvw_of(g)), dtype=np.uint64).astype(np.uint32)
        init &= np.random.RandomState(preset + 1).randint(0, 2 ** 32, size=init.shape, dtype=np.uint64).astype(np.uint32)
        if nvox_of(g) % 32:
            init[:, -1] &= np.uint32((1 << (nvox_of(g) % 32)) - 1)
    return dict(name=name, g=tuple(g), W=W, H=H, rows=rows, step=step, N=np.ascontiguousarray(N, dtype=np.float64),
                K=np.array(K, dtype=np.float64), depth=depth, z_near=float(z_near), max_depth=float(max_depth), init=init)


def _table():
    T = []
    # --- axis-aligned, camera inside the box at a voxel corner: rays along grid lines and through voxel corners (ties on two and three axes) ---
    # fx = fy = 1 and an integer principal point: dx and dy are whole numbers, so with Z whole every end is a lattice point
    d = np.array([[[3, 2, 1, 2, 3, 4, 5], [2, 1, 3, 2, 2, 2, 2], [1, 1, 2, 3, 1, 9, 3], [2, 2, 1, 1, 2, 2, 1], [3, 3, 3, 3, 2, 1, 2]]], dtype=np.float32)
    T.append(_case("corners 8x8x4, 7x5", (8, 8, 4), 7, 5, 1, 1, axis_aligned((4.0, 4.0, 0.0)), (1.0, 1.0, 3.0, 2.0), d))
    T.append(_case("corners 5x7x3, 7x5, step 2, z_near on a face", (5, 7, 3), 7, 5, 2, 2, axis_aligned((2.0, 3.0, 0.0)), (1.0, 1.0, 3.0, 2.0),
                   np.concatenate([d, d[:, ::-1] * 0.5]), z_near=1.0))
    # half a voxel: rays run along the middle of a column and diagonally through edges
    T.append(_case("half cell 8x8x4, 24x16, step 3", (8, 8, 4), 24, 16, 3, 3, axis_aligned((4.5, 3.5, 0.5), cell=0.5), (4.0, 4.0, 12.0, 8.0),
                   _depth(3, 16, 24, 0.25, 2.5, 11), z_near=0.125, max_depth=2.0))
    # depth equal to z_near (cast nothing), just above it, above max_depth; 1 x 1 and 64 x 1 cameras
    T.append(_case("1x1 inside", (8, 8, 4), 1, 1, 1, 1, axis_aligned((4.25, 4.75, 0.5)), (1.0, 1.0, 0.0, 0.0), [[[2.0]]]))
    T.append(_case("1x1 step 2 casts nothing", (8, 8, 4), 1, 1, 2, 2, axis_aligned((4.25, 4.75, 0.5)), (1.0, 1.0, 0.0, 0.0), [[[2.0]], [[1.0]]], preset=5))
    T.append(_case("1x1 at z_near", (8, 8, 4), 1, 1, 1, 1, axis_aligned((4.25, 4.75, 0.5)), (1.0, 1.0, 0.0, 0.0), [[[0.5]]], z_near=0.5))
    row = np.linspace(0.2, 6.0, 64, dtype=np.float32)
    row[[0, 5, 9, 63]] = (0.5, np.nan, 0.5000001, np.inf)
    T.append(_case("64x1 z_near and max_depth", (8, 8, 4), 64, 1, 1, 1, axis_aligned((0.5, 4.5, 0.25)), (8.0, 8.0, 1.0, 0.0), row.reshape(1, 1, 64), z_near=0.5,
                   max_depth=3.0))
    # camera outside the box: clipped entries, rays that miss, rays ending before and beyond the box
    T.append(_case("outside 5x7x3, 65x3", (5, 7, 3), 65, 3, 2, 1, axis_aligned((2.3, 3.1, -2.0)), (20.0, 1.5, 32.0, 1.0), _depth(2, 3, 65, 0.5, 8.0, 12)))
    T.append(_case("outside sideways 33x2x40, 65x3, step 2", (33, 2, 40), 65, 3, 3, 2, axis_aligned((-3.0, 1.0, 5.5)), (30.0, 40.0, -10.0, 1.0),
                   _depth(3, 3, 65, 1.0, 60.0, 13), preset=7))
    T.append(_case("column over two words 33x2x40, 7x5", (33, 2, 40), 7, 5, 1, 1, axis_aligned((16.5, 0.5, 0.0)), (2.0, 6.0, 3.0, 2.0), _depth(1, 5, 7, 1.0, 50.0, 14)))
    # --- the model's matrix with correction_angle, and the processor's ---
    ext_small = (16.0, 16.0, 6.0)
    T.append(_case("model 8x8x4, 24x16", (8, 8, 4), 24, 16, 2, 1, model_matrix((8, 8, 4), ext_small, (7.0, 0.0, 0.0)), (20.0, 20.2, -1.7, -2.2),
                   _depth(2, 16, 24, 0.5, 9.0, 15), z_near=0.1, preset=9))
    T.append(_case("model 5x7x3 rotated, 7x5, step 3", (5, 7, 3), 7, 5, 3, 3, model_matrix((5, 7, 3), (10.0, 9.0, 7.0), (7.0, -3.0, 5.0)), (6.0, 6.1, -0.7, 0.2),
                   _depth(3, 5, 7, 0.5, 12.0, 16), max_depth=8.0))
    shift, scale = (100.0, 40.0, 0.0), (500.0, 2500.0, 200.0)
    T.append(_case("processor 33x2x40, 24x16, step 2", (33, 2, 40), 24, 16, 2, 2,
                   processor_matrix((33, 2, 40), (128.0, 128.0, 48.0), scale, shift, (7.0, 0.0, 0.0)), (30.0, 30.3, 11.7, 8.2),
                   _depth(2, 16, 24, 0.02, 0.12, 17), z_near=0.001))
    T.append(_case("processor 256x256x32, 7x5", (256, 256, 32), 7, 5, 2, 1,
                   processor_matrix((256, 256, 32), (128.0, 128.0, 32 / 0.666), scale, shift, (7.0, 3.0, -2.0)), (9.0, 9.1, 3.2, 2.2),
                   _depth(2, 5, 7, 0.02, 0.3, 18, specials=False), max_depth=0.25, preset=3))
    T.append(_case("model 256x256x32, 65x3, step 2", (256, 256, 32), 65, 3, 3, 2, model_matrix((256, 256, 32), (128.0, 128.0, 32 / 0.666), (7.0, 0.0, 0.0)),
                   (40.0, 41.0, -3.0, 1.2), _depth(3, 3, 65, 1.0, 90.0, 19), z_near=0.5))
    T.append(_case("model 256x256x32, 64x1", (256, 256, 32), 64, 1, 1, 1, model_matrix((256, 256, 32), (128.0, 128.0, 32 / 0.666), (7.0, -3.0, 5.0)),
                   (25.0, 25.0, -20.0, -10.0), _depth(1, 1, 64, 5.0, 60.0, 20)))
    return T


PLACEMENTS = ("inside the box", "outside the box with a clipped entry", "misses the box", "ends before the box", "ends beyond the box")


def placements(case):
    """Which of the camera placements the issue names occur among the rays of a case -> set of names."""
    g, found = case["g"], set()
    inside = lambda P: all(0.0 <= P[a] < g[a] for a in range(3))
    with np.errstate(all="ignore"):
        for r in range(case["rows"]):
            for v in cast_pixels(case["H"], case["step"]):
                for u in cast_pixels(case["W"], case["step"]):
                    d = case["depth"][r, v, u]
                    sd = segment(case["N"], case["K"], case["z_near"], case["max_depth"], u, v, d)
                    if sd is None:
                        continue
                    S, _, E = sd
                    got = cast_ray(case["N"], case["K"], g, case["z_near"], case["max_depth"], u, v, d)
                    if inside(S):
                        found.add(PLACEMENTS[0])
                    elif got:
                        found.add(PLACEMENTS[1])
                    elif cast_ray(case["N"], case["K"], g, case["z_near"], 0.0, u, v, np.float32(d) * np.float32(4096.0)):
                        found.add(PLACEMENTS[3])      # the same ray, prolonged, reaches the box
                    else:
                        found.add(PLACEMENTS[2])
                    if got and not inside(E):
                        found.add(PLACEMENTS[4])
    return found


TABLE = _table()
BY_NAME = {c["name"]: c for c in TABLE}
