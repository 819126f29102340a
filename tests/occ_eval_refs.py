"""numpy specification of the occupancy-evaluation layer (soccdpt_amd/utils/occupancy.py, csrc/occ_eval.hip).  tests/test_occ_eval_cpu.py pins it
bit for bit to lists recorded from the reference's own occupancy_grid_to_points / transform_points_to_occupancy_grid_vect
(tests/golden/occ_points.npz); the GPU tests and tools/occ_eval_bench.py compare the kernels with it.

Bit layout: cell n = row-major index of [g0,g1,g2,C], class n % C, bit n & 31 of little-endian word n >> 5."""
import numpy as np


def occupancy_shape_f32(grid_size, scale):
    return np.array([float(grid_size[i] / scale[i]) for i in range(3)], dtype=np.float32)


def pack_bits(mask):
    """bool [..ncell] (flattened) -> uint32 words, padding bits zero."""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    by = np.packbits(m, bitorder="little")
    by = np.concatenate([by, np.zeros((-by.size) % 4, dtype=np.uint8)])
    return by.view("<u4").astype(np.uint32)


def unpack_bits(words, ncell):
    """uint32 / int32 words -> bool [ncell]; bits at or beyond ncell are ignored."""
    w = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.uint32).astype("<u4")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:ncell].astype(bool)


def points_from_mask(mask, grid_size, scale, num_classes):
    """bool [ncell] (or [g0,g1,g2,C]) -> float64 [N,4] (x, y, z, class_id): sorted by (class, cell); x = f32(f64(i) / g0 * f64(shape_f32[0]))."""
    g = [int(v) for v in grid_size[:3]]
    C = int(num_classes)
    n = np.flatnonzero(np.asarray(mask, dtype=bool).reshape(-1)).astype(np.int64)
    cls, cell = n % C, n // C
    order = np.lexsort((cell, cls))
    cls, cell = cls[order], cell[order]
    idx = np.stack([cell // (g[1] * g[2]), (cell // g[2]) % g[1], cell % g[2]], axis=1)          # int64 [N,3]
    shape = occupancy_shape_f32(g, scale)
    xyz = (idx.astype(np.float64) / np.array(g, dtype=np.float64) * shape.astype(np.float64)).astype(np.float32)
    out = np.empty((n.size, 4), dtype=np.float64)
    out[:, :3] = xyz
    out[:, 3] = cls
    return out


def points_from_bits(words, grid_size, scale, num_classes):
    g = [int(v) for v in grid_size[:3]]
    return points_from_mask(unpack_bits(words, g[0] * g[1] * g[2] * int(num_classes)), g, scale, num_classes)


def class_counts(mask, num_classes):
    n = np.flatnonzero(np.asarray(mask, dtype=bool).reshape(-1))
    return np.bincount(n % num_classes, minlength=num_classes).astype(np.int64)


def iou_counts(pred_mask, gt_mask, num_classes):
    """bool [ncell] each -> int64 [C,4] (intersection, union, pred, gt)."""
    p = np.asarray(pred_mask, dtype=bool).reshape(-1, num_classes)
    g = np.asarray(gt_mask, dtype=bool).reshape(-1, num_classes)
    return np.stack([(p & g).sum(0), (p | g).sum(0), p.sum(0), g.sum(0)], axis=1).astype(np.int64)


def iou_from_counts(counts):
    """int64 [..,C,4] -> (iou_per_class [..,C], iou_3D [..]) in float64: inter / (union + 1e-7), mean over the classes."""
    c = np.asarray(counts).astype(np.float64)
    iou = c[..., 0] / (c[..., 1] + 1e-7)
    return iou, iou.mean(axis=-1)
