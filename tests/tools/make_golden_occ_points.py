"""Generates tests/golden/occ_points.npz by running THE REFERENCE'S OWN occupancy_grid_to_points (SOccDPT/utils/__init__.py:532-568) and
OccupancyProcessor.transform_points_to_occupancy_grid_vect (SOccDPT/datasets/bdd_helper.py:289-362) on seeded inputs.  It needs the reference
checkout next to this repository (the stub recipe for its optional imports is oracle/make_golden.py import_reference), so it runs where the other
goldens are generated, never as part of the test suite; the file it writes is data (inputs as packed bits, outputs as recorded).

    python tests/tools/make_golden_occ_points.py

Model side (`<case>_bits`, `<case>_grid`, `<case>_scale`, `<case>_points`): the grid is stored as packed little-endian bits (cell n = row-major
index of [g0,g1,g2,C] -> bit n & 31 of word n >> 5); the reference saw the dense f32 grid those bits expand to.  `small` has 315 cells: its last
word carries padding bits that are SET in the file on purpose (consumers must ignore them).
GT side (`gt_points`): the `occupancy_points` value transform_points_to_occupancy_grid_vect returned inside process_frame on the frame of
tests/golden_inputs.py gt_occ_inputs() at point_count_threshold = 10, before process_frame un-rotates it for drawing."""
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from oracle.make_golden import import_reference  # noqa: E402
from tests.golden_inputs import gt_occ_inputs  # noqa: E402
from tests.occ_eval_refs import pack_bits  # noqa: E402

CASES = {   # name: (grid_size, scale, num_classes, density, seed)
    "default": ((256, 256, 32), (2.0, 2.0, 0.666), 3, 0.003, 101),
    "odd": ((48, 40, 12), (2.0, 2.0, 0.666), 3, 0.30, 102),
    "small": ((5, 7, 3), (1.5, 0.7, 0.666), 3, 0.50, 103),
    "empty": ((16, 8, 4), (2.0, 2.0, 0.666), 3, 0.0, 104),
}


def main():
    import_reference()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, **k: it
    from SOccDPT.utils import occupancy_grid_to_points
    out = {}
    for name, (grid, scale, C, density, seed) in CASES.items():
        rng = np.random.default_rng(seed)
        mask = rng.random(grid + (C,)) < density
        dense = mask.astype(np.float32)
        pts = occupancy_grid_to_points(dense, grid_size=grid, scale=scale, shift=(0.0, 0.0, 0.0))
        assert pts.dtype == np.float64 and pts.shape == (int(mask.sum()), 4)
        words = pack_bits(mask)
        tail = mask.size & 31
        if tail:
            words[-1] |= np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF)      # padding bits set on purpose
        out[name + "_bits"] = words
        out[name + "_grid"] = np.array(grid + (C,), dtype=np.int64)
        out[name + "_scale"] = np.array(scale, dtype=np.float64)
        out[name + "_points"] = pts
        print(name, grid, "rows", pts.shape[0])

    # ---- GT side: the reference's OccupancyProcessor on the frame the GT-occupancy golden uses ----
    cv2 = sys.modules["cv2"]
    cv2.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])
    spec = importlib.util.spec_from_file_location("ref_bdd_helper", os.path.join(os.path.dirname(REPO), "reference", "SOccDPT", "datasets", "bdd_helper.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    disparity, seg_class, K, H, W, C = gt_occ_inputs()
    colors = {c: (40 * c + 10, 40 * c + 10, 40 * c + 10) for c in range(C)}
    seg_frame = np.zeros((H, W, 3), dtype=np.uint8)
    for c, col in colors.items():
        seg_frame[seg_class == c] = col
    proc = ref.OccupancyProcessor(intrinsic_matrix=K, height=H, width=W, grid_size=(256, 256, 32), scale=(2.0, 2.0, 0.666), shift=(0.0, 0.0, 0.0),
                                  pc_scale=(500.0, 2500.0, 200.0), pc_shift=(100.0, 40.0, 0.0), point_count_threshold=10,
                                  class_2_color=dict(colors), color_2_class={v: k for k, v in colors.items()}, num_classes=C)
    seen = {}
    inner = proc.transform_points_to_occupancy_grid_vect

    def recording(points, semantics):
        r = inner(points, semantics)
        seen["points"] = np.array(r["occupancy_points"], copy=True)       # process_frame rotates this list in place afterwards
        seen["grid"] = np.array(r["occupancy_grid"], copy=True)
        return r
    proc.transform_points_to_occupancy_grid_vect = recording
    proc.process_frame(dict(rgb_frame=np.zeros((H, W, 3), dtype=np.uint8), disparity_frame=disparity.copy(), seg_frame=seg_frame))
    assert seen["points"].dtype == np.float64
    out["gt_points"] = seen["points"]
    out["gt_grid_cells"] = np.array([int(seen["grid"].sum())])
    print("gt rows", seen["points"].shape[0], "cells of the > grid", int(seen["grid"].sum()))
    path = os.path.join(REPO, "tests", "golden", "occ_points.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
