"""What the occupancy grid pictures cost, one line per entry point (DESIGN.md section 12.5 quotes them; profiles/occ_view_cost.json records them).
Default geometry: grid 256 x 256 x 32 x 3 classes, rows = 8, camera 1920 x 1080.  The protocol is tools/batch_targets_bench.py's: HIP events, 20 warm-up
calls, 5 blocks of 100 calls per case; host cases by wall clock, 3 blocks of 3 calls, the device synchronised before the clock stops.  The grid is
synthetic: a ground sheet of class 1 that rises with depth, seeded boxes of class 2, and 0.2 % seeded cells of class 0.

  columns / paint / iou2d / splat / resolve   each entry point of include/soccdpt_occ_view.h alone
  bird_eye_view, occupancy_overlay, bev_iou    the Python functions (allocation and table upload included)
  host recipe                                   what these replace: the dense grid [8,256,256,32,3] f32 copied to the host, reduced along axis 1 with
                                                numpy (any / argmax) and coloured by a table lookup; and, for the overlay, np.argwhere of row 0 and the
                                                matrix product that brings its cells to pixels (no drawing: a lower bound)

Nothing is asserted about time: the numbers are reported, not gated.

    python tools/occ_view_bench.py [--json profiles/occ_view_cost.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from soccdpt_amd.lib import _call, _ptr, csrc_sha, host_rotation_matrices  # noqa: E402
from soccdpt_amd.utils import occupancy_views as V  # noqa: E402
from soccdpt_amd.utils.occupancy import pack_occupancy  # noqa: E402
from tools.batch_targets_bench import HOST_BLOCKS, HOST_CALLS, alternate, dev, stat, wall  # noqa: E402

GRID, C, ROWS, H, W = (256, 256, 32), 3, 8, 1080, 1920
COLORS = ((0, 0, 0), (0, 0, 142), (220, 20, 60))
K = np.array([1250.6, 1254.8, 978.4, 562.1])


def synthetic_grid(seed: int = 0) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    d = np.zeros((ROWS,) + GRID + (C,), dtype=bool)
    d[..., 0] = rng.random((ROWS,) + GRID) < 0.002
    i0, i2 = np.meshgrid(np.arange(GRID[0]), np.arange(GRID[2]), indexing="ij")
    for r in range(ROWS):
        d[r, i0, np.clip(12 - i2 // 4 + r, 1, GRID[1] - 1), i2, 1] = True
        for _ in range(12):
            a, b, c = rng.integers(100, 156), rng.integers(4, 12), rng.integers(2, 28)
            d[r, a:a + 6, b:b + 5, c:c + 3, 2] = True
    return torch.from_numpy(d.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    sha = lambda p: hashlib.sha1(open(os.path.join(REPO, p), "rb").read()).hexdigest()[:16]
    out = dict(device=torch.cuda.get_device_name(0), grid=list(GRID), C=C, rows=ROWS, camera=[W, H], csrc_sha=csrc_sha(),
               occ_view_hip_sha=sha("soccdpt_amd/csrc/occ_view.hip"), occupancy_views_py_sha=sha("soccdpt_amd/utils/occupancy_views.py"))
    dense = synthetic_grid().to(dev)
    bits = pack_occupancy(dense)
    out["set_bits_per_row"] = float(dense.sum().item() / ROWS)
    M = V.model_voxel_to_camera(GRID, (128.0, 128.0, 32 / 0.666), host_rotation_matrices((7.0, 0.0, 0.0)))
    M[:, 3] = (-64.0, -8.0, 0.0)        # the camera in the middle of the X range, 8 m above the grid's low Y face
    half = V.default_half_extent(M)
    frames = torch.randint(0, 256, (ROWS, H, W, 3), dtype=torch.uint8, device=dev)
    table = V._table(COLORS, C, dev)
    g3 = (ctypes.c_int32 * 3)(*GRID)
    A, B = GRID[0], GRID[2]
    cols = V._columns(bits, GRID, C, 1, False)
    zbuf = V.occupancy_zbuffer(bits, GRID, C, M, K, half, 12, 0.1, H, W)
    out["overlay_pixels_hit_per_row"] = float((zbuf != -1).sum().item() / ROWS)
    pic_bev, pic_cam = torch.empty((ROWS, B * 2, A * 2, 3), dtype=torch.uint8, device=dev), torch.empty((ROWS, H, W, 3), dtype=torch.uint8, device=dev)
    counts = torch.empty((ROWS, C, 4), dtype=torch.int64, device=dev)
    f64 = ctypes.POINTER(ctypes.c_double)
    bg = (ctypes.c_uint8 * 3)(32, 32, 32)
    cases = {
        "columns": lambda: _call("soccdpt_occ_view_columns", _ptr(bits), ROWS, g3, C, 1, 0, _ptr(cols["top"]), _ptr(cols["first"]), _ptr(cols["count"]),
                                 _ptr(cols["classes"]), device=dev),
        "paint": lambda: _call("soccdpt_occ_view_paint", _ptr(cols["top"]), _ptr(cols["first"]), ROWS, A, B, GRID[1], 0, _ptr(table), C, bg, 128, 2, 0, 1, 1, _ptr(pic_bev),
                               A * 2, 0, A * B * 4, ROWS * A * B * 4, device=dev),
        "iou2d": lambda: _call("soccdpt_occ_view_iou2d", _ptr(cols["classes"][:1].contiguous()), 1, _ptr(cols["classes"]), ROWS, A * B, C, _ptr(counts), device=dev),
        "splat": lambda: _call("soccdpt_occ_view_splat", _ptr(bits), ROWS, g3, C, M.ctypes.data_as(f64), K.ctypes.data_as(f64), half, 12, 0.1, H, W, _ptr(zbuf), device=dev),
        "resolve": lambda: _call("soccdpt_occ_view_resolve", _ptr(zbuf), _ptr(frames), ROWS, ROWS, H, W, C, _ptr(table), 160, _ptr(pic_cam), W, 0, H * W, ROWS * H * W,
                                 device=dev),
        "bird_eye_view": lambda: V.bird_eye_view(bits, GRID, COLORS, num_classes=C),
        "occupancy_overlay": lambda: V.occupancy_overlay(bits, frames, M, K, GRID, COLORS, num_classes=C),
        "bev_iou": lambda: V.bev_iou(bits[:1], bits, GRID, num_classes=C),
    }
    out["device_us"] = alternate(cases)
    for k, v in out["device_us"].items():
        print(f"{k:18s} {v['mean']:9.1f} us [{v['min']:.1f}-{v['max']:.1f}]")

    lut = np.array(COLORS + ((32, 32, 32),), dtype=np.uint8)

    def host_bev():
        d = dense.cpu().numpy() >= 0.5
        occ = d.any(axis=-1)
        first = occ.argmax(axis=2)
        at = np.take_along_axis(d, first[:, :, None, :, None], axis=2)[:, :, 0]
        top = np.where(occ.any(axis=2), C - 1 - at[..., ::-1].argmax(axis=-1), C)
        return lut[top]

    def host_project():
        idx = np.argwhere(dense[0].cpu().numpy() >= 0.5)
        P = (idx[:, :3] + 0.5) @ M[:, :3].T + M[:, 3]
        return np.floor(P[:, :2] / P[:, 2:3] * K[:2] + K[2:] + 0.5)

    host_bev(), host_project()
    hb, hp = [wall(host_bev, HOST_CALLS) for _ in range(HOST_BLOCKS)], [wall(host_project, HOST_CALLS) for _ in range(HOST_BLOCKS)]
    out["host_bev_ms"], out["host_project_row0_ms"] = stat(hb), stat(hp)
    out["host_bev_over_bird_eye_view"] = float(np.mean(hb) * 1e3 / out["device_us"]["bird_eye_view"]["mean"])
    print(f"host recipe, bird's-eye view of {ROWS} rows: {np.mean(hb):.0f} ms [{min(hb):.0f}-{max(hb):.0f}] = {out['host_bev_over_bird_eye_view']:.0f} x bird_eye_view")
    print(f"host recipe, cells of row 0 to pixels (no drawing): {np.mean(hp):.0f} ms [{min(hp):.0f}-{max(hp):.0f}]")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
