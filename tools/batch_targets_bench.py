"""What a training batch of Bengaluru frames costs, one line per case (DESIGN.md section 12.3 quotes them; profiles/batch_targets_cost.json records them).
B = 8 frames of 1080 x 1920, C = 3.  Device cases: HIP events, 20 warm-up calls, the sides of a comparison alternating in blocks inside one process, each
figure the mean over the blocks with their minimum and maximum.  Host cases: wall clock around the calls, the device synchronised before the clock stops.

  (a) host_recipe   the reference's per-item host recipe restated in numpy (three same-size cv2.resize copies, rgb_seg_to_bool, the float copies, torch.cat)
                    plus the .to(device) of its float / bool tensors (pageable memory, as the reference has it).  The input transform is not in it.
  (b) gpu_path      the datasets' device half on already decoded frames: uint8 frames staged in pinned memory and uploaded, the input transform launch and
                    the targets launch (BDD_Depth_Segmentation.assemble)
  (c) targets       soccdpt_data_targets alone (onehot + y_disp from u8 labels and u8 disparity), its bytes written per second beside occ_expand's (B = 8)
  (d) decode        host decode of the batch's 24 PNGs with 1, 8 and 16 pool workers

    python tools/batch_targets_bench.py [--json profiles/batch_targets_cost.json]
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from soccdpt_amd.lib import Engine, csrc_sha, make_config, op_data_targets  # noqa: E402
from soccdpt_amd.utils.occupancy import occupancy_shape_f32  # noqa: E402

B, H, W, C = 8, 1080, 1920, 3
GRID, SCALE = (256, 256, 32), (2.0, 2.0, 0.666)
WARM, BLOCK, BLOCKS = 20, 100, 5
HOST_BLOCKS, HOST_CALLS = 3, 3
STEP_MS = 15.9       # the B = 8 training step the batches have to feed (README)
COLORS = ((0, 0, 0), (0, 0, 142), (220, 20, 60))
dev = torch.device("cuda:0")


def stat(v):
    return dict(mean=float(np.mean(v)), min=float(np.min(v)), max=float(np.max(v)), blocks=[round(float(x), 3) for x in v])


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n       # us per call


def alternate(fns):
    for f in fns.values():
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(BLOCKS):
        for k, f in fns.items():
            per[k].append(timed(f, BLOCK))
    return {k: stat(v) for k, v in per.items()}


def wall(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n       # ms per call


def write_recording(root, rec_id, n):
    """n frames of 1080 x 1920 with the statistics that matter to a PNG decoder: a smooth picture with pixel noise, label blocks, a smooth disparity."""
    from PIL import Image
    rng = np.random.default_rng(0)
    d = os.path.join(root, rec_id)
    for sub in ("rgb_img", "depth_img", "seg_img"):
        os.makedirs(os.path.join(d, sub), exist_ok=True)
    palette = np.array(COLORS + ((7, 7, 7),), dtype=np.uint8)
    up = lambda a, k: np.repeat(np.repeat(a, k, axis=0), k, axis=1)[:H, :W]
    with open(os.path.join(d, rec_id + ".csv"), "w") as f:
        f.write("Index,Timestamp\n")
        for i in range(n):
            f.write(f"{i},{1000 + i}\n")
            lo = rng.integers(0, 256, size=(H // 8 + 1, W // 8 + 1, 3)).astype(np.int16)
            rgb = np.clip(up(lo, 8) + rng.integers(-6, 7, size=(H, W, 3)), 0, 255).astype(np.uint8)
            seg = palette[up(rng.integers(0, 4, size=(H // 40 + 1, W // 40 + 1)), 40)]
            disp = up(rng.integers(1, 256, size=(H // 16 + 1, W // 16 + 1)), 16).astype(np.uint8)
            Image.fromarray(rgb).save(os.path.join(d, "rgb_img", f"{1000 + i}.png"))
            Image.fromarray(seg).save(os.path.join(d, "seg_img", f"{1000 + i}.png"))
            Image.fromarray(disp).save(os.path.join(d, "depth_img", f"{1000 + i}.png"))
    return d


def host_recipe(frames):
    """The reference's BDD_Depth_Segmentation.__getitem__ for every frame (without the input transform), get_batch's torch.cat, the loop's .to(device)."""
    items = []
    for f in frames:
        rgb, seg, disp = f["rgb_frame"].copy(), f["seg_frame"].copy(), f["disparity_frame"].copy()      # cv2.resize to the size the frames already have
        seg_bool = np.zeros(seg.shape[:2] + (C,), dtype=bool)
        for c, color in enumerate(COLORS):
            seg_bool[:, :, c] = np.all(seg == np.array(color), axis=-1)
        y_disp = torch.tensor(disp).unsqueeze(0)
        y_seg = torch.tensor(seg_bool).unsqueeze(0).permute(0, 3, 1, 2)
        items.append((torch.tensor(rgb).unsqueeze(0), torch.ones_like(y_disp, dtype=torch.bool), y_disp, torch.ones_like(y_seg, dtype=torch.bool), y_seg))
    x_raw, mask_disp, y_disp, mask_seg, y_seg = [torch.cat([it[k] for it in items], dim=0) for k in range(5)]
    return (y_disp.to(device=dev, dtype=torch.float32), y_seg.to(device=dev, dtype=torch.float32), mask_disp.to(device=dev, dtype=torch.bool),
            mask_seg.to(device=dev, dtype=torch.bool))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    from soccdpt_amd.model.loader import load_transforms
    from soccdpt_amd.utils.synth import write_synth_calib
    root = tempfile.mkdtemp()
    calib = write_synth_calib(os.path.join(root, "calib.yaml"))
    write_recording(root, "1", B)
    t, _, _ = load_transforms("dpt_swin2_tiny_256")
    t.device = dev
    ds = D.BDD_Depth_Segmentation(dataset_path=os.path.join(root, "1"), settings_doc=calib, transform=t, device=dev)
    idx = list(range(B))
    out = dict(device=torch.cuda.get_device_name(0), B=B, camera=[W, H], C=C, csrc_sha=csrc_sha(),
               batch_targets_sha=hashlib.sha1(open(os.path.join(REPO, "soccdpt_amd", "csrc", "batch_targets.hip"), "rb").read()).hexdigest()[:16], step_ms=STEP_MS)

    # ---- (d) decode ----
    out["decode_ms"] = {}
    ds.decode(idx)
    per = {w: [] for w in (1, 8, 16)}
    for _ in range(HOST_BLOCKS):
        for w in per:
            ds.workers = w
            t0 = time.perf_counter()
            frames = ds.decode(idx)
            per[w].append((time.perf_counter() - t0) * 1e3)
    ds.workers = D.DEFAULT_WORKERS
    for w, v in per.items():
        out["decode_ms"][str(w)] = stat(v)
        print(f"(d) decode of {3 * B} PNGs, {w:2d} workers: {np.mean(v):.1f} ms [{min(v):.1f}-{max(v):.1f}] = {np.mean(v) / STEP_MS:.1f} x the {STEP_MS} ms step")

    # ---- (a) against (b) ----
    host_recipe(frames), ds.assemble(frames)
    pa, pb = [], []
    for _ in range(HOST_BLOCKS):
        pa.append(wall(lambda: host_recipe(frames), HOST_CALLS))
        pb.append(wall(lambda: ds.assemble(frames), HOST_CALLS))
    out["host_recipe_ms"], out["gpu_path_ms"] = stat(pa), stat(pb)
    got, ref = ds.assemble(frames), host_recipe(frames)
    assert torch.equal(got[3], ref[0]) and torch.equal(got[5], ref[1]), "the two recipes build different targets"
    print(f"(a) host recipe + .to(device): {np.mean(pa):.1f} ms [{min(pa):.1f}-{max(pa):.1f}] | (b) pinned uint8 upload + transform + targets: {np.mean(pb):.2f} ms "
          f"[{min(pb):.2f}-{max(pb):.2f}] | a / b = {np.mean(pa) / np.mean(pb):.1f}")

    # ---- (c) the targets launch beside occ_expand ----
    seg = torch.from_numpy(np.stack([f["seg_frame"] for f in frames])).to(dev)
    disp = torch.from_numpy(np.stack([f["disparity_frame"] for f in frames])).to(dev)
    colors = torch.tensor(COLORS, dtype=torch.uint8, device=dev)
    from soccdpt_amd.lib import _call, _ptr
    onehot = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    y_disp = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    unmatched = torch.empty((B,), dtype=torch.int64, device=dev)
    eng = Engine(make_config("swin2t16_256", C, 256, True, True, W, H, 1250.6, 1254.8, 978.4, 562.1, GRID, occupancy_shape_f32(GRID, SCALE),
                             (10000.0, 50000.0, 800.0), (55.0, -20.0, 15.0), (7.0, 0, 0)), dev)
    ncell = GRID[0] * GRID[1] * GRID[2] * C
    bits = torch.zeros(((ncell + 31) // 32,), dtype=torch.int32, device=dev)
    occ = torch.empty((B,) + GRID + (C,), dtype=torch.float32, device=dev)
    tt = alternate({
        "targets": lambda: _call("soccdpt_data_targets", _ptr(seg), _ptr(colors), C, _ptr(disp), 0, B, H, W, 0, _ptr(onehot), None, _ptr(y_disp), None, device=dev),
        "targets_with_unmatched": lambda: _call("soccdpt_data_targets", _ptr(seg), _ptr(colors), C, _ptr(disp), 0, B, H, W, 0, _ptr(onehot), None, _ptr(y_disp),
                                                 _ptr(unmatched), device=dev),
        "occ_expand": lambda: eng.occ_expand(bits, B, occ)})
    wr_t, wr_e = B * H * W * 4 * (C + 1), B * ncell * 4
    rate = lambda nbytes, s: nbytes / s["mean"] / 1e6      # TB/s
    out["targets_us"], out["targets_with_unmatched_us"], out["occ_expand_us"] = tt["targets"], tt["targets_with_unmatched"], tt["occ_expand"]
    out["targets_written_TBps"], out["occ_expand_written_TBps"] = rate(wr_t, tt["targets"]), rate(wr_e, tt["occ_expand"])
    out["targets_over_occ_expand_rate"] = out["targets_written_TBps"] / out["occ_expand_written_TBps"]
    print(f"(c) targets: {tt['targets']['mean']:.1f} us [{tt['targets']['min']:.1f}-{tt['targets']['max']:.1f}], {out['targets_written_TBps']:.2f} TB/s of the "
          f"{wr_t / 1e6:.0f} MB written (with the unmatched counters {tt['targets_with_unmatched']['mean']:.1f} us) | occ_expand B={B}: {tt['occ_expand']['mean']:.1f} us, "
          f"{out['occ_expand_written_TBps']:.2f} TB/s of {wr_e / 1e6:.0f} MB | rate ratio {out['targets_over_occ_expand_rate']:.2f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
