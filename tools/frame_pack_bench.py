"""What a frame pack saves, one line per case (DESIGN.md section 12.4 quotes them; profiles/frame_pack_cost.json records them).  The protocol and the
synthetic recording are those of tools/batch_targets_bench.py: B = 8 frames of 1080 x 1920, C = 3.  Device cases: HIP events, 20 warm-up calls, the
two sides alternating in 5 blocks of 100 calls.  Host cases: wall clock, 3 alternating blocks of 3 calls, the device synchronised before the clock
stops.  The files are in the page cache (written a moment ago): these are warm figures; cold reads are not measured.

  (a) batch         BDD_Depth_Segmentation.batch() from the PNGs against batch() from the pack of the same recording
  (b) targets       soccdpt_pack_targets against soccdpt_data_targets on the expanded labels (onehot + y_disp + unmatched)
  (c) upload bytes  per batch, PNG path and pack path
  (d) pack bytes    per frame on disk
  (e) packing       write_pack of the 8-frame recording, and --verify

    python tools/frame_pack_bench.py [--json profiles/frame_pack_cost.json]
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

from soccdpt_amd.lib import _call, _ptr, csrc_sha, op_pack_expand  # noqa: E402
from tools.batch_targets_bench import B, C, COLORS, H, HOST_BLOCKS, HOST_CALLS, W, alternate, dev, stat, wall, write_recording  # noqa: E402


def step_ms():
    """The bf16-amp B = 8 training step of profiles/r06_bench_train_step_amp.json, or None when the file does not say."""
    try:
        line = json.load(open(os.path.join(REPO, "profiles", "r06_bench_train_step_amp.json")))
    except (OSError, ValueError):
        return None
    for key in ("step_ms", "ms_per_step", "train_step_ms"):
        if isinstance(line, dict) and isinstance(line.get(key), (int, float)):
            return float(line[key])
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    from soccdpt_amd.datasets import bengaluru_driving_dataset as D
    from soccdpt_amd.datasets.frame_pack import verify_pack, write_pack
    from soccdpt_amd.model.loader import load_transforms
    from soccdpt_amd.utils.synth import write_synth_calib
    root = tempfile.mkdtemp()
    calib = write_synth_calib(os.path.join(root, "calib.yaml"))
    rec = write_recording(root, "1", B)
    t, _, _ = load_transforms("dpt_swin2_tiny_256")
    t.device = dev
    sha = lambda p: hashlib.sha1(open(os.path.join(REPO, "soccdpt_amd", p), "rb").read()).hexdigest()[:16]
    out = dict(device=torch.cuda.get_device_name(0), B=B, camera=[W, H], C=C, csrc_sha=csrc_sha(), frame_pack_hip_sha=sha("csrc/frame_pack.hip"),
               frame_pack_py_sha=sha("datasets/frame_pack.py"), page_cache="warm", step_ms=step_ms())

    # ---- (e) packing ----
    t0 = time.perf_counter()
    pack_file = write_pack(rec)
    out["write_pack_ms"] = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    assert verify_pack(rec) == B
    out["verify_pack_ms"] = (time.perf_counter() - t0) * 1e3
    print(f"(e) write_pack of {B} frames, {D.DEFAULT_WORKERS} workers: {out['write_pack_ms']:.0f} ms ({out['write_pack_ms'] / B:.0f} ms a frame); "
          f"--verify {out['verify_pack_ms']:.0f} ms")

    kw = dict(dataset_path=rec, settings_doc=calib, transform=t, device=dev)
    png, packed = D.BDD_Depth_Segmentation(**kw), D.BDD_Depth_Segmentation(frame_pack=True, frame_pack_required=True, **kw)
    pack = packed.pack
    idx = list(range(B))

    # ---- (d), (c) ----
    png_bytes = sum(os.path.getsize(os.path.join(rec, d, f)) for d in ("rgb_img", "depth_img", "seg_img") for f in os.listdir(os.path.join(rec, d)))
    out["pack_bytes_per_frame"] = os.path.getsize(pack_file) / B
    out["png_bytes_per_frame"] = png_bytes / B
    out["record_bytes"] = dict(zip(("rgb", "disparity", "labels"), pack.rec_bytes))
    out["label_bits"], out["palette_entries"] = pack.k, pack.P
    up_png = B * (H * W * 3 * 2 + H * W * pack.disp_dtype.itemsize)
    up_pack = B * sum(pack.rec_bytes)
    out["upload_bytes_per_batch"] = dict(png=up_png, pack=up_pack)
    print(f"(d) pack: {out['pack_bytes_per_frame'] / 1e6:.2f} MB a frame on disk (rgb {pack.rec_bytes[0] / 1e6:.2f} + disparity {pack.rec_bytes[1] / 1e6:.2f} + "
          f"labels {pack.rec_bytes[2] / 1e6:.2f} at {pack.k} bits, {pack.P} colours) against {out['png_bytes_per_frame'] / 1e6:.2f} MB of PNGs")
    print(f"(c) uploaded per batch: {up_png / 1e6:.1f} MB from PNGs, {up_pack / 1e6:.1f} MB from the pack")

    # ---- (a) batch() from PNGs against batch() from the pack ----
    a, b = png.batch(idx), packed.batch(idx)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(png.last_unmatched, packed.last_unmatched), "the two paths build different batches"
    pa, pb = [], []
    for _ in range(HOST_BLOCKS):
        pa.append(wall(lambda: png.batch(idx), HOST_CALLS))
        pb.append(wall(lambda: packed.batch(idx), HOST_CALLS))
    out["batch_png_ms"], out["batch_pack_ms"] = stat(pa), stat(pb)
    out["batch_png_over_pack"] = float(np.mean(pa) / np.mean(pb))
    out["pack_slowest_block_below_png_fastest"] = bool(max(pb) < min(pa))
    step = out["step_ms"]
    print(f"(a) batch() from PNGs: {np.mean(pa):.1f} ms [{min(pa):.1f}-{max(pa):.1f}] | from the pack: {np.mean(pb):.2f} ms [{min(pb):.2f}-{max(pb):.2f}] | "
          f"ratio {out['batch_png_over_pack']:.1f}" + (f" | the pack path is {np.mean(pb) / step:.2f} x the {step} ms step" if step else ""))

    # ---- (b) the targets launch from indices against the one from label frames ----
    frames = packed.decode(idx)
    idx_d = torch.from_numpy(np.stack([f["seg_index"] for f in frames])).to(dev)
    pal_d = torch.from_numpy(pack.palette).to(dev)
    disp = torch.from_numpy(np.stack([f["disparity_frame"] for f in frames])).to(dev)
    seg = op_pack_expand(idx_d, pack.k, pal_d, H, W)
    colors = torch.tensor(COLORS, dtype=torch.uint8, device=dev)
    code = {1: 0, 2: 1, 4: 2}[pack.disp_dtype.itemsize]
    outs = [(torch.empty((B, C, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W), dtype=torch.float32, device=dev),
             torch.empty((B,), dtype=torch.int64, device=dev)) for _ in range(2)]
    from_frames = lambda: _call("soccdpt_data_targets", _ptr(seg), _ptr(colors), C, _ptr(disp), code, B, H, W, 0, _ptr(outs[0][0]), None, _ptr(outs[0][1]),
                                _ptr(outs[0][2]), device=dev)
    from_indices = lambda: _call("soccdpt_pack_targets", _ptr(idx_d), pack.k, idx_d.shape[1], _ptr(pal_d), pack.P, _ptr(colors), C, _ptr(disp), code, B, H, W, 0,
                                 _ptr(outs[1][0]), None, _ptr(outs[1][1]), _ptr(outs[1][2]), device=dev)
    tt = alternate({"data_targets": from_frames, "pack_targets": from_indices})
    assert all(torch.equal(x, y) for x, y in zip(*outs)), "the two launches build different targets"
    out["data_targets_us"], out["pack_targets_us"] = tt["data_targets"], tt["pack_targets"]
    out["pack_over_data_targets"] = tt["pack_targets"]["mean"] / tt["data_targets"]["mean"]
    out["targets_bytes"] = dict(written=B * H * W * 4 * (C + 1), read_data=B * H * W * (3 + pack.disp_dtype.itemsize),
                                read_pack=B * (pack.rec_bytes[2] + H * W * pack.disp_dtype.itemsize))
    print(f"(b) soccdpt_data_targets: {tt['data_targets']['mean']:.1f} us [{tt['data_targets']['min']:.1f}-{tt['data_targets']['max']:.1f}] | "
          f"soccdpt_pack_targets: {tt['pack_targets']['mean']:.1f} us [{tt['pack_targets']['min']:.1f}-{tt['pack_targets']['max']:.1f}] | "
          f"pack / data = {out['pack_over_data_targets']:.3f}")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)
    assert out["pack_slowest_block_below_png_fastest"], "the pack path's slowest block is not faster than the PNG path's fastest: a defect"


if __name__ == "__main__":
    main()
