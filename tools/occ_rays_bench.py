"""What the observed-space mask and the IoU over it cost (DESIGN.md section 12.6 quotes the figures; profiles/occ_rays_cost.json records them).
Shape: B = 8 frames of 1920 x 1080, grid 256 x 256 x 32 x 3 classes.  The depth maps are the ones eval_SOccDPT --occupancy-observed casts: `depth` of
OccupancyProcessor.process on the synthetic validation frames (the upper half hidden, as the generator leaves it).  The protocol is
tools/batch_targets_bench.py's: HIP events, 20 warm-up calls, the cases alternating in 5 blocks of 100 calls inside one process, each figure the mean
over the blocks with their minimum and maximum.

  rays step 1 / 2 / 4     soccdpt_occ_rays_observed alone (clear = 1: the 2 MB memset of the mask is inside), rays per second, and the share of the
                          voxels step 1 observes that step 2 and step 4 lose
  iou_masked              soccdpt_occ_iou_counts_masked (8 predictions against 8 ground-truth rows, 8 masks, include_gt) beside soccdpt_occ_iou_counts
  the two yardsticks, in the same run:
    gt_occupancy          soccdpt_gt_occupancy on the same frames (depth + counts + grid, no point list): the launch that reads the same pixels and
                          scatters one atomic per run of pixels; the caster walks a whole ray per pixel
    depth_read            torch.sum of the depth maps: the time to merely read the 66 MB the caster reads

Nothing is asserted about time: the numbers are reported, not gated.

    python tools/occ_rays_bench.py [--json profiles/occ_rays_cost.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from soccdpt_amd.lib import _call, _ptr, csrc_sha  # noqa: E402
from soccdpt_amd.utils import occupancy_rays as O  # noqa: E402
from soccdpt_amd.utils.occupancy import pack_occupancy  # noqa: E402
from tools.batch_targets_bench import alternate, dev  # noqa: E402

ROWS, C = 8, 3
STEPS = (1, 2, 4)


def frames():
    """-> (processor, disparity [8,H,W] f32, class ids [8,H,W] int32) of the synthetic validation set, and the model's packed per-frame grids."""
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.scripts.eval_SOccDPT import synthetic_val_set
    from soccdpt_amd.utils.gt_occupancy import OccupancyProcessor
    from soccdpt_amd.utils.synth import synth_state_dict, write_synth_calib
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    net = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, occupancy_per_frame=True, num_classes=C)
    net.load_state_dict(synth_state_dict(alias_pretrained=True), strict=False)
    net = net.eval().to(dev)
    items = synthetic_val_set(net, dev, 256, n=ROWS)
    disp = torch.cat([it[3] for it in items]).to(device=dev, dtype=torch.float32).contiguous()
    seg = torch.cat([it[-1] for it in items]).to(dev).argmax(dim=1).to(torch.int32).contiguous()
    with torch.no_grad():
        net(torch.cat([it[0] for it in items]).to(dev))
    proc = OccupancyProcessor(intrinsic_matrix=net.intrinsic_matrix, height=net.height, width=net.width, grid_size=net.grid_size, scale=net.scale, shift=net.shift,
                              pc_scale=net.pc_scale, pc_shift=net.pc_shift, point_count_threshold=10.0, num_classes=C, correction_angle=net.correction_angle)
    return proc, disp, seg, net.last_occ_frame_bits.clone()


def popcount(mask: torch.Tensor) -> int:
    shifts = torch.arange(32, dtype=torch.int32, device=mask.device)
    return int(((mask.unsqueeze(-1) >> shifts) & 1).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    sha = lambda p: hashlib.sha1(open(os.path.join(REPO, p), "rb").read()).hexdigest()[:16]
    proc, disp, seg, pred_bits = frames()
    g, H, W = proc.grid_size, proc.height, proc.width
    out = dict(device=torch.cuda.get_device_name(0), grid=list(g), C=C, rows=ROWS, camera=[W, H], csrc_sha=csrc_sha(),
               occ_rays_hip_sha=sha("soccdpt_amd/csrc/occ_rays.hip"), occ_rays_core_sha=sha("soccdpt_amd/csrc/occ_rays_core.h"))
    gt = proc.process(disp, seg, want_points=False)
    depth, gt_bits = gt["depth"], pack_occupancy(gt["occupancy_grid"])
    valid = torch.isfinite(depth) & (depth > 0)
    out["pixels_with_depth_share"] = float(valid.float().mean().item())
    out["depth_m_min_median_max"] = [float(v) for v in (depth[valid].min(), depth[valid].median(), depth[valid].max())]
    N, K = O.camera_to_voxel(proc.voxel_to_camera()), np.array([proc.fx, proc.fy, proc.cx, proc.cy])
    nvw, nvox = O.mask_words(g), g[0] * g[1] * g[2]
    masks = {s: torch.empty((ROWS, nvw), dtype=torch.int32, device=dev) for s in STEPS}
    cast = lambda s: O.observed_voxels_raw(depth, N, K, g, 0.0, None, s, masks[s], True)
    for s in STEPS:
        cast(s)
    seen = {s: popcount(masks[s]) for s in STEPS}
    out["observed_voxels_per_row"] = {str(s): seen[s] / ROWS for s in STEPS}
    out["observed_fraction"] = {str(s): seen[s] / (ROWS * nvox) for s in STEPS}
    out["lost_share_of_step1"] = {str(s): popcount(masks[1] & ~masks[s]) / max(seen[1], 1) for s in STEPS[1:]}
    res = O.occupancy_iou_observed(pred_bits, gt_bits, masks[1], num_classes=C, grid_size=g)
    out["gt_voxels_outside_the_rays_share"] = float(1.0 - popcount(masks[1]) / max(int(res["observed_voxels"].sum().item()), 1))

    counts = torch.empty((ROWS, C, 4), dtype=torch.int64, device=dev)
    nobs = torch.empty((ROWS,), dtype=torch.int64, device=dev)
    d32 = disp.contiguous()
    gdepth = torch.empty_like(depth)
    gcounts = torch.empty((ROWS,) + tuple(g) + (C,), dtype=torch.int32, device=dev)
    gocc = torch.empty((ROWS,) + tuple(g) + (C,), dtype=torch.uint8, device=dev)
    arr = lambda vals, t: (t * len(vals))(*vals)
    gt_args = (ROWS, H, W, C, arr([proc.fx, proc.fy, proc.cx, proc.cy, proc.baseline], ctypes.c_double), arr(proc.pc_scale, ctypes.c_double),
               arr(proc.pc_shift, ctypes.c_double), arr([float(v) for v in proc._rot], ctypes.c_double), arr([float(v) for v in proc.occupancy_shape], ctypes.c_float),
               arr(list(g), ctypes.c_int), proc.point_count_threshold, _ptr(d32), _ptr(seg), _ptr(gdepth), None, _ptr(gcounts), _ptr(gocc))
    cases = {f"rays_step{s}": (lambda s=s: cast(s)) for s in STEPS}
    cases.update({
        "iou_masked": lambda: _call("soccdpt_occ_iou_counts_masked", _ptr(pred_bits), ROWS, _ptr(gt_bits), ROWS, nvox, C, _ptr(masks[1]), ROWS, 1, _ptr(counts), _ptr(nobs),
                                    device=dev),
        "occ_iou_counts": lambda: _call("soccdpt_occ_iou_counts", _ptr(pred_bits), ROWS, _ptr(gt_bits), ROWS, nvox * C, C, _ptr(counts), device=dev),
        "gt_occupancy": lambda: _call("soccdpt_gt_occupancy", *gt_args, device=dev),
        "depth_read": lambda: depth.sum(),
    })
    out["device_us"] = alternate(cases)
    for k, v in out["device_us"].items():
        print(f"{k:16s} {v['mean']:9.1f} us [{v['min']:.1f}-{v['max']:.1f}]")
    us = {k: v["mean"] for k, v in out["device_us"].items()}
    out["rays_cast"] = {str(s): ROWS * len(range(s // 2, W, s)) * len(range(s // 2, H, s)) for s in STEPS}
    out["rays_with_depth"] = {str(s): int(valid[:, s // 2::s, s // 2::s].sum().item()) for s in STEPS}
    out["rays_with_depth_per_s"] = {str(s): out["rays_with_depth"][str(s)] / (us[f"rays_step{s}"] * 1e-6) for s in STEPS}
    out["rays_step1_over_gt_occupancy"] = us["rays_step1"] / us["gt_occupancy"]
    out["rays_step1_over_depth_read"] = us["rays_step1"] / us["depth_read"]
    out["iou_masked_over_occ_iou_counts"] = us["iou_masked"] / us["occ_iou_counts"]
    for k in ("observed_fraction", "lost_share_of_step1", "rays_with_depth_per_s", "rays_step1_over_gt_occupancy", "rays_step1_over_depth_read",
              "iou_masked_over_occ_iou_counts", "gt_voxels_outside_the_rays_share", "pixels_with_depth_share", "depth_m_min_median_max"):
        print(k, out[k])
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
        print("wrote", args.json)


if __name__ == "__main__":
    main()
