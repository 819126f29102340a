"""Counterpart of the reference's evaluation entry point (`/root/reference/SOccDPT/scripts/eval_SOccDPT.py`,
invoked by `scripts/eval.sh:3-13` as `python -m SOccDPT.scripts.eval_SOccDPT -v 3 -dt bdd -t dpt_swin2_tiny_256 ...`):
same flags, same protocol — load the model through `load_model`, run the FPS loop (50 forwards,
eval_SOccDPT.py:246-259), then `evaluate_seg` / `evaluate_depth` on the validation subset and print the same lines.

An existing `--base_path` evaluates the reference's ten-frame subset of the Bengaluru recordings under it (`random_split(dataset, [10, n - 10])`
with generator seed 0, eval_SOccDPT.py:126-135) through soccdpt_amd/datasets/: uint8 frames uploaded, targets and the ground-truth class map built on the
GPU (csrc/batch_targets.hip).

Differences, all forced by what exists on a GPU box: when `--base_path`
does not exist the 10-image validation subset is synthetic (seeded frames, ground truth = a smooth perturbation of
the CPU-free model output, so the numbers are meaningful only as a smoke/regression signal); the PNG visual dumps of
eval_SOccDPT.py:136-243 are opt-in (`--visuals [DIR]`, default off; see write_visuals); the FPS loop synchronises the stream before stopping the clock (the reference does
not); metrics run on the GPU (soccdpt_amd.utils.metrics).  `-l/--load` may be omitted for random weights.

    python -m soccdpt_amd.scripts.eval_SOccDPT -v 3 -dt bdd -t dpt_swin2_tiny_256 -d cuda:0 [-l ckpt.pth] [-o] [--visuals [DIR]] [--occupancy-views [DIR]] [--occupancy-observed]
"""
import argparse
import os
import random
import tempfile
import time

import numpy as np
import torch

from ..model.loader import load_model, load_transforms
from ..model.SOccDPT import DepthNet, SegNet, SOccDPT_versions, model_types
from ..utils.metrics import evaluate_depth, evaluate_seg
from ..utils.synth import synth_input, synth_state_dict, write_synth_calib


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Evaluate SOccDPT")
    parser.add_argument("-v", "--version", choices=[1, 2, 3], required=True, type=int, help="SOccDPT version")
    parser.add_argument("-dt", "--dataset", choices=["bdd", "idd"], required=True, help="Dataset to evaluate on")
    parser.add_argument("-t", "--model_type", choices=model_types, required=True, help="Model architecture to use")
    parser.add_argument("-d", "--device", default="cpu", help="Device (the HIP path needs cuda:N; cpu raises like any missing-GPU use)")
    parser.add_argument("-l", "--load", default=None, help="Checkpoint path (omit: deterministic synthetic weights)")
    parser.add_argument("-cm", "--compile", action="store_true", help="accepted for compatibility; the HIP path has no tracing compiler")
    parser.add_argument("-o", "--optimize", action="store_true", help="fp16 operands (the reference's net.half())")
    parser.add_argument("-b", "--base_path", default=os.path.expanduser("~/Datasets/Depth_Dataset_Bengaluru"), help="Base path to dataset")
    parser.add_argument("-ld", "--load_depth", default=None, help="Which depth checkpoint to load")
    parser.add_argument("-ls", "--load_seg", default=None, help="Which seg checkpoint to load")
    parser.add_argument("--camera_intrinsics_yaml", default=None, help="calibration file (default: the synthetic 1920x1080 camera of SURVEY.md 8d)")
    parser.add_argument("--recordings", nargs="*", default=None, help="recording ids under --base_path (default: the reference's six)")
    parser.add_argument("--frame_pack", nargs="?", const=True, default=None, metavar="DIR", help="read the recordings' frame packs (<id>.sfp, written by "
                        "python -m soccdpt_amd.scripts.pack_recordings) instead of decoding their PNGs; bare flag: the pack inside each recording, DIR: "
                        "a directory of packs.  A missing or stale pack warns and falls back to the PNGs")
    parser.add_argument("--frame_pack_required", action="store_true", help="with --frame_pack: a missing or stale pack is an error")
    parser.add_argument("--occupancy", action="store_true", help="also evaluate the semantic occupancy grid on the GPU: 3-D IoU against the ground-truth "
                        "grid of OccupancyProcessor and the mean length of the occupancy point list (prints IOU_3D / OCC_POINTS)")
    parser.add_argument("--occupancy-per-frame", dest="occupancy_per_frame", action="store_true", help="implies --occupancy, with the model built with "
                        "occupancy_per_frame=True: every frame's own grid (not the union over the batch) is scored against that frame's ground truth, "
                        "and OCC_POINTS is the mean point-list length per frame")
    parser.add_argument("--occupancy-observed", dest="occupancy_observed", action="store_true", help="implies --occupancy; also score the grid over observed "
                        "space only: the voxels the rays of the ground truth's depth map cross, plus its occupied voxels (prints IOU_3D_OBSERVED / "
                        "OBSERVED_FRACTION beside the unchanged IOU_3D)")
    parser.add_argument("--visuals", nargs="?", const=os.path.join("media", "visuals"), default=None, metavar="DIR", help="also write the reference's PNG "
                        "dumps of the validation frames (RGB, GT_Depth, GT_Seg, Pred_Depth, Pred_Seg) and the evaluation panel under "
                        "DIR/{model_type}_{dataset}_{version}/ (bare flag: media/visuals), coloured on the GPU")
    parser.add_argument("--occupancy-views", dest="occupancy_views", nargs="?", const=os.path.join("media", "occupancy_views"), default=None, metavar="DIR",
                        help="implies --occupancy; also write pictures of the occupancy grid of every validation frame under DIR/{Occ_BEV,Occ_Overlay,Occ_Panel}/ "
                        "(bare flag: media/occupancy_views): the grid from above and over the camera frame, prediction left, ground truth right "
                        "(the frame's own grid with --occupancy-per-frame), and print their mean 2-D IoU (BEV_IOU)")
    return parser


# class -> colour of the 3-class bdd layout, in the channel order of the frames (datasets/bengaluru_driving_dataset.py:59-64)
CLASS_2_COLOR_BDD = {0: (0, 0, 0), 1: (0, 0, 142), 2: (220, 20, 60)}
VISUAL_DIRS = ("RGB", "GT_Depth", "GT_Seg", "Pred_Depth", "Pred_Seg", "Panel")
OCCUPANCY_VIEW_DIRS = ("Occ_BEV", "Occ_Overlay", "Occ_Panel")


def write_visuals(net, dataset, device, root: str, class_2_color=None) -> str:
    """The PNG dumps of the reference's evaluation script (eval_SOccDPT.py:138-244) for every frame of `dataset`, plus the evaluation panel:
    root/{RGB,GT_Depth,GT_Seg,Pred_Depth,Pred_Seg,Panel}/000N.png.  Depth pictures are the per-frame normalised inverse depth through the plasma table,
    class pictures color_segmentation; everything is coloured on the GPU (utils/visualise.py) and only the finished u8 pictures are copied to the host
    for the PNG encoder.  GT_Seg is drawn from y_seg: the reference draws y_seg_pred there too (eval_SOccDPT.py:205-217, the same lines as its
    Pred_Seg block), an evident slip that would make the two folders identical.  A sample without a raw frame (the synthetic subset) gets one made of
    its network input: de-normalised, B <-> R swapped, resized to the camera size.  Every frame is run through the model once more here, after
    evaluate_seg and evaluate_depth have already done so: the dump is opt-in and ten frames long, and keeping it apart leaves those two loops as
    they are."""
    from ..utils.visualise import color_masks, colorize_disparity, evaluation_panel, resize_bgr, write_png
    class_2_color = class_2_color or CLASS_2_COLOR_BDD
    for d in VISUAL_DIRS:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    H, W = net.height, net.width
    for index, batch in enumerate(dataset):
        x, x_raw, _, y_disp, _, y_seg = batch
        x = x.to(device=device, dtype=torch.float32)
        y_disp = y_disp.to(device=device, dtype=torch.float32).reshape(-1, H, W)[0]
        y_seg = y_seg.to(device=device, dtype=torch.float32).reshape(1, -1, H, W)
        y_disp_pred, y_seg_pred, _, _ = net(x)
        y_disp_pred = y_disp_pred.reshape(-1, H, W)[0]
        y_seg_pred = y_seg_pred.reshape(1, -1, H, W)
        if x_raw is None:
            rgb = ((x[0] * 0.5 + 0.5) * 255.0).clamp(0.0, 255.0).to(torch.uint8).permute(1, 2, 0)
            frame = resize_bgr(rgb.flip(2).contiguous(), (W, H))
        else:
            frame = x_raw[0].to(device=device, dtype=torch.uint8)
        pictures = {
            "RGB": frame,
            "GT_Depth": colorize_disparity(y_disp),
            "GT_Seg": color_masks(y_seg, class_2_color)[0],
            "Pred_Depth": colorize_disparity(y_disp_pred),
            "Pred_Seg": color_masks(y_seg_pred, class_2_color)[0],
        }
        for d, img in pictures.items():
            write_png(os.path.join(root, d, f"{index:04d}.png"), img, bgr=True)      # cv2.imwrite takes B, G, R
        panel = evaluation_panel(frame, y_disp_pred, y_seg_pred[0], class_2_color, disp_gt=y_disp, seg_gt=y_seg[0])
        write_png(os.path.join(root, "Panel", f"{index:04d}.png"), panel)               # already R, G, B
    return root


def write_occupancy_views(net, dataset, device, root: str, class_maps=None, class_2_color=None, point_count_threshold: float = 10.0) -> dict:
    """Pictures of the occupancy grid for every frame of `dataset` (utils/occupancy_views.py, painted on the GPU; only the finished u8 pictures are
    copied to the host for the PNG encoder): root/Occ_BEV/000N.png the grid from above, root/Occ_Overlay/000N.png the grid over the camera frame --
    prediction left, ground truth right in both -- and root/Occ_Panel/000N.png the four of them in one picture.  The ground truth is the grid
    evaluate_occupancy_set scores against; the prediction is frame 0's own grid for a model built with occupancy_per_frame=True, else the union
    grid of the forward.  Returns dict(root, bev_iou): the mean over the frames of bev_iou(pred, gt)["iou_2D"].  Like write_visuals it runs every
    frame through the model once more and leaves the metric loops as they are."""
    from ..utils.gt_occupancy import OccupancyProcessor
    from ..utils.occupancy import pack_occupancy
    from ..utils.occupancy_views import _Rect, _grid_bits, _overlay_into, _table, _view_into, BEV, bev_iou, occupancy_panel, view_size
    from ..utils.visualise import resize_bgr, write_png
    class_2_color = class_2_color or CLASS_2_COLOR_BDD
    for d in OCCUPANCY_VIEW_DIRS:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    proc = OccupancyProcessor(intrinsic_matrix=net.intrinsic_matrix, height=net.height, width=net.width, grid_size=net.grid_size, scale=net.scale, shift=net.shift,
                              pc_scale=net.pc_scale, pc_shift=net.pc_shift, point_count_threshold=point_count_threshold, num_classes=net.num_classes,
                              correction_angle=net.correction_angle)
    H, W, C = net.height, net.width, net.num_classes
    M, K = net.voxel_to_camera(), np.array([net.fx, net.fy, net.cx, net.cy], dtype=np.float64)
    zoom = 2
    bh, bw = view_size(net.grid_size, zoom=zoom, axis=BEV["axis"], transpose=BEV["transpose"])
    ious = []
    for index, batch in enumerate(dataset):
        x, x_raw, y_disp, y_seg = batch[0], batch[1], batch[3], batch[-1]
        x = x.to(device=device, dtype=torch.float32)
        seg_class = class_maps[index] if class_maps is not None else y_seg.to(device).argmax(dim=1)
        gt = proc.process(y_disp.to(device=device, dtype=torch.float32), seg_class, want_points=False, want_depth=False)
        net(x)
        if x_raw is None:
            rgb = ((x[0] * 0.5 + 0.5) * 255.0).clamp(0.0, 255.0).to(torch.uint8).permute(1, 2, 0)
            frame = resize_bgr(rgb.flip(2).contiguous(), (W, H))
        else:
            frame = x_raw[0].to(device=device, dtype=torch.uint8)
        pred_bits = net.last_occ_frame_bits[0] if getattr(net, "occupancy_per_frame", False) else net.last_occ_bits
        gt_bits = pack_occupancy(gt["occupancy_grid"][0], 0.5)
        table = _table(class_2_color, C, frame.device)
        bev = torch.empty((bh, 2 * bw, 3), dtype=torch.uint8, device=frame.device)
        overlay = torch.empty((H, 2 * W, 3), dtype=torch.uint8, device=frame.device)
        for k, b in enumerate((pred_bits, gt_bits)):
            bits, g = _grid_bits(b, net.grid_size, C, "write_occupancy_views")
            _view_into(bits, g, C, table, BEV["axis"], BEV["from_high"], zoom, 128, (32, 32, 32), BEV["flip"], BEV["transpose"], _Rect.tile(bev, 0, k * bw))
            _overlay_into(bits, g, C, frame.unsqueeze(0), H, W, M, K, table, 160, None, 12, 0.1, _Rect.tile(overlay, 0, k * W))
        panel = occupancy_panel(frame, pred_bits, gt_bits, voxel_to_camera=M, intrinsics=K, grid_size=net.grid_size, class_2_color=class_2_color, num_classes=C)
        write_png(os.path.join(root, "Occ_BEV", f"{index:04d}.png"), bev, bgr=True)
        write_png(os.path.join(root, "Occ_Overlay", f"{index:04d}.png"), overlay, bgr=True)
        write_png(os.path.join(root, "Occ_Panel", f"{index:04d}.png"), panel)              # already R, G, B
        ious.append(bev_iou(pred_bits, gt_bits, net.grid_size, num_classes=C)["iou_2D"])
    return dict(root=root, bev_iou=float(torch.cat(ious).mean().item()))


def synthetic_val_set(net, device, img: int, n: int = 10):
    """n batches (x, x_raw, mask_disp, y_disp, mask_seg, y_seg) in the datasets' layout (bengaluru_driving_dataset.py:118-140):
    GT at camera resolution, masks all-true.  GT = smooth perturbation of the model's own output."""
    H, W = net.height, net.width
    g = torch.Generator().manual_seed(0)
    out = []
    for i in range(n):
        x = synth_input(1, size=img, seed0=100 + i)
        with torch.no_grad():
            inv, seg, _, _ = net(x.to(device))
        inv, seg = inv.float().cpu().reshape(1, H, W), seg.float().cpu().reshape(1, -1, H, W)
        pert = torch.nn.functional.interpolate(torch.rand((1, 1, 9, 16), generator=g), size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        blobs = torch.nn.functional.interpolate(torch.rand((1, seg.shape[1], 12, 20), generator=g), size=(H, W), mode="bilinear", align_corners=False)
        y_disp = inv * (0.7 + 0.6 * pert) + 0.01 * pert
        y_seg = ((seg > 0.5) ^ (blobs > 0.8)).float()
        out.append((x, None, torch.ones_like(y_disp, dtype=torch.bool), y_disp, torch.ones_like(y_seg, dtype=torch.bool), y_seg))
    return out


def recorded_val_set(base_path: str, transforms, calib: str, device, n: int = 10, recordings=None, want_class_maps: bool = False, frame_pack=None,
                     frame_pack_required: bool = False):
    """The reference's evaluation subset of the recordings under base_path (eval_SOccDPT.py:126-135): random_split(dataset, [n, len - n]) with generator
    seed 0 -> (n items in the datasets' layout, each a batch of one; their ground-truth class maps [1,H,W] int32 from soccdpt_data_targets when asked
    for, else None; the (recording id, frame index) of every item).  The n frames are decoded concurrently, then assembled one by one."""
    from ..datasets.bengaluru_driving_dataset import BDD_Depth_Segmentation, get_bdd_dataset, resolve_index, submit_decode
    full = get_bdd_dataset(BDD_Depth_Segmentation, transforms, base_path, recordings=recordings, settings_doc=calib, device=device, frame_pack=frame_pack,
                           frame_pack_required=frame_pack_required)
    assert len(full) >= n, f"{base_path}: {len(full)} frames, the evaluation subset needs {n}"
    subset, _ = torch.utils.data.random_split(full, [n, len(full) - n], generator=torch.Generator().manual_seed(0))
    pending = [submit_decode(subset, [i]) for i in range(n)]
    items, class_maps = [], []
    for head, futures in pending:
        head.keep_class_map = want_class_maps
        items.append(head.assemble([f.result() for f in futures]))
        class_maps.append(head.last_class_map)
    picked = [(leaf.dataset_id, k) for leaf, k in (resolve_index(subset, i) for i in range(n))]
    return items, (class_maps if want_class_maps else None), picked


@torch.no_grad()
def main(args) -> dict:
    print(f"Model: SOccDPT_V{str(args.version)}_{args.model_type}")
    SOccDPT = SOccDPT_versions[args.version]
    device = torch.device(args.device)
    transforms, net_w, net_h = load_transforms(model_type=args.model_type)
    if "idd" in args.dataset:
        from ..datasets import IDD_UNSUPPORTED
        raise NotImplementedError(IDD_UNSUPPORTED)
    num_classes = 3
    real_data = os.path.isdir(os.path.expanduser(args.base_path))
    calib = args.camera_intrinsics_yaml
    if calib is None and real_data and os.path.isfile(os.path.join(os.path.expanduser(args.base_path), "calibration", "pocoX3", "calib.yaml")):
        calib = os.path.join(os.path.expanduser(args.base_path), "calibration", "pocoX3", "calib.yaml")
    calib = calib or write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    model_kwargs = dict(num_classes=num_classes, camera_intrinsics_yaml=calib)
    per_frame = bool(getattr(args, "occupancy_per_frame", False))
    occupancy_views = getattr(args, "occupancy_views", None)
    occupancy_observed = bool(getattr(args, "occupancy_observed", False))
    occupancy = bool(getattr(args, "occupancy", False)) or per_frame or bool(occupancy_views) or occupancy_observed
    if per_frame:
        model_kwargs.update(compute_occ=True, occupancy_per_frame=True)
    elif occupancy:
        model_kwargs.update(compute_occ=True, share_occupancy_rows=True)
    if args.version == 1:
        model_kwargs["load_depth"] = args.load_depth
        model_kwargs["load_seg"] = args.load_seg
    elif args.version == 2:
        assert args.load_depth is None or args.load_depth is False, "V2 does not support loading depth"
        assert args.load_seg is None or args.load_seg is False, "V2 does not support loading seg"
    elif args.version == 3:
        model_kwargs["load_depth"] = args.load_depth if args.load_depth is not None else False
        # the reference's script leaves model_type to the class default, so its -t only names the run; here -t builds that model (without it every
        # model but dpt_swin2_tiny_256 failed at load_state_dict with size mismatches)
        model_kwargs["model_type"] = args.model_type
        assert args.load_seg is None or args.load_seg is False, "V3 does not support loading seg"
    net = load_model(arch=SOccDPT, model_kwargs=model_kwargs, device=torch.device("cpu"), model_path=args.load,
                     model_type=args.model_type)
    if args.load is None:
        from ..model.spec import MODEL_TYPE_TO_BACKBONE
        net.load_state_dict(synth_state_dict(MODEL_TYPE_TO_BACKBONE[args.model_type], num_classes=num_classes, alias_pretrained=True), strict=False)
    if args.optimize and hasattr(net, "precision"):
        from ..lib import PREC_F16
        net.precision = PREC_F16
    net = net.to(device=device).eval()
    print("Model Parameters: {:.2f}M".format(sum(p.numel() for p in net.parameters()) / 1e6))

    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    class_maps = None
    if real_data:
        transforms.device = device
        dataset, class_maps, picked = recorded_val_set(os.path.expanduser(args.base_path), transforms, calib, device, n=10,
                                                       recordings=getattr(args, "recordings", None), want_class_maps=occupancy,
                                                       frame_pack=getattr(args, "frame_pack", None),
                                                       frame_pack_required=bool(getattr(args, "frame_pack_required", False)))
    else:
        dataset = synthetic_val_set(net, device, net_w, n=10)
    x = dataset[-1][0].to(device=device, dtype=torch.float32)

    frame_count = 50          # eval_SOccDPT.py:246-259
    for _ in range(5):
        _ = net(x)
    torch.cuda.synchronize(device)
    start_time = time.time()
    for _ in range(frame_count):
        _ = net(x)
    torch.cuda.synchronize(device)
    end_time = time.time()
    fps = frame_count / (end_time - start_time)
    print(f"FPS: {fps:.2f} ({frame_count} frames in {(end_time - start_time):.4f} seconds)")

    iou = evaluate_seg(SegNet(net), dataset, device, amp=False)
    abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 = evaluate_depth(DepthNet(net), dataset, device, amp=False)
    print(f"IOU: {iou:.4f}")
    print(f"ABS_REL: {abs_rel:.4f}")
    print(f"SQ_REL: {sq_rel:.4f}")
    print(f"RMSE: {rmse:.4f}")
    print(f"RMSE_LOG: {rmse_log:.4f}")
    print(f"A1: {a1:.4f}")
    print(f"A2: {a2:.4f}")
    print(f"A3: {a3:.4f}")
    result = dict(fps=fps, iou=iou, abs_rel=abs_rel, sq_rel=sq_rel, rmse=rmse, rmse_log=rmse_log, a1=a1, a2=a2, a3=a3)
    if occupancy:
        if occupancy_observed:
            result.update(evaluate_occupancy_set(net, dataset, device, class_maps=class_maps, observed=True))
        else:
            result.update(evaluate_occupancy_set(net, dataset, device, class_maps=class_maps))
        print(f"IOU_3D: {result['iou_3D']:.4f}")
        if occupancy_observed:
            print(f"IOU_3D_OBSERVED: {result['iou_3D_observed']:.4f}")
            print(f"OBSERVED_FRACTION: {result['observed_fraction']:.4f}")
        print(f"OCC_POINTS: {result['occ_points']:.1f}")
    if getattr(args, "visuals", None):
        result["visuals"] = write_visuals(net, dataset, device, os.path.join(args.visuals, f"{args.model_type}_{args.dataset}_{args.version}"))
        print(f"VISUALS: {result['visuals']}")
    if occupancy_views:
        views = write_occupancy_views(net, dataset, device, occupancy_views, class_maps=class_maps)
        result["occupancy_views"], result["bev_iou"] = views["root"], views["bev_iou"]
        print(f"BEV_IOU: {result['bev_iou']:.4f}")
    if real_data:
        result["frames"] = picked
    print("=" * 20)
    return result


def evaluate_occupancy_set(net, dataset, device, point_count_threshold: float = 10.0, class_maps=None, observed: bool = False) -> dict:
    """Mean 3-D IoU of the model's occupancy grid (packed bits of each forward) against the ground-truth grid OccupancyProcessor builds from the
    sample's (y_disp, class ids: class_maps[i] when given -- the recordings' class maps from soccdpt_data_targets --, else argmax y_seg), and the mean length of the model's occupancy point list -- everything on the GPU.  A model built with
    occupancy_per_frame=True is scored row by row: frame b's own grid (net.last_occ_frame_bits[b]) against ground-truth row b, and the list length
    is the mean over the frames; otherwise the one union grid of each forward is scored against every ground-truth row of its batch.
    observed=True adds iou_3D_observed and observed_fraction: the same comparison over only the voxels the ground truth's camera saw -- the rays of the
    generator's own `depth` through the grid (utils/occupancy_rays.py), plus the ground truth's occupied voxels; iou_3D itself does not change."""
    from ..utils.gt_occupancy import OccupancyProcessor
    from ..utils.occupancy import occupancy_iou
    from ..utils.occupancy_rays import occupancy_iou_observed
    proc = OccupancyProcessor(intrinsic_matrix=net.intrinsic_matrix, height=net.height, width=net.width, grid_size=net.grid_size, scale=net.scale, shift=net.shift,
                              pc_scale=net.pc_scale, pc_shift=net.pc_shift, point_count_threshold=point_count_threshold, num_classes=net.num_classes,
                              correction_angle=net.correction_angle)
    ious, lengths, ious_obs, fractions = [], [], [], []
    for i, batch in enumerate(dataset):
        x, y_disp, y_seg = batch[0], batch[3], batch[-1]
        x = x.to(device=device, dtype=torch.float32)
        seg_class = class_maps[i] if class_maps is not None else y_seg.to(device).argmax(dim=1)
        gt = proc.process(y_disp.to(device=device, dtype=torch.float32), seg_class, want_points=False, want_depth=False, want_observed=observed)
        net(x)
        if getattr(net, "occupancy_per_frame", False):
            pred = rows = net.last_occ_frame_bits
            ious.append(occupancy_iou(rows, gt["occupancy_grid"], num_classes=net.num_classes)["iou_3D"])
            lengths.extend(net.occupancy_points(frame=b).shape[0] for b in range(rows.shape[0]))
        else:
            pred = net.last_occ_bits
            ious.append(occupancy_iou(net.last_occ_bits, gt["occupancy_grid"], num_classes=net.num_classes)["iou_3D"])
            lengths.append(net.occupancy_points().shape[0])
        if observed:
            res = occupancy_iou_observed(pred, gt["occupancy_grid"], gt["observed"], num_classes=net.num_classes)
            ious_obs.append(res["iou_3D"])
            fractions.append(res["observed_fraction"])
    out = dict(iou_3D=float(torch.cat(ious).mean().item()), occ_points=float(np.mean(lengths)))
    if observed:
        out.update(iou_3D_observed=float(torch.cat(ious_obs).mean().item()), observed_fraction=float(torch.cat(fractions).mean().item()))
    return out


if __name__ == "__main__":
    main(build_parser().parse_args())
