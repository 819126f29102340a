"""Evaluation metrics on the GPU: same definitions and call shapes as the reference's
`evaluate_depth` / `evaluate_seg` loop bodies (/root/reference/SOccDPT/utils/__init__.py:161-332), computed by the
reduction kernels of libsoccdpt_hip.so without leaving HBM."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F

from ..lib import _call, _ptr, load_library

DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


def _scratch(B: int, C: int, device) -> torch.Tensor:
    n = load_library().soccdpt_metrics_scratch_bytes(B, C)
    return torch.empty(int(n), dtype=torch.uint8, device=device)


def depth_metrics(y_pred: torch.Tensor, y: torch.Tensor, mask: torch.Tensor) -> Dict[str, torch.Tensor]:
    """y_pred, y [B,H,W] f32, mask [B,H,W] bool (cuda) -> dict of 0-dim device tensors + 'scale'/'shift' [B].
    A prediction at another resolution is bicubic-resized to the ground truth first, like the reference
    (utils/__init__.py:207-212; that resize is torch plumbing, not part of the hot path)."""
    if y_pred.dim() == 2:
        y_pred = y_pred.unsqueeze(0)
    if y_pred.shape[-2:] != y.shape[-2:]:
        y_pred = F.interpolate(y_pred.unsqueeze(1), size=y.shape[-2:], mode="bicubic", align_corners=False)[:, 0]
    B = y.shape[0]
    npix = y.shape[1] * y.shape[2]
    p = y_pred.detach().to(torch.float32).contiguous()
    t = y.detach().to(torch.float32).contiguous()
    m = mask.detach().to(torch.uint8).contiguous()
    out = torch.empty(7 + 2 * B, dtype=torch.float32, device=y.device)
    sc = _scratch(B, 1, y.device)
    _call("soccdpt_metrics_depth", _ptr(p), _ptr(t), _ptr(m), B, npix, _ptr(out), _ptr(sc), device=y.device)
    res = {k: out[i] for i, k in enumerate(DEPTH_KEYS)}
    res["scale"] = out[7::2]
    res["shift"] = out[8::2]
    return res


def iou_metric(y_pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y_pred, y [B,C,H,W] (cuda) -> per-image IoU [B] (threshold 0.5, mean over classes)."""
    if y_pred.dim() == 3:
        y_pred = y_pred.unsqueeze(0)
    if y_pred.shape[-2:] != y.shape[-2:]:
        y_pred = F.interpolate(y_pred, size=y.shape[-2:], mode="bicubic", align_corners=False)
    B, C = y.shape[0], y.shape[1]
    npix = y.shape[2] * y.shape[3]
    p = y_pred.detach().to(torch.float32).contiguous()
    t = y.detach().to(torch.float32).contiguous()
    out = torch.empty(B, dtype=torch.float32, device=y.device)
    sc = _scratch(B, C, y.device)
    _call("soccdpt_metrics_iou", _ptr(p), _ptr(t), B, C, npix, _ptr(out), _ptr(sc), device=y.device)
    return out


def evaluate_depth(net, dataloader, device, amp=False):
    """Same signature/return as the reference's evaluate_depth: mean over batches of the 7 depth metrics."""
    import numpy as np
    net.eval()
    acc = []
    for batch in dataloader:
        if len(batch) == 4:
            x, _, mask, y = batch
        else:
            x, _, mask, y, _, _ = batch
        x = x.to(device=device, dtype=torch.float32)
        y = y.to(device=device, dtype=torch.float32)
        mask = mask.to(device=device, dtype=torch.bool)
        y_pred = net(x)
        m = depth_metrics(y_pred, y, mask)
        acc.append(torch.stack([m[k] for k in DEPTH_KEYS]))
    vals = torch.stack(acc).cpu().numpy().astype(np.float64)          # [batches, 7]
    # per-metric filtering of the reference (utils/__init__.py:236-244): a non-finite abs_rel / sq_rel / rmse_log of ONE batch is
    # dropped from that metric's mean instead of poisoning it; rmse and a1..a3 are always kept
    out = []
    for i, k in enumerate(DEPTH_KEYS):
        col = vals[:, i]
        if k in ("abs_rel", "sq_rel", "rmse_log"):
            col = col[np.isfinite(col)]
        out.append(float(np.mean(col)))
    return tuple(out)


def evaluate_seg(net, dataloader, device, amp=False):
    """Same signature/return as the reference's evaluate_seg: mean IoU over images and batches."""
    net.eval()
    ious = []
    for batch in dataloader:
        if len(batch) == 4:
            x, _, _, y = batch
        else:
            x, _, _, _, _, y = batch
        x = x.to(device=device, dtype=torch.float32)
        y = y.to(device=device, dtype=torch.float32)
        ious.append(iou_metric(net(x), y))
    return float(torch.cat(ious).mean().item())


def _histograms(net) -> dict:
    """The reference's wandb.Histogram of every weight and gradient, only when wandb is installed."""
    out = {}
    try:
        import wandb
    except ImportError:
        return out
    for tag, value in net.named_parameters():
        if value is not None and value.grad is not None:
            tag = tag.replace("/", ".")
            out["Weights/" + tag] = wandb.Histogram(value.data.cpu())
            out["Gradients/" + tag] = wandb.Histogram(value.grad.data.cpu())
    return out


def evaluate(net, seg_wrapper, disp_wrapper, val_set, device, amp, x_raw, y_disp, y_disp_pred, y_seg, y_seg_pred, points, class_2_color, loss, lr,
             global_step, epoch, experiment):
    """The reference's per-epoch evaluate (SOccDPT/utils/__init__.py:598-765), same 18 positional parameters: evaluate_depth and evaluate_seg over
    val_set (the same two printed lines), the image panel and the coloured point list of sample 0, all computed on the GPU.  Logs the reference's keys
    through experiment.log and returns the logged dict: `learning rate`, the seven depth metrics, `iou`, `plot` as a uint8 RGB numpy array
    [H, round(3 W / 2), 3] (the payload of its wandb.Image: frame | predicted | ground-truth depth over frame | predicted | ground-truth classes, at
    half size), `plot_points` as an [N,6] numpy array (the payload of its wandb.Object3D: every tenth point of points[0] beside every tenth pixel of
    the ground-truth class picture, rows whose first colour channel is 0 dropped), `loss`, `step`, `epoch`; the wandb histograms only when wandb is
    installed."""
    from .visualise import color_masks, evaluation_panel
    dev = torch.device(device)
    abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 = evaluate_depth(disp_wrapper, val_set, device, amp=amp)
    print("abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3", abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3)
    iou = evaluate_seg(seg_wrapper, val_set, device, amp=amp)
    print("iou", iou)
    frame_bgr = x_raw[0].detach().squeeze().to(device=dev, dtype=torch.uint8)
    disp_pred = (y_disp_pred if y_disp_pred.dim() == 2 else y_disp_pred[0]).to(dev)
    seg_pred = (y_seg_pred if y_seg_pred.dim() == 3 else y_seg_pred[0]).to(dev)
    disp_gt, seg_gt = y_disp[0].to(dev), y_seg[0].to(dev)
    vis_img = evaluation_panel(frame_bgr, disp_pred, seg_pred, class_2_color, disp_gt=disp_gt, seg_gt=seg_gt)
    gt_colors = color_masks(seg_gt.unsqueeze(0), class_2_color)[0].reshape(-1, 3)[::10]
    pts = torch.as_tensor(points)[0].detach().to(dev).reshape(-1, 3)[::10]
    keep = gt_colors[:, 0] > 0
    plot_points_colors = torch.cat([pts[keep], gt_colors[keep].to(pts.dtype)], dim=1).cpu().numpy()
    print("plot_points_colors", plot_points_colors.shape)
    print("loss: {}".format(loss))
    log = {
        "learning rate": lr,
        "abs_rel": abs_rel, "sq_rel": sq_rel, "rmse": rmse, "rmse_log": rmse_log, "a1": a1, "a2": a2, "a3": a3,
        "iou": iou,
        "plot": vis_img.cpu().numpy(),
        "plot_points": plot_points_colors,
        "loss": loss.item() if hasattr(loss, "item") else float(loss),
        "step": global_step,
        "epoch": epoch,
    }
    log.update(_histograms(net))
    experiment.log(log)
    return log


def evaluate_occupancy(net, val_set, device, amp, x_raw, y_occupancy_grid, y_occupancy_grid_pred, y_disp_pred, y_seg_pred, class_2_color, loss, lr,
                       global_step, epoch, experiment):
    """The reference's evaluate_occupancy (SOccDPT/utils/__init__.py:375-529), same 15 positional parameters, with the grids left on
    the GPU: both point lists of sample 0 come from csrc/occ_eval.hip (occupancy_grid_to_points), and `iou_3D` -- 0.0 with a "# TODO: Implement"
    there -- is the mean over the batch of occupancy_iou(pred, gt)["iou_3D"].  Logs the reference's keys through experiment.log and returns the
    logged dict: `learning rate`, `iou_3D`, `plot_points_gt` / `plot_points_pred` as [N,6] float64 numpy arrays (x, y, z, r, g, b: the payload of
    the reference's wandb.Object3D), `plot` as a uint8 RGB numpy array [H, W, 3] (the payload of its wandb.Image: frame | depth over frame | classes
    at half size, utils.visualise.evaluation_panel), `loss`, `step`, `epoch`; the wandb weight / gradient histograms are added only when wandb is installed."""
    from .occupancy import occupancy_grid_to_points, occupancy_iou, semantic_pc_to_colors_and_pc
    from .visualise import evaluation_panel
    grid_size = tuple(getattr(net, "grid_size", (256, 256, 32)))
    scale = tuple(getattr(net, "scale", (2.0, 2.0, 0.666)))

    def rows_of(t):     # [B,g0,g1,g2,C]; a stride-0 batch view (share_occupancy_rows) is one row
        t = t if t.dim() == 5 else t.unsqueeze(0)
        return t[:1] if t.stride(0) == 0 else t

    def plot_points(grid):
        pc = occupancy_grid_to_points(grid, grid_size=grid_size, scale=scale, shift=(0.0, 0.0, 0.0))
        pts, colors = semantic_pc_to_colors_and_pc(pc, class_2_color)
        return torch.cat([pts, colors.to(pts.dtype)], dim=1).cpu().numpy()

    gt, pred = rows_of(y_occupancy_grid.detach().to(device)), rows_of(y_occupancy_grid_pred.detach().to(device))
    num_classes = gt.shape[-1]
    iou_3D = float(occupancy_iou(pred, gt, num_classes=num_classes)["iou_3D"].mean().item())
    log = {
        "learning rate": lr,
        "iou_3D": iou_3D,
        "plot_points_gt": plot_points(gt[0]),
        "plot_points_pred": plot_points(pred[0]),
        "loss": loss.item() if hasattr(loss, "item") else float(loss),
        "step": global_step,
        "epoch": epoch,
    }
    frame_bgr = x_raw[0].detach().squeeze().to(device=device, dtype=torch.uint8)
    disp = y_disp_pred[0] if y_disp_pred.dim() > 2 else y_disp_pred
    seg = y_seg_pred[0] if y_seg_pred.dim() > 3 else y_seg_pred
    log["plot"] = evaluation_panel(frame_bgr, disp.to(device), seg.to(device), class_2_color).cpu().numpy()
    log.update(_histograms(net))
    print("loss: {}".format(loss))
    experiment.log(log)
    return log


def occupancy_pictures(net, x_raw, y_occupancy_grid, y_occupancy_grid_pred, class_2_color) -> dict:
    """The picture evaluate_occupancy's log lacks: {"plot_occupancy": u8 RGB numpy array}, utils.occupancy_views.occupancy_panel of sample 0 --
    predicted | ground-truth grid over the camera frame, above both grids seen from above.  Same x_raw / grid arguments as evaluate_occupancy
    (dense [B,g0,g1,g2,C] or [g0,g1,g2,C], or packed rows); `net` supplies the geometry: grid_size, intrinsics and voxel_to_camera().  Callers merge
    the dict into their log; evaluate_occupancy itself logs what the reference logs."""
    from .occupancy_views import occupancy_panel

    def first(t, dev):     # one grid: row 0 of a batch of dense grids or of packed rows
        t = t.detach().to(dev)
        return t[0] if t.dim() in (2, 5) else t

    frame_bgr = x_raw[0].detach().squeeze()
    dev = y_occupancy_grid_pred.device
    frame_bgr = frame_bgr.to(device=dev, dtype=torch.uint8)
    panel = occupancy_panel(frame_bgr, first(y_occupancy_grid_pred, dev), first(y_occupancy_grid, dev), voxel_to_camera=net.voxel_to_camera(),
                            intrinsics=(net.fx, net.fy, net.cx, net.cy), grid_size=net.grid_size, class_2_color=class_2_color, num_classes=net.num_classes)
    return {"plot_occupancy": panel.cpu().numpy()}
