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


def evaluate_occupancy(net, val_set, device, amp, x_raw, y_occupancy_grid, y_occupancy_grid_pred, y_disp_pred, y_seg_pred, class_2_color, loss, lr,
                       global_step, epoch, experiment):
    """The reference's evaluate_occupancy (SOccDPT/utils/__init__.py:375-529), same 15 positional parameters, with the grids left on
    the GPU: both point lists of sample 0 come from csrc/occ_eval.hip (occupancy_grid_to_points), and `iou_3D` -- 0.0 with a "# TODO: Implement"
    there -- is the mean over the batch of occupancy_iou(pred, gt)["iou_3D"].  Logs the reference's keys through experiment.log and returns the
    logged dict: `learning rate`, `iou_3D`, `plot_points_gt` / `plot_points_pred` as [N,6] float64 numpy arrays (x, y, z, r, g, b: the payload of
    the reference's wandb.Object3D), `loss`, `step`, `epoch`; the cv2 image panel (`plot`) and the wandb weight / gradient histograms are added only
    when those packages are installed."""
    import numpy as np
    from .occupancy import occupancy_grid_to_points, occupancy_iou, semantic_pc_to_colors_and_pc
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
    try:
        import cv2
        frame_rgb = x_raw[0].detach().squeeze().cpu().numpy()
        disp = (y_disp_pred[0] if y_disp_pred.dim() > 2 else y_disp_pred).detach().squeeze().cpu().numpy()
        disp = (disp - np.min(disp)) / (np.max(disp) - np.min(disp))
        disp = cv2.resize(cv2.applyColorMap((disp * 255).astype(np.uint8), cv2.COLORMAP_PLASMA), frame_rgb.shape[:2][::-1])
        masks = (y_seg_pred[0] if y_seg_pred.dim() > 3 else y_seg_pred).permute(1, 2, 0).detach().cpu().numpy() > 0.5
        if masks.shape[:2] != frame_rgb.shape[:2]:
            masks = cv2.resize(masks.astype(np.uint8), frame_rgb.shape[:2][::-1], interpolation=cv2.INTER_NEAREST).astype(bool)
        seg_img = np.zeros_like(frame_rgb)
        for c in range(masks.shape[2]):
            seg_img[masks[:, :, c]] = class_2_color[c]
        vis = np.concatenate([np.concatenate([frame_rgb, disp], 1), np.concatenate([frame_rgb, seg_img], 1)], 0)
        log["plot"] = cv2.resize(cv2.cvtColor(vis, cv2.COLOR_BGR2RGB), (0, 0), fx=0.5, fy=0.5)
    except ImportError:
        pass
    try:
        import wandb
        for tag, value in net.named_parameters():
            if value is not None and value.grad is not None:
                tag = tag.replace("/", ".")
                log["Weights/" + tag] = wandb.Histogram(value.data.cpu())
                log["Gradients/" + tag] = wandb.Histogram(value.grad.data.cpu())
    except ImportError:
        pass
    print("loss: {}".format(loss))
    experiment.log(log)
    return log
