"""numpy specification of the batch targets (include/soccdpt_data.h, csrc/batch_targets.hip): what the reference's dataset code does on the host
(SOccDPT/datasets/bengaluru_driving_dataset.py:67-76 rgb_seg_to_bool, SOccDPT/datasets/bdd_helper.py:10-25 rgb_seg_to_class, torch.tensor(disparity)),
restated for a batch and an arbitrary colour table.  Every result is exact: comparisons of bytes, exact integer -> f32 conversions, integer resize."""
import numpy as np

from tests.visualise_refs import resize_taps

BDD_COLORS = np.array([(0, 0, 0), (0, 0, 142), (220, 20, 60)], dtype=np.uint8)      # row c: the colour of class c


def onehot(seg, colors):
    """seg u8 [B,H,W,3], colors u8 [C,3] -> f32 [B,C,H,W]: plane c is 1 where the stored channels equal colors[c]; the classes are independent."""
    seg, colors = np.asarray(seg, dtype=np.uint8), np.asarray(colors, dtype=np.uint8)
    return np.stack([np.all(seg == colors[c], axis=-1) for c in range(colors.shape[0])], axis=1).astype(np.float32)


def class_map(seg, colors, flip=False):
    """-> i32 [B,H,W]: 0, then c for c = 0 .. C-1 in order where the pixel (channels 0 and 2 exchanged first when flip) equals colors[c]."""
    seg, colors = np.asarray(seg, dtype=np.uint8), np.asarray(colors, dtype=np.uint8)
    cmp = seg[..., ::-1] if flip else seg
    out = np.zeros(seg.shape[:3], dtype=np.int32)
    for c in range(colors.shape[0]):
        out[np.all(cmp == colors[c], axis=-1)] = c
    return out


def unmatched(seg, colors):
    """-> u64 [B]: pixels whose stored channels equal no colour of the table."""
    return (onehot(seg, colors).sum(axis=1) == 0).reshape(np.asarray(seg).shape[0], -1).sum(axis=1).astype(np.uint64)


def y_disp(disp):
    """u8 / u16 / f32 [B,H,W] -> f32, exactly (an f32 input keeps its bits, NaN payloads included)."""
    disp = np.asarray(disp)
    assert disp.dtype in (np.uint8, np.uint16, np.float32)
    return disp.copy() if disp.dtype == np.float32 else disp.astype(np.float32)


def resize_u8c1(img, dsize):
    """u8 [H,W], dsize = (width, height) -> u8 [height,width]: the integer bilinear of visualise_refs.resize for one channel."""
    a = np.asarray(img).astype(np.int64)
    Wd, Hd = int(dsize[0]), int(dsize[1])
    if (Hd, Wd) == a.shape:
        return a.astype(np.uint8)
    yt, xt = resize_taps(a.shape[0], Hd).astype(np.int64), resize_taps(a.shape[1], Wd).astype(np.int64)
    wy1, wx1 = yt[:, 2][:, None], xt[:, 2][None, :]
    wy0, wx0 = 2048 - wy1, 2048 - wx1
    ya, yb, xa, xb = yt[:, 0], yt[:, 1], xt[:, 0], xt[:, 1]
    s = a[ya][:, xa] * wx0 * wy0 + a[ya][:, xb] * wx1 * wy0 + a[yb][:, xa] * wx0 * wy1 + a[yb][:, xb] * wx1 * wy1
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


# ---- inputs shared by the CPU and the GPU tests ----
PALETTE = np.array([(0, 0, 0), (0, 0, 142), (220, 20, 60),        # the three class colours
                    (142, 0, 0), (60, 20, 220),                    # their channel-reversed forms: no class for rgb_seg_to_bool, a class for rgb_seg_to_class
                    (0, 0, 141), (220, 20, 61)], dtype=np.uint8)   # near misses


def label_frames(B, H, W, seed, palette=PALETTE):
    """u8 [B,H,W,3] drawn uniformly from the palette."""
    rng = np.random.default_rng(seed)
    return palette[rng.integers(0, len(palette), size=(B, H, W))]


def write_recording(base, rec_id, n=12, size=(48, 64), disp_mode="L", seed=0, t0=1658384707877, palette=PALETTE, blocky=True):
    """Write a recording in the Bengaluru layout under base/rec_id with PIL: rgb_img / depth_img / seg_img/<timestamp>.png and <rec_id>.csv (a header
    row, the timestamp in the second column).  size = (H, W); disp_mode 'L' (u8) or 'I;16' (u16).  blocky: labels in 4 x 4 blocks, so that a
    resized label image keeps class pixels inside the blocks and gets blended ones at their borders.  -> the frames as the PNGs hold them:
    {'rgb': u8 [n,H,W,3], 'seg': u8 [n,H,W,3], 'disp': [n,H,W], 'timestamps': [n]}."""
    import os
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = size
    root = os.path.join(str(base), str(rec_id))
    for d in ("rgb_img", "depth_img", "seg_img"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    rgb = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    if blocky:
        idx = rng.integers(0, len(palette), size=(n, (H + 3) // 4, (W + 3) // 4))
        seg = palette[np.repeat(np.repeat(idx, 4, axis=1), 4, axis=2)[:, :H, :W]]
    else:
        seg = palette[rng.integers(0, len(palette), size=(n, H, W))]
    if disp_mode == "L":
        disp = rng.integers(1, 256, size=(n, H, W), dtype=np.uint8)
    else:
        disp = rng.integers(1, 65536, size=(n, H, W)).astype(np.uint16)
        disp.reshape(-1)[:5] = (0, 1, 255, 256, 65535)
    ts = [t0 + 33 * i for i in range(n)]
    with open(os.path.join(root, f"{rec_id}.csv"), "w") as f:
        f.write("Index,Timestamp,speed\n")
        for i, t in enumerate(ts):
            f.write(f"{i},{t},{0.5 * i}\n")
    for i, t in enumerate(ts):
        Image.fromarray(rgb[i]).save(os.path.join(root, "rgb_img", f"{t}.png"))
        Image.fromarray(seg[i]).save(os.path.join(root, "seg_img", f"{t}.png"))
        Image.fromarray(disp[i]).save(os.path.join(root, "depth_img", f"{t}.png"))
    return dict(rgb=rgb, seg=np.ascontiguousarray(seg), disp=disp, timestamps=ts)
