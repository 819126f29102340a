"""The Bengaluru datasets with the names of the reference's `SOccDPT/datasets/bengaluru_driving_dataset.py` (`BDD_Depth`, `BDD_Segmentation`,
`BDD_Depth_Segmentation`, `get_bdd_dataset`, `color_2_class`, `class_2_color`), their item layouts and shapes -- and the targets built on the GPU.

The reference builds an item on the host: three PNG decodes, three cv2.resize calls to 1920 x 1080, `rgb_seg_to_bool`, float copies, and a
`.to(device)` of float / bool targets (about 330 MB per batch of 8).  Here only the decode stays on the host.  The uint8 frames are uploaded from
pinned memory and everything else is a kernel:

    x_raw    soccdpt_vis_resize           frames -> camera size (an equal size is a copy)
    x        soccdpt_input_transform_u8   model/transforms.py InputTransform.batch, one launch per batch
    labels   soccdpt_vis_resize, disparity (uint8) soccdpt_data_resize_u8c1
    y_seg, y_disp, unmatched              soccdpt_data_targets, one launch per batch (csrc/batch_targets.hip)

Items are lists of cuda tensors that carry their batch dimension, `[x, x_raw, mask_disp, y_disp, mask_seg, y_seg]` for the combined class; the masks
are cached all-true tensors.  `dataset.batch(indices)` is the fast path (one decode round, one upload, one transform and one targets launch for the
whole batch) and is bit-identical to `torch.cat` of the single items; `dataset_batch` reaches it through `Subset` / `ConcatDataset` index maps and
`BatchPrefetcher` overlaps the next batch's decode and upload with the current step.

Deviations from the reference, all stated: the target size is the calibration file's Camera.width x Camera.height (1920 x 1080 for the real
calibration; the reference hard-codes that literal); y_seg is float32 0 / 1 rather than bool (what the criterion reads); uint16 / float32 disparity
must be stored at camera size (OpenCV resizes those with float weights; without cv2 there is nothing to pin a resampling against, so none is
guessed); byte parity of the two uint8 resizes with cv2.resize itself is not pinned for the same reason.  There is no CPU
fallback: the items need the HIP library and a GPU.

`frame_pack=` (opt-in, datasets/frame_pack.py) takes the decode away as well: the recording's frames are read from one mapped
file, the pool's threads copy them straight into the pinned staging buffers, label frames go up as palette indices and the targets are built from
those (soccdpt_pack_targets).  Items and batches are bit-identical to the PNG path's."""
from __future__ import annotations

import bisect
import os
import warnings
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .bdd_helper import DEFAULT_CALIB, DEFAULT_DATASET, BengaluruDepthDatasetIterator
from .frame_pack import FramePack, FramePackError, open_current, pack_path

color_2_class = {
    (0, 0, 0): 0,         # background
    (0, 0, 142): 1,       # vehicle
    (220, 20, 60): 2,     # pedestrian
}
class_2_color = {v: k for k, v in color_2_class.items()}

DEFAULT_RECORDINGS = ("1653972957447", "1652937970859", "1654493684259", "1654507149598", "1658384707877", "1658384924059")

DEFAULT_WORKERS = 8      # decode threads; a fixed number, never the machine's CPU count
MAX_WORKERS = 16

_pools: Dict[int, ThreadPoolExecutor] = {}


def decode_pool(workers: int = DEFAULT_WORKERS) -> ThreadPoolExecutor:
    """The shared pool of `workers` decode threads (1 .. MAX_WORKERS).  Its threads only read files and fill host arrays; none touches the GPU."""
    workers = int(workers)
    if not 1 <= workers <= MAX_WORKERS:
        raise ValueError(f"decode workers must be between 1 and {MAX_WORKERS}, got {workers}")
    if workers not in _pools:
        _pools[workers] = ThreadPoolExecutor(max_workers=workers, thread_name_prefix="bdd-decode")
    return _pools[workers]


def rgb_seg_to_bool(seg_frame: np.ndarray) -> np.ndarray:
    """Host form of the one-hot labels (bengaluru_driving_dataset.py:67-76): plane color_2_class[colour] is true where the pixel, channels as stored,
    equals the colour.  The batched GPU form is soccdpt_data_targets(onehot)."""
    seg_frame = np.asarray(seg_frame)
    out = np.zeros((seg_frame.shape[0], seg_frame.shape[1], len(color_2_class)), dtype=bool)
    for color, cls in color_2_class.items():
        out[:, :, cls] = np.all(seg_frame == np.array(color), axis=-1)
    return out


def color_table(c2c: Optional[Dict[tuple, int]] = None) -> np.ndarray:
    """{colour: class} -> uint8 [C,3] with row c the colour of class c (classes 0 .. C-1, each exactly once)."""
    c2c = color_2_class if c2c is None else c2c
    assert sorted(c2c.values()) == list(range(len(c2c))), "the classes of a colour table are 0 .. C-1, each once"
    table = np.zeros((len(c2c), 3), dtype=np.uint8)
    for color, cls in c2c.items():
        table[cls] = color
    return table


class _Staging:
    """Pinned host buffers for the uploads, reused.  A buffer is handed out again only after the copy that last read it has finished (its event)."""

    def __init__(self, ring: int = 4):
        self.ring, self.slots = ring, {}

    def upload(self, arrays: Sequence[np.ndarray], device: torch.device, pool: Optional[ThreadPoolExecutor] = None) -> torch.Tensor:
        """Equal-shaped host arrays -> one [n, ...] device tensor, copied from pinned memory on the current stream without blocking the host.  With a
        pool, its threads copy one array each straight into their slice of the pinned buffer (np.copyto releases the GIL) and this thread only waits
        for them: how the views of a frame pack's mapping are staged."""
        shape, dtype = (len(arrays),) + tuple(arrays[0].shape), torch.from_numpy(np.empty(0, arrays[0].dtype)).dtype
        slots = self.slots.setdefault((shape, dtype), deque())
        if len(slots) < self.ring:
            buf, ev = torch.empty(shape, dtype=dtype, pin_memory=True), torch.cuda.Event()
        else:
            buf, ev = slots.popleft()
            ev.synchronize()
        view = buf.numpy()
        if pool is not None and len(arrays) > 1:
            list(pool.map(np.copyto, [view[i] for i in range(len(arrays))], arrays))
        else:
            for i, a in enumerate(arrays):
                np.copyto(view[i], a)
        out = buf.to(device, non_blocking=True)
        ev.record(torch.cuda.current_stream(device))
        slots.append((buf, ev))
        return out


class BDD_Dataset(BengaluruDepthDatasetIterator):
    """Base of the three datasets.  `transform` is what model.loader.load_transforms returns (its `.batch` runs the input transform kernel)."""

    fields: Tuple[str, ...] = ()          # of x, x_raw, mask_disp, y_disp, mask_seg, y_seg, in the item's order
    to_camera_size = False                # only the combined class resizes its frames (bengaluru_driving_dataset.py:118-121)

    def __init__(self, dataset_path: str = DEFAULT_DATASET, settings_doc: str = DEFAULT_CALIB, transform: Callable = lambda x: x, device=None,
                 workers: int = DEFAULT_WORKERS, frame_pack=None, frame_pack_required: bool = False):
        """frame_pack: None reads the PNGs; True reads <recording>/<id>.sfp, a string <that directory>/<id>.sfp (datasets/frame_pack.py).  A pack that
        is missing, truncated, of another version or older than its PNGs is not read: the dataset warns once, naming the file, and reads the PNGs;
        with frame_pack_required it raises FramePackError instead."""
        super().__init__(dataset_path=dataset_path, settings_doc=settings_doc)
        assert transform is not None
        self.img_transform = transform
        self.device = torch.device(device if device is not None else getattr(transform, "device", "cuda:0"))
        self.workers = int(workers)
        self.colors = color_table()
        self.last_unmatched: Optional[torch.Tensor] = None      # int64 [B] (cuda): pixels of each frame of the last batch that carry no class colour
        self.keep_class_map = False                             # True: every batch also leaves its class ids [B,H,W] int32 in last_class_map
        self.last_class_map: Optional[torch.Tensor] = None
        self._staging = _Staging()
        self._on_device: dict = {}
        self.pack: Optional[FramePack] = None
        if frame_pack is not None and frame_pack is not False:
            try:
                self.pack = open_current(self.dataset_path, frame_pack)
            except FramePackError as e:
                if frame_pack_required:
                    raise
                warnings.warn(f"{e}; reading the PNGs of {self.dataset_path} instead", RuntimeWarning, stacklevel=2)

    # ---- host half: runs in worker threads, touches no GPU ----
    def _pack_row(self, key: int) -> dict:
        """The CSV half of a frame dictionary from the pack, with the reader's bounds rules (bdd_helper.frame_paths)."""
        if key > len(self):
            raise IndexError("Out of bounds; key=", key)
        if key < 0 or key == len(self):
            raise KeyError(key)
        csv_frame = dict(zip(self.csv_columns, self.csv_dat[key]))
        return dict(csv_frame=csv_frame, **csv_frame)

    def read_frame(self, key: int) -> dict:
        """The reader's frame dictionary.  From a pack: the same keys and bytes, the arrays being read-only views of the mapping (seg_frame a copy
        made by the host palette lookup)."""
        if self.pack is None:
            frame = super().read_frame(key)
        else:
            row, f = self._pack_row(key), self.pack.frame(key)
            frame = {"rgb_frame": f["rgb"], "disparity_frame": f["disparity"], "seg_frame": self.pack.labels_rgb(key), "csv_frame": row.pop("csv_frame")}
            frame.update(row)
        return self._checked(frame, key)

    def batch_frame(self, key: int) -> dict:
        """What `assemble` takes for frame `key`: read_frame's dictionary, except that a pack with indexed labels hands over the indices themselves
        (`seg_index`: u32 words, `seg_pack`: the FramePack) instead of looking the colours up on the host."""
        if self.pack is None or self.pack.raw_labels:
            frame = self.read_frame(key)
        else:
            row, f = self._pack_row(key), self.pack.frame(key)
            frame = {"rgb_frame": f["rgb"], "disparity_frame": f["disparity"], "seg_index": f["labels"].view(np.int32), "seg_pack": self.pack,
                     "csv_frame": row.pop("csv_frame")}
            frame.update(row)
            self._checked(frame, key)
        if self.pack is not None:
            frame["_pooled"] = True      # views of a mapping: staged by the pool's threads
        return frame

    def _checked(self, frame: dict, key: int) -> dict:
        d = frame["disparity_frame"]
        if self.to_camera_size and d.dtype != np.uint8 and tuple(d.shape) != (self.height, self.width):
            raise NotImplementedError(
                f"{self.dataset_path} frame {key}: a {d.dtype} disparity image stored at {d.shape[1]} x {d.shape[0]} would have to be resampled to the "
                f"camera's {self.width} x {self.height}; only uint8 disparity is resized (integer bilinear), 16-bit and float disparity must be stored at "
                "camera size")
        return frame

    def decode(self, indices: Iterable[int]) -> List[dict]:
        """The frame dictionaries of `indices`, decoded concurrently by the shared pool."""
        return list(decode_pool(self.workers).map(self.batch_frame, [int(i) for i in indices]))

    # ---- device half: the caller's thread, the current stream ----
    def _cached(self, key, make):
        """Small device tensors made once (masks, tap tables, colours, blank labels) and then read from whichever stream assembles a batch: the host waits
        for the stream that fills a new one, so no later reader on another stream can be ahead of the fill."""
        if key not in self._on_device:
            self._on_device[key] = make()
            torch.cuda.current_stream(self.device).synchronize()
        return self._on_device[key]

    def _taps(self, src: int, dst: int) -> torch.Tensor:
        from ..utils.visualise import resize_taps
        return self._cached(("taps", src, dst), lambda: torch.from_numpy(resize_taps(src, dst)).to(self.device))

    def _ones(self, shape) -> torch.Tensor:
        return self._cached(("ones", tuple(shape)), lambda: torch.ones(tuple(shape), dtype=torch.bool, device=self.device))

    def _upload(self, frames: List[dict], key: str) -> torch.Tensor:
        """frames[i][key], all of one shape and dtype -> [B, ...] on the device; at camera size afterwards when this class resizes."""
        arrays = [f[key] for f in frames]
        t = self._staging.upload(arrays, self.device, decode_pool(self.workers) if frames[0].get("_pooled") else None)
        return t if key == "seg_index" else self._to_camera_size(t)

    def _to_camera_size(self, t: torch.Tensor) -> torch.Tensor:
        if not self.to_camera_size:
            return t
        Hc, Wc = int(self.height), int(self.width)
        if tuple(t.shape[1:3]) == (Hc, Wc):
            return t
        if t.dim() == 4:
            from ..utils.visualise import resize_bgr
            return resize_bgr(t, (Wc, Hc))
        from ..lib import op_data_resize_u8c1
        assert t.dtype == torch.uint8       # read_frame refused the others
        return op_data_resize_u8c1(t, Hc, Wc, self._taps(t.shape[1], Hc), self._taps(t.shape[2], Wc))

    def assemble(self, frames: List[dict]) -> list:
        """Decoded frames -> the item's tensors for the whole batch, on the current stream of self.device.  Frames stored alike (the sizes and the
        disparity format of one recording) go through one upload, one transform and one targets launch; a batch that mixes recordings stored
        differently is assembled group by group and put back into the batch's order."""
        def kind(f):
            if "seg_frame" in f:
                labels = (f["seg_frame"].shape, f["seg_frame"].dtype.str)
            elif "y_seg" in self.fields:      # indexed labels are alike when they share the frame size, k and the palette
                labels = ("indexed", f["seg_pack"].shapes["labels"], f["seg_pack"].k, f["seg_pack"].palette.tobytes())
            else:                             # not read: only their size counts, as for label frames
                labels = (f["seg_pack"].shapes["labels"] + (3,), "|u1")
            return ((f["rgb_frame"].shape, f["rgb_frame"].dtype.str), labels, (f["disparity_frame"].shape, f["disparity_frame"].dtype.str))
        groups: Dict[tuple, List[int]] = {}
        for pos, f in enumerate(frames):
            groups.setdefault(kind(f), []).append(pos)
        if len(groups) == 1:
            return self._assemble_alike(frames)
        if not self.to_camera_size:
            raise ValueError(f"{type(self).__name__} does not resize: the frames of one batch must be stored alike, got {sorted(groups)}")
        parts, extras = [], []
        for positions in groups.values():
            parts.append(self._assemble_alike([frames[p] for p in positions]))
            extras.append((self.last_unmatched, self.last_class_map))
        order = torch.tensor([p for positions in groups.values() for p in positions]).argsort().to(self.device)
        merged = lambda ts: None if ts[0] is None else torch.cat(ts, dim=0).index_select(0, order)
        self.last_unmatched, self.last_class_map = merged([e[0] for e in extras]), merged([e[1] for e in extras])
        return [self._ones(torch.Size([len(frames)]) + parts[0][k].shape[1:]) if name.startswith("mask") else merged([p[k] for p in parts])
                for k, name in enumerate(self.fields)]

    def _labels_from_indices(self, frames: List[dict]):
        """Packed labels of frames stored alike -> (idx [B,words] on the device, pack) when they are stored at the size the targets are wanted at, else
        (None, the label frames expanded and resized: soccdpt_pack_expand -> soccdpt_vis_resize), ready for soccdpt_data_targets."""
        from ..lib import op_pack_expand
        pack = frames[0]["seg_pack"]
        idx = self._upload(frames, "seg_index")
        Hl, Wl = pack.shapes["labels"]
        if not self.to_camera_size or (Hl, Wl) == (int(self.height), int(self.width)):
            return idx, pack
        palette = self._cached(("palette", pack.palette.tobytes()), lambda: torch.from_numpy(pack.palette).to(self.device))
        return None, self._to_camera_size(op_pack_expand(idx, pack.k, palette, Hl, Wl))

    def _assemble_alike(self, frames: List[dict]) -> list:
        from ..lib import op_data_targets, op_pack_targets
        if not hasattr(self.img_transform, "batch"):
            raise TypeError("the datasets need the GPU input transform of model.loader.load_transforms (an object with .batch); got " +
                            type(self.img_transform).__name__)
        with torch.cuda.device(self.device):
            out = {}
            out["x_raw"] = self._upload(frames, "rgb_frame")
            out["x"] = self.img_transform.batch(out["x_raw"])
            want_seg, want_disp = "y_seg" in self.fields, "y_disp" in self.fields
            disp = self._upload(frames, "disparity_frame") if want_disp else None
            idx = None
            if want_seg and "seg_index" in frames[0]:
                idx, seg = self._labels_from_indices(frames)
            elif want_seg:
                seg = self._upload(frames, "seg_frame")
            else:       # the kernel reads labels whatever it writes: a depth-only item hands it blank ones and asks for no label output
                seg = self._cached(("blank", tuple(disp.shape)), lambda: torch.zeros(tuple(disp.shape) + (3,), dtype=torch.uint8, device=self.device))
            colors = self._cached("colors", lambda: torch.from_numpy(self.colors).to(self.device))
            if want_seg or disp is not None:
                # flip stays 0: the frames are already in the iterator's (channel-flipped) order.  The reference's OccupancyProcessor.process_frame flips
                # such a frame once and rgb_seg_to_class flips it back before comparing, so its class ids are those of the frame as it is here.
                wants = dict(want_onehot=want_seg, want_unmatched=want_seg, want_class_map=want_seg and self.keep_class_map)
                if idx is not None:      # seg is the pack: the targets straight from the indices
                    palette = self._cached(("palette", seg.palette.tobytes()), lambda: torch.from_numpy(seg.palette).to(self.device))
                    Hl, Wl = seg.shapes["labels"]
                    t = op_pack_targets(idx, seg.k, palette, colors, Hl, Wl, disp, **wants)
                else:
                    t = op_data_targets(seg, colors, disp, **wants)
                out["y_seg"], out["y_disp"] = t["onehot"], t["y_disp"]
                self.last_unmatched, self.last_class_map = t["unmatched"], t["class_map"]
            if want_disp:
                out["mask_disp"] = self._ones(out["y_disp"].shape)
            if want_seg:
                out["mask_seg"] = self._ones(out["y_seg"].shape)
        return [out[k] for k in self.fields]

    def batch(self, indices: Iterable[int]) -> list:
        """The items `indices` of this recording as one batch: bit-identical to torch.cat of the single items along dim 0."""
        return self.assemble(self.decode(indices))

    def __getitem__(self, frame_index):
        return self.batch([frame_index])


class BDD_Depth(BDD_Dataset):
    """[x, x_raw, mask, y]: network input, the frame as stored (for pictures), all-true mask, disparity as float32 -- at the stored size."""
    fields = ("x", "x_raw", "mask_disp", "y_disp")


class BDD_Segmentation(BDD_Dataset):
    """[x, x_raw, mask, y]: network input, the frame as stored, all-true mask, one 0 / 1 plane per class [B,C,H,W] -- at the stored size."""
    fields = ("x", "x_raw", "mask_seg", "y_seg")


class BDD_Depth_Segmentation(BDD_Dataset):
    """[x, x_raw, mask_disp, y_disp, mask_seg, y_seg], every frame resized to the camera size first."""
    fields = ("x", "x_raw", "mask_disp", "y_disp", "mask_seg", "y_seg")
    to_camera_size = True


def get_bdd_dataset(BDD_Dataset, transform, base_path: str, recordings: Optional[Sequence[str]] = None, settings_doc: Optional[str] = None,
                    **kwargs) -> torch.utils.data.ConcatDataset:
    """ConcatDataset of one BDD_Dataset per recording under base_path; `recordings` defaults to the reference's six ids.  settings_doc: the
    calibration file (default: <base_path>/calibration/pocoX3/calib.yaml when it exists, else the reference's DEFAULT_CALIB)."""
    if settings_doc is None:
        local = os.path.join(os.path.expanduser(base_path), "calibration", "pocoX3", "calib.yaml")
        settings_doc = local if os.path.isfile(local) else DEFAULT_CALIB
    ids = DEFAULT_RECORDINGS if recordings is None else tuple(recordings)
    return torch.utils.data.ConcatDataset([BDD_Dataset(dataset_path=os.path.join(base_path, str(r)), settings_doc=settings_doc, transform=transform, **kwargs)
                                           for r in ids])


# ---- batches through Subset / ConcatDataset index maps ----
def resolve_index(dataset, index: int):
    """-> (leaf dataset, index inside it) behind any nesting of torch.utils.data.Subset and ConcatDataset."""
    index = int(index)
    while True:
        if isinstance(dataset, torch.utils.data.Subset):
            dataset, index = dataset.dataset, int(dataset.indices[index])
        elif isinstance(dataset, torch.utils.data.ConcatDataset):
            if index < 0:
                index += len(dataset)
            if not 0 <= index < len(dataset):
                raise IndexError(index)
            d = bisect.bisect_right(dataset.cumulative_sizes, index)
            index -= dataset.cumulative_sizes[d - 1] if d > 0 else 0
            dataset = dataset.datasets[d]
        else:
            return dataset, index


def batch_indices(index: int, batch_size: int) -> range:
    """The reference's get_batch rule (utils/__init__.py:768-780): the batch that ENDS at `index` holds items [index - batch_size, index)."""
    return range(index - batch_size, index)


def _leaves(dataset, indices: Iterable[int]):
    pairs = [resolve_index(dataset, i) for i in indices]
    assert pairs, "an empty batch"
    for leaf, _ in pairs:
        if not isinstance(leaf, BDD_Dataset):
            raise TypeError(f"dataset_batch needs BDD datasets behind the index maps, found {type(leaf).__name__}")
    head = pairs[0][0]
    for leaf, _ in pairs:
        assert type(leaf) is type(head) and (leaf.height, leaf.width) == (head.height, head.width) and leaf.device == head.device, \
            "the recordings of one batch share the dataset class, the camera and the device"
    return head, pairs


def submit_decode(dataset, indices: Iterable[int]):
    """Start decoding a batch in the pool -> (leaf that assembles it, one future per frame).  Host work only."""
    head, pairs = _leaves(dataset, indices)
    pool = decode_pool(head.workers)
    return head, [pool.submit(leaf.batch_frame, i) for leaf, i in pairs]


def dataset_batch(dataset, indices: Iterable[int]) -> list:
    """`dataset.batch(indices)` for a BDD dataset behind Subset / ConcatDataset maps: one decode round and one set of launches for the whole batch."""
    head, futures = submit_decode(dataset, indices)
    return head.assemble([f.result() for f in futures])


class BatchPrefetcher:
    """Iterates over `batches` (an iterable of index lists into `dataset`) and yields what dataset_batch returns, in order, while the following ones
    are prepared: the frames of the next `depth` batches are being decoded by the pool's threads (host only), and the upload and the kernels of
    the next batch are already queued on a side stream when a batch is handed out, so they overlap the consumer's step.  All GPU calls happen on
    the consumer's thread; the consumer's current stream waits on the batch's event before it is returned."""

    def __init__(self, dataset, batches: Iterable[Sequence[int]], depth: int = 2):
        assert depth >= 1
        self.dataset, self.depth = dataset, int(depth)
        self._batches = iter(batches)
        self._decoding: deque = deque()      # (head, futures)
        self._ready: deque = deque()         # (tensors, event)
        self._stream: Optional[torch.cuda.Stream] = None
        self.last_unmatched: Optional[torch.Tensor] = None      # of the batch handed out last (also restored onto the leaf that assembled it)
        self.last_class_map: Optional[torch.Tensor] = None

    def _fill(self):
        while len(self._decoding) < self.depth:
            try:
                idx = next(self._batches)
            except StopIteration:
                return
            self._decoding.append(submit_decode(self.dataset, idx))

    def _launch_next(self):
        if not self._decoding:
            return
        head, futures = self._decoding.popleft()
        self._fill()
        frames = [f.result() for f in futures]
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=head.device)
        with torch.cuda.stream(self._stream):
            tensors = head.assemble(frames)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        self._ready.append((tensors, ev, head, head.last_unmatched, head.last_class_map))      # the batch's own diagnostics travel with it

    def __iter__(self):
        return self

    def __next__(self) -> list:
        if not self._ready:
            self._fill()
            self._launch_next()
        if not self._ready:
            raise StopIteration
        tensors, ev, head, unmatched, class_map = self._ready.popleft()
        cur = torch.cuda.current_stream(head.device)
        cur.wait_event(ev)
        for t in tensors + [unmatched, class_map]:
            if t is not None:
                t.record_stream(cur)      # allocated on the side stream, read on the consumer's
        self._launch_next()           # the batch after this one: queued now, runs beside the consumer's step
        # assembling the next batch replaced the leaf's diagnostics; what the consumer reads after next() belongs to the batch it was handed
        self.last_unmatched, self.last_class_map = unmatched, class_map
        head.last_unmatched, head.last_class_map = unmatched, class_map
        return tensors
