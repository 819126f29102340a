"""Frame packs: one file per recording that holds every frame already decoded.

The PNGs of a recording never change, and decoding the 24 of a batch costs several training steps.  `write_pack` decodes a recording once, with the
reader's own `decode_color` / `decode_disparity`, and `FramePack` maps the result: `frame(i)` hands out views of the file, no copy and no decode.
rgb and disparity are stored raw, exactly the bytes the decoders return.  Label frames hold a handful of colours and are stored as indices into one
palette per recording, 1, 2, 4 or 8 bits per pixel (include/soccdpt_pack.h gives the bit layout; soccdpt_pack_targets builds the targets from the
indices); a recording with more than 256 label colours keeps raw labels.

Layout, little-endian, offsets in bytes (HEADER below):

    0     8s   magic b"SOCCFPK\\0"
    8     u32  version (VERSION)
    12    u32  N, the number of frames
    16    3 x {u32 height, u32 width, u32 dtype, u32 encoding}   rgb, disparity, labels
               dtype 0 / 1 / 2 = u8 / u16 / f32 (SOCCDPT_DATA_*); encoding 0 = raw, k = 1 / 2 / 4 / 8 = palette indices of k bits (labels only)
    64    u32  P, the palette's entries (0 with raw labels)
    68    u32  reserved, 0
    72    3 x u64  bytes of one record of rgb, disparity, labels (before alignment)
    96    u64  offset of the CSV text; 104 u64 its length
    112   u64  offset of the source table; 120 u64 offset of the record offset table
    128   u64  size of the whole file
    136   u64  reserved, 0
    144   u8 [256][3]  palette, sorted by c0 | c1 << 8 | c2 << 16 (channels as decode_color returns them); entries past P are zero
    912   source table  (3 N + 1) x {u64 size, u64 mtime_ns}: the CSV, then rgb, disparity, labels PNG of frame 0, of frame 1, ...
          record offset table  N x 3 x u64: rgb, disparity, labels record of frame 0, of frame 1, ...
          the CSV file's bytes
          records, each aligned to 4096 bytes; padding is zero

A pack is current when the version matches and every recorded size and mtime_ns equals the file's stat.  A missing, stale or truncated pack is never
read silently: `FramePackError` names the first file that differs (`.path`), and the file's size is checked against the offset table before anything
is mapped."""
from __future__ import annotations

import csv
import io
import mmap
import os
import struct
from typing import Dict, List, Optional, Tuple

import numpy as np

from .bdd_helper import _number, decode_color, decode_disparity

MAGIC = b"SOCCFPK\0"
VERSION = 1
SUFFIX = ".sfp"
ALIGN = 4096
HEADER = struct.Struct("<8sII12III3Q6Q")
PALETTE_OFFSET = HEADER.size                     # 144
SOURCES_OFFSET = PALETTE_OFFSET + 256 * 3        # 912
MAX_PALETTE = 256
DTYPES = (np.uint8, np.uint16, np.float32)       # code -> dtype (SOCCDPT_DATA_U8 / _U16 / _F32)
STREAMS = ("rgb", "disparity", "labels")
assert HEADER.size == 144 and SOURCES_OFFSET % 8 == 0


class FramePackError(RuntimeError):
    """A pack that is missing, truncated, of another version, or older than its recording.  `path` is the file the message names."""

    def __init__(self, message: str, path: str):
        super().__init__(message)
        self.path = path


# ---- palette indices ----
def index_bits(P: int) -> int:
    """The smallest k of 1, 2, 4, 8 with 2^k >= P (1 <= P <= 256)."""
    assert 1 <= P <= MAX_PALETTE
    return next(k for k in (1, 2, 4, 8) if (1 << k) >= P)


def record_words(npix: int, k: int) -> int:
    return (npix * k + 31) // 32


def color_keys(frame: np.ndarray) -> np.ndarray:
    """u8 [...,3] -> u32 [...]: c0 | c1 << 8 | c2 << 16."""
    f = np.asarray(frame)
    return f[..., 0].astype(np.uint32) | (f[..., 1].astype(np.uint32) << 8) | (f[..., 2].astype(np.uint32) << 16)


def keys_to_palette(keys: np.ndarray) -> np.ndarray:
    """sorted distinct u32 keys -> u8 [P,3]."""
    keys = np.asarray(keys, dtype=np.uint32)
    return np.stack([keys & 255, (keys >> 8) & 255, (keys >> 16) & 255], axis=-1).astype(np.uint8)


def pack_indices(idx: np.ndarray, k: int) -> np.ndarray:
    """Indices (any integer dtype, values < 2^k), row-major -> u32 [ceil(n k / 32)]: index p in bits [(p k) mod 32, + k) of word p k // 32."""
    idx = np.asarray(idx).reshape(-1)
    per = 32 // k
    words = record_words(idx.size, k)
    padded = np.zeros(words * per, dtype=np.uint32)
    padded[: idx.size] = idx
    shifts = (np.arange(per, dtype=np.uint32) * np.uint32(k))
    return np.bitwise_or.reduce(padded.reshape(words, per) << shifts, axis=1).astype("<u4")


def unpack_indices(words: np.ndarray, k: int, n: int) -> np.ndarray:
    """The inverse of pack_indices: the first n indices of a record, as u8."""
    b = np.ascontiguousarray(np.asarray(words, dtype="<u4")).view(np.uint8)
    if k == 8:
        return b[:n].copy()
    bits = np.unpackbits(b, bitorder="little")[: n * k].reshape(n, k)
    return (bits << np.arange(k, dtype=np.uint8)).sum(axis=1, dtype=np.uint8)


# ---- where a pack lives, which files it stands for ----
def pack_path(recording_path: str, where=True) -> str:
    """The pack of a recording: `where` True -> <recording>/<id>.sfp, a string -> <where>/<id>.sfp."""
    recording_path = os.path.expanduser(str(recording_path)).rstrip("/")
    rec_id = recording_path.split("/")[-1]
    folder = recording_path if where is True or where is None else os.path.expanduser(str(where))
    return os.path.join(folder, rec_id + SUFFIX)


def _parse_csv(text: bytes) -> Tuple[List[str], List[list]]:
    rows = list(csv.reader(io.StringIO(text.decode(), newline="")))
    assert rows and len(rows[0]) >= 2, "a header row and at least two columns (the second is the timestamp)"
    return rows[0], [[_number(v) for v in r] for r in rows[1:] if r]


def source_files(recording_path: str, csv_dat: List[list], file_extension: str = ".png") -> List[str]:
    """The files a pack stands for, in the source table's order: the CSV, then rgb, disparity and label PNG of every frame."""
    recording_path = os.path.expanduser(str(recording_path)).rstrip("/")
    out = [os.path.join(recording_path, recording_path.split("/")[-1] + ".csv")]
    for row in csv_dat:
        name = str(int(row[1])) + file_extension
        out += [os.path.join(recording_path, d, name) for d in ("rgb_img", "depth_img", "seg_img")]
    return out


def _stat(path: str) -> Tuple[int, int]:
    st = os.stat(path)
    return int(st.st_size), int(st.st_mtime_ns)


# ---- writing ----
def write_pack(recording_path: str, out_dir: Optional[str] = None, workers: int = 8) -> str:
    """Decode the recording at `recording_path` once and write its pack (to <recording>/<id>.sfp, or into out_dir) -> the pack's path.  Two passes
    over the label frames: the first collects their distinct colours (the palette has to be known before an index can be written), the second writes
    the records; both decode through the reader's pool of `workers` threads.  Written under a temporary name and renamed when complete."""
    from .bengaluru_driving_dataset import decode_pool
    pool = decode_pool(workers)
    recording_path = os.path.expanduser(str(recording_path)).rstrip("/")
    out = pack_path(recording_path, True if out_dir is None else out_dir)
    csv_file = os.path.join(recording_path, recording_path.split("/")[-1] + ".csv")
    with open(csv_file, "rb") as f:
        csv_text = f.read()
    _, csv_dat = _parse_csv(csv_text)
    N = len(csv_dat)
    assert N > 0, f"{csv_file}: no frames"
    sources = source_files(recording_path, csv_dat)
    stats = [_stat(p) for p in sources]          # taken before the decode: a file rewritten meanwhile makes the pack stale, not wrong
    rgb_files, disp_files, seg_files = sources[1::3], sources[2::3], sources[3::3]

    # pass 1: the palette, and the label frames' size
    def distinct(path):
        a = decode_color(path)
        return a.shape[:2], np.unique(color_keys(a))
    seg_shape, keys = None, np.zeros(0, dtype=np.uint32)
    for path, (shape, u) in zip(seg_files, pool.map(distinct, seg_files)):
        if seg_shape is None:
            seg_shape = shape
        if shape != seg_shape:
            raise ValueError(f"{path}: a pack holds label frames of one size, this one is {shape[1]} x {shape[0]} after {seg_shape[1]} x {seg_shape[0]}")
        keys = np.union1d(keys, u)
    raw_labels = keys.size > MAX_PALETTE
    P, k = (0, 0) if raw_labels else (int(keys.size), index_bits(int(keys.size)))
    palette = np.zeros((MAX_PALETTE, 3), dtype=np.uint8)
    if not raw_labels:
        palette[:P] = keys_to_palette(keys)

    first_rgb, first_disp = decode_color(rgb_files[0]), decode_disparity(disp_files[0])
    shapes = [first_rgb.shape[:2], first_disp.shape, seg_shape]
    disp_code = [np.dtype(t) for t in DTYPES].index(first_disp.dtype)
    rec_bytes = [first_rgb.nbytes, first_disp.nbytes, seg_shape[0] * seg_shape[1] * 3 if raw_labels else 4 * record_words(seg_shape[0] * seg_shape[1], k)]

    offsets_off = SOURCES_OFFSET + 16 * len(sources)
    csv_off = offsets_off + 24 * N
    up = lambda v: (v + ALIGN - 1) // ALIGN * ALIGN
    offsets, at = np.zeros((N, 3), dtype="<u8"), up(csv_off + len(csv_text))
    for i in range(N):
        for s in range(3):
            offsets[i, s] = at
            at = up(at + rec_bytes[s])
    file_bytes = at
    streams = [shapes[0][0], shapes[0][1], 0, 0, shapes[1][0], shapes[1][1], disp_code, 0, shapes[2][0], shapes[2][1], 0, k]
    header = HEADER.pack(MAGIC, VERSION, N, *streams, P, 0, *rec_bytes, csv_off, len(csv_text), SOURCES_OFFSET, offsets_off, file_bytes, 0)

    # pass 2: the records
    def records(i):
        rgb, disp, seg = decode_color(rgb_files[i]), decode_disparity(disp_files[i]), decode_color(seg_files[i])
        for what, a, shape, dtype, path in (("rgb", rgb, shapes[0], np.uint8, rgb_files[i]), ("disparity", disp, shapes[1], first_disp.dtype, disp_files[i])):
            if a.shape[:2] != tuple(shape) or a.dtype != dtype:
                raise ValueError(f"{path}: a pack holds {what} frames of one size and type, this one is {a.dtype} {a.shape[1]} x {a.shape[0]}")
        if not raw_labels:
            seg = pack_indices(np.searchsorted(keys, color_keys(seg).reshape(-1)), k)
        return rgb.tobytes(), disp.tobytes(), seg.tobytes()

    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + f".tmp{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            f.write(header)
            f.write(palette.tobytes())
            f.write(np.array(stats, dtype="<u8").tobytes())
            f.write(offsets.tobytes())
            f.write(csv_text)
            chunk = 4 * int(workers)      # decoded frames held at a time
            for start in range(0, N, chunk):
                for i, recs in zip(range(start, N), pool.map(records, range(start, min(N, start + chunk)))):
                    for s in range(3):
                        assert len(recs[s]) == rec_bytes[s]
                        f.seek(int(offsets[i, s]))
                        f.write(recs[s])
            f.truncate(file_bytes)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return out


# ---- reading ----
class FramePack:
    """The mmap reader of one pack.  Opening checks the magic, the version and the file's size against the header and the offset table (before anything
    is mapped); `check_current` checks it against the recording's files.  `frame(i)` returns read-only views of the mapping."""

    def __init__(self, path: str):
        self.path = path = os.path.expanduser(str(path))
        if not os.path.isfile(path):
            raise FramePackError(f"{path}: no such frame pack (python -m soccdpt_amd.scripts.pack_recordings writes it)", path)
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            head = f.read(HEADER.size)
            if len(head) < HEADER.size or head[:8] != MAGIC:
                raise FramePackError(f"{path}: not a frame pack (truncated header or wrong magic)", path)
            (_, version, N, *rest) = HEADER.unpack(head)
            if version != VERSION:
                raise FramePackError(f"{path}: frame pack version {version}, this reader reads version {VERSION}; write the pack again", path)
            streams, P, _, rec_bytes = rest[:12], rest[12], rest[13], rest[14:17]
            csv_off, csv_len, sources_off, offsets_off, file_bytes, _ = rest[17:]
            tables_end = max(csv_off + csv_len, sources_off + 16 * (3 * N + 1), offsets_off + 24 * N)
            if size < tables_end or size != file_bytes:
                raise FramePackError(f"{path}: truncated frame pack: {size} bytes on disk, its header says {file_bytes}", path)
            f.seek(PALETTE_OFFSET)
            palette = np.frombuffer(f.read(3 * MAX_PALETTE), dtype=np.uint8).reshape(MAX_PALETTE, 3)
            f.seek(sources_off)
            self.sources = np.frombuffer(f.read(16 * (3 * N + 1)), dtype="<u8").reshape(3 * N + 1, 2)
            f.seek(offsets_off)
            self.offsets = np.frombuffer(f.read(24 * N), dtype="<u8").reshape(N, 3).astype(np.int64)
            f.seek(csv_off)
            self.csv_text = f.read(csv_len)
            self.N = int(N)
            self.shapes = {s: (int(streams[4 * j]), int(streams[4 * j + 1])) for j, s in enumerate(STREAMS)}
            self.k, self.P = int(streams[11]), int(P)
            if streams[6] >= len(DTYPES) or self.k not in (0, 1, 2, 4, 8) or (self.k and not 1 <= self.P <= (1 << self.k)):
                raise FramePackError(f"{path}: not a frame pack this reader understands (disparity type {streams[6]}, k = {self.k}, P = {self.P})", path)
            self.disp_dtype = np.dtype(DTYPES[streams[6]])
            self.raw_labels = self.k == 0
            self.palette = palette[: self.P].copy()
            self.rec_bytes = tuple(int(b) for b in rec_bytes)
            Hl, Wl = self.shapes["labels"]
            want = (self.shapes["rgb"][0] * self.shapes["rgb"][1] * 3, self.shapes["disparity"][0] * self.shapes["disparity"][1] * self.disp_dtype.itemsize,
                    Hl * Wl * 3 if self.raw_labels else 4 * record_words(Hl * Wl, self.k))
            if self.rec_bytes != want:
                raise FramePackError(f"{path}: record sizes {self.rec_bytes} do not follow from the frame sizes ({want})", path)
            if N and (int(self.offsets.min()) < tables_end or int((self.offsets + np.array(self.rec_bytes)).max()) > size or (self.offsets % ALIGN).any()):
                raise FramePackError(f"{path}: truncated frame pack: a record of its offset table lies outside its {size} bytes", path)
            self.csv_columns, self.csv_dat = _parse_csv(self.csv_text)
            if len(self.csv_dat) != N:
                raise FramePackError(f"{path}: {N} frames but {len(self.csv_dat)} CSV rows", path)
            self._map = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
        self._buf = np.frombuffer(self._map, dtype=np.uint8)

    def __len__(self) -> int:
        return self.N

    @property
    def words_per_frame(self) -> int:
        return self.rec_bytes[2] // 4

    def _record(self, i: int, s: int) -> np.ndarray:
        at = int(self.offsets[i, s])
        return self._buf[at: at + self.rec_bytes[s]]

    def frame(self, i: int) -> Dict[str, np.ndarray]:
        """Views of frame i: 'rgb' u8 [H,W,3] and 'disparity' [H,W] as decode_color / decode_disparity return them; 'labels' u32 [words] palette indices,
        or u8 [H,W,3] when the pack keeps raw labels."""
        if not 0 <= i < self.N:
            raise IndexError(i)
        labels = self._record(i, 2)
        return {"rgb": self._record(i, 0).reshape(self.shapes["rgb"] + (3,)),
                "disparity": self._record(i, 1).view(self.disp_dtype).reshape(self.shapes["disparity"]),
                "labels": labels.reshape(self.shapes["labels"] + (3,)) if self.raw_labels else labels.view("<u4")}

    def labels_rgb(self, i: int) -> np.ndarray:
        """The label frame u8 [H,W,3], the bytes decode_color returns for its PNG (a host palette lookup; raw labels are copied)."""
        labels = self.frame(i)["labels"]
        if self.raw_labels:
            return labels.copy()
        H, W = self.shapes["labels"]
        return self.palette[unpack_indices(labels, self.k, H * W)].reshape(H, W, 3)

    def check_current(self, recording_path: str) -> None:
        """Raise FramePackError, naming the first file that differs, unless every file the pack was made from has its recorded size and mtime_ns."""
        files = source_files(recording_path, self.csv_dat)
        for path, (size, mtime) in zip(files, self.sources):
            try:
                now = _stat(path)
            except OSError:
                raise FramePackError(f"{self.path} is stale: {path} is gone", path) from None
            if now != (int(size), int(mtime)):
                raise FramePackError(f"{self.path} is stale: {path} changed since the pack was written (size {now[0]} / mtime_ns {now[1]}, "
                                     f"packed {int(size)} / {int(mtime)})", path)

    def close(self) -> None:
        self._buf = None
        try:
            self._map.close()
        except BufferError:      # views are still alive; the mapping goes with them
            pass


def open_current(recording_path: str, where=True) -> FramePack:
    """The current pack of a recording, or FramePackError naming what is missing, truncated, of another version or changed."""
    pack = FramePack(pack_path(recording_path, where))
    pack.check_current(recording_path)
    return pack


def verify_pack(recording_path: str, where=True, workers: int = 8) -> int:
    """Decode every PNG of the recording again and compare it with the pack byte for byte -> the number of frames compared; FramePackError names the
    first PNG whose frame differs."""
    from .bengaluru_driving_dataset import decode_pool
    pack = open_current(recording_path, where)
    files = source_files(recording_path, pack.csv_dat)

    def differs(i) -> Optional[str]:
        f = pack.frame(i)
        for path, want, got in ((files[1 + 3 * i], decode_color(files[1 + 3 * i]), f["rgb"]),
                                (files[2 + 3 * i], decode_disparity(files[2 + 3 * i]), f["disparity"]),
                                (files[3 + 3 * i], decode_color(files[3 + 3 * i]), pack.labels_rgb(i))):
            if want.shape != got.shape or want.dtype != got.dtype or want.tobytes() != got.tobytes():
                return path
        return None
    for bad in decode_pool(workers).map(differs, range(len(pack))):
        if bad is not None:
            raise FramePackError(f"{pack.path}: frame differs from {bad}", bad)
    return len(pack)
