"""numpy specification of the packed label frames (include/soccdpt_pack.h), written from the format's sentences rather than
from soccdpt_amd/datasets/frame_pack.py: one scatter / gather per pixel, no reshaping tricks.  Everything is integer and exact."""
import numpy as np


def index_bits(P):
    """The smallest k of 1, 2, 4, 8 with 2^k >= P."""
    for k in (1, 2, 4, 8):
        if (1 << k) >= P:
            return k
    raise ValueError(P)


def record_words(npix, k):
    return -(-npix * k // 32)


def palette_of(frames):
    """u8 [...,3] -> u8 [P,3]: the distinct colours, sorted by the 24-bit key c0 | c1 << 8 | c2 << 16."""
    f = np.asarray(frames, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
    keys = sorted(set((f[:, 0] | (f[:, 1] << 8) | (f[:, 2] << 16)).tolist()))
    return np.array([(key & 255, (key >> 8) & 255, key >> 16) for key in keys], dtype=np.uint8).reshape(-1, 3)


def indices_of(frame, palette):
    """u8 [H,W,3] -> the index into `palette` of every pixel, row-major [H*W]."""
    f = np.asarray(frame, dtype=np.uint8).reshape(-1, 3)
    hit = (f[:, None, :] == np.asarray(palette)[None, :, :]).all(axis=2)
    assert (hit.sum(axis=1) == 1).all(), "every pixel's colour is in the palette exactly once"
    return hit.argmax(axis=1)


def pack(idx, k, words=None):
    """Pixel p occupies bits [(p*k) mod 32, +k) of little-endian 32-bit word floor(p*k / 32); a record is ceil(n*k / 32) words (or `words`, when more
    are asked for), unused bits zero."""
    idx = np.asarray(idx, dtype=np.uint64).reshape(-1)
    assert (idx < (1 << k)).all()
    n = idx.size
    out = np.zeros(record_words(n, k) if words is None else words, dtype=np.uint64)
    p = np.arange(n, dtype=np.uint64)
    np.bitwise_or.at(out, (p * k // 32).astype(np.int64), idx << (p * k % 32))
    assert (out < (1 << 32)).all()
    return out.astype(np.uint32)


def unpack(words, k, n):
    """The n indices of a record, not clamped."""
    w = np.asarray(words, dtype=np.uint32).astype(np.uint64)
    p = np.arange(n, dtype=np.uint64)
    return ((w[(p * k // 32).astype(np.int64)] >> (p * k % 32)) & ((1 << k) - 1)).astype(np.int64)


def expand(words, k, palette, B, H, W):
    """u32 [B, words_per_frame] -> u8 [B,H,W,3] = palette[min(index, P - 1)]: what soccdpt_pack_expand writes."""
    palette = np.asarray(palette, dtype=np.uint8)
    words = np.asarray(words).reshape(B, -1)
    return np.stack([palette[np.minimum(unpack(words[b], k, H * W), len(palette) - 1)].reshape(H, W, 3) for b in range(B)])


def random_palette(P, seed, include=()):
    """u8 [P,3] of distinct colours sorted by key, holding the colours of `include` (as many as fit)."""
    rng = np.random.default_rng(seed)
    keys = set()
    for c in list(include)[:P]:
        keys.add(int(c[0]) | (int(c[1]) << 8) | (int(c[2]) << 16))
    while len(keys) < P:
        keys.add(int(rng.integers(0, 1 << 24)))
    return np.array([(key & 255, (key >> 8) & 255, key >> 16) for key in sorted(keys)], dtype=np.uint8)
