"""Generates tests/golden/vis_color_segmentation.npz by running THE REFERENCE'S OWN color_segmentation (SOccDPT/utils/__init__.py:35-43) on seeded
[12,16,C] masks for C = 3 and C = 5.  It needs the reference checkout next to this repository (the stub recipe for its optional imports is
oracle/make_golden.py import_reference, as in tests/tools/make_golden_occ_points.py), so it runs where the other goldens are generated, never as part
of the test suite; the file it writes is data (inputs and recorded outputs).

    python tests/tools/make_golden_vis.py

Per case `c<C>_masks` f32 [12,16,C], `c<C>_colors` u8 [C,3], `c<C>_image` u8 [12,16,3].  The masks are seeded uniform values with about a third
of the pixels set in more than one class (the later class must win), a band of values exactly 0.5 (must not match) and values just above it."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from oracle.make_golden import import_reference  # noqa: E402


def main():
    import_reference()
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            sys.modules["tqdm"] = types.ModuleType("tqdm")
            sys.modules["tqdm"].tqdm = lambda it, **k: it
    from SOccDPT.utils import color_segmentation
    out = {}
    for C, seed in ((3, 301), (5, 305)):
        rng = np.random.default_rng(seed)
        masks = rng.random((12, 16, C)).astype(np.float32)
        masks[3, :, :] = 0.5                                     # exactly the threshold: no class matches
        masks[4, :, C - 1] = np.nextafter(np.float32(0.5), np.float32(1.0))
        masks[5, ::2, 0] = 0.9                                   # overlaps with whatever the later classes say
        colors = rng.integers(1, 256, size=(C, 3)).astype(np.uint8)
        class_2_color = {c: tuple(int(v) for v in colors[c]) for c in range(C)}
        frame = np.zeros((12, 16, 3), dtype=np.uint8)
        img = color_segmentation(masks, frame, class_2_color)
        assert img.dtype == np.uint8 and img.shape == (12, 16, 3) and not img[3].any()
        overlaps = int(((masks > 0.5).sum(axis=2) > 1).sum())
        assert overlaps > 20
        out[f"c{C}_masks"], out[f"c{C}_colors"], out[f"c{C}_image"] = masks, colors, img
        print("C", C, "pixels with more than one class", overlaps)
    path = os.path.join(REPO, "tests", "golden", "vis_color_segmentation.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
