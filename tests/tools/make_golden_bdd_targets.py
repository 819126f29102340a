"""Generates tests/golden/bdd_targets.npz by running THE REFERENCE'S OWN rgb_seg_to_bool (SOccDPT/datasets/bengaluru_driving_dataset.py:67-76) and
rgb_seg_to_class (SOccDPT/datasets/bdd_helper.py:10-25) on seeded label images.  It needs the reference checkout next to this repository (the stub
recipe for its optional imports is oracle/make_golden.py import_reference, as in tests/tools/make_golden_vis.py, plus a torchvision.transforms stub and
cv2.cvtColor as the channel flip it is for COLOR_BGR2RGB), so it runs where the other goldens are generated, never as part of the test suite; the file
it writes is data (inputs and recorded outputs).

    python tests/tools/make_golden_bdd_targets.py

Per case `<name>_seg` u8 [H,W,3], `<name>_bool` bool [H,W,3] (rgb_seg_to_bool), `<name>_class` int64 [H,W] (rgb_seg_to_class with the reference's
color_2_class).  The images are 5 x 7 and 37 x 53, drawn from the three class colours, their channel-reversed forms (142,0,0) and (60,20,220) -- which
match nothing in rgb_seg_to_bool and do match in rgb_seg_to_class -- and the near misses (0,0,141) and (220,20,61)."""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from oracle.make_golden import import_reference  # noqa: E402
from tests.bdd_targets_refs import label_frames  # noqa: E402


def main():
    import_reference()
    sys.modules["cv2"].cvtColor = lambda img, code: np.ascontiguousarray(img[:, :, ::-1])
    sys.modules["cv2"].resize = None
    if "torchvision.transforms" not in sys.modules:
        sys.modules["torchvision.transforms"] = types.ModuleType("torchvision.transforms")
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    if not hasattr(sys.modules["torchvision.transforms"], "Compose"):
        sys.modules["torchvision.transforms"].Compose = lambda l: l
    from SOccDPT.datasets.bdd_helper import rgb_seg_to_class
    from SOccDPT.datasets.bengaluru_driving_dataset import color_2_class, rgb_seg_to_bool
    out = {}
    for name, (H, W), seed in (("small", (5, 7), 57), ("odd", (37, 53), 3753)):
        seg = label_frames(1, H, W, seed)[0]
        b = rgb_seg_to_bool(seg)
        c = rgb_seg_to_class(seg, color_2_class)
        assert b.dtype == bool and b.shape == (H, W, 3) and c.shape == (H, W)
        out[f"{name}_seg"], out[f"{name}_bool"], out[f"{name}_class"] = seg, b, c.astype(np.int64)
        print(name, "unmatched", int((~b.any(axis=2)).sum()), "class counts", np.bincount(c.reshape(-1), minlength=3).tolist())
    path = os.path.join(REPO, "tests", "golden", "bdd_targets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
