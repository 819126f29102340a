"""Writes tests/golden/depth_tail_parent.npz: the f32 bit patterns of soccdpt_op_depth_tail's output for both 16-bit formats at
tests.depth_tail_build_refs.PARENT_SHAPES, with a checksum of each case's inputs, from the library given with --lib.  Run on an MI355X with a
libsoccdpt_hip.so BUILT FROM THE COMMIT BEFORE the patch build of csrc/depth_tail.hip became separable; tests/test_depth_tail_build_gpu.py holds the
current library to these bits.

    python tests/tools/make_golden_depth_tail.py --lib /path/to/parent/libsoccdpt_hip.so [--out tests/golden/depth_tail_parent.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "depth_tail_parent.npz"))
    args = ap.parse_args()
    import soccdpt_amd.lib as lib
    lib.LIB_PATH = os.path.abspath(args.lib)
    lib.load_library()
    from tests import depth_tail_build_refs as D
    dev = torch.device("cuda:0")
    out = {}
    for fmt in D.FORMATS:
        for B, h, w in D.PARENT_SHAPES:
            inp = D.inputs(B, h, w, fmt)
            got = D.launch(inp, fmt, B, h, w, dev)
            assert bool(torch.isfinite(got).all())
            out[D.key(fmt, B, h, w) + ".out"] = D.bits(got)
            out[D.key(fmt, B, h, w) + ".in"] = np.asarray(D.input_checksum(*inp, fmt))
            print(D.key(fmt, B, h, w), tuple(got.shape), "input checksum", hex(int(out[D.key(fmt, B, h, w) + ".in"])))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes from", lib.LIB_PATH)


if __name__ == "__main__":
    main()
