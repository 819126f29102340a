"""Writes tests/golden/swin_large_parent_kernels.npz: the outputs of two soccdpt_op_fwd_aux calls (patch_embed 1x32x96 with an fp16 copy, ln_residual
c1024_m7) as integer views of their bits, from the library given with --lib.  Run on an MI355X with a libsoccdpt_hip.so BUILT FROM THE COMMIT BEFORE
patch_embed / ln_residual were widened for dpt_swin2_large_384; tests/test_swin_large_kernels_gpu.py holds the current library to these bits.

    python tests/tools/make_golden_swin_large_kernels.py --lib /path/to/parent/libsoccdpt_hip.so [--out tests/golden/swin_large_parent_kernels.npz]
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
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "swin_large_parent_kernels.npz"))
    args = ap.parse_args()
    import soccdpt_amd.lib as lib
    lib.LIB_PATH = os.path.abspath(args.lib)
    lib.load_library()
    from tests import swin_large_refs as L
    from tests.test_fwd_aux_gpu import run_twice
    dev = torch.device("cuda:0")
    out = {}
    for label, call in L.parent_calls():
        got, path = run_twice(call, dev)
        for name, t in got.items():
            out[f"{label}.{name}"] = L.bits(t).numpy()
        print(label, "path", hex(path), {k: tuple(v.shape) for k, v in got.items()})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes from", lib.LIB_PATH)


if __name__ == "__main__":
    main()
