"""python -m soccdpt_amd.scripts.pack_recordings -b BASE [--recordings ...] [--out DIR] [--workers N] [--verify]

Writes the frame pack (<id>.sfp, datasets/frame_pack.py) of every recording under BASE: each PNG is decoded once, here, and the
datasets then map the pack instead (`--frame_pack` of train_SOccDPT / eval_SOccDPT, `frame_pack=` of the dataset classes).  `--verify` writes nothing:
it decodes every PNG again and compares it with the pack byte for byte, and exits with status 1 naming the first file that differs.  Host only."""
from __future__ import annotations

import argparse
import os
import sys
import time


def build_parser() -> argparse.ArgumentParser:
    from ..datasets.bengaluru_driving_dataset import DEFAULT_WORKERS
    parser = argparse.ArgumentParser(description="Write or verify the frame packs of Bengaluru recordings")
    parser.add_argument("-b", "--base_path", required=True, help="Base path to dataset")
    parser.add_argument("--recordings", nargs="*", default=None, help="recording ids under --base_path (default: the reference's six)")
    parser.add_argument("--out", default=None, metavar="DIR", help="directory for the packs (default: inside each recording)")
    parser.add_argument("--workers", default=DEFAULT_WORKERS, type=int, help="decode threads (1 .. 16)")
    parser.add_argument("--verify", action="store_true", help="compare existing packs with the PNGs instead of writing them")
    return parser


def main(args) -> int:
    from ..datasets.bengaluru_driving_dataset import DEFAULT_RECORDINGS
    from ..datasets.frame_pack import FramePack, FramePackError, verify_pack, write_pack
    base = os.path.expanduser(args.base_path)
    for rec in (DEFAULT_RECORDINGS if args.recordings is None else args.recordings):
        path, t0 = os.path.join(base, str(rec)), time.perf_counter()
        if args.verify:
            try:
                n = verify_pack(path, True if args.out is None else args.out, workers=args.workers)
            except FramePackError as e:
                print(f"{rec}: FAILED: {e}", file=sys.stderr)
                return 1
            print(f"{rec}: {n} frames equal their PNGs ({time.perf_counter() - t0:.1f} s)")
        else:
            out = write_pack(path, args.out, workers=args.workers)
            pack = FramePack(out)
            labels = "raw labels" if pack.raw_labels else f"{pack.P} label colours at {pack.k} bits"
            print(f"{rec}: {out}: {len(pack)} frames, {os.path.getsize(out)} bytes, {labels} ({time.perf_counter() - t0:.1f} s)")
            pack.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(build_parser().parse_args()))
