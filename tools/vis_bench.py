"""Device time of the evaluation pictures (csrc/visualise.hip) at camera resolution, 1080 x 1920, written to profiles/vis_cost.json (DESIGN.md section 12.2
quotes it).  HIP events, 20 warm-up and 100 timed calls per case in four blocks of 25; the sides of a comparison alternate block by block inside one
process, and each figure is the mean over the blocks with their minimum and maximum.  Every case cycles through enough distinct inputs to exceed the
256 MiB Infinity Cache, so the bytes come from HBM.  `hbm_fraction` = bytes the algorithm needs / time / the achievable HBM rate (6.3 TB/s).

  primitives   min / max, colour map (given min / max), class colours (C = 3), the tile copy, a 384 x 384 -> camera resize, the half-size shrink
  panel        evaluation_panel with ground truth (k = 3): tiles written in place, against the same pictures made separately and joined with torch.cat
  cpu          the same panel through tests/visualise_refs.py on the host, inputs already there: plain numpy element-wise and indexing work, which
               runs on one thread however many the process may use (16 here)
  --alt-minmax-lib PATH   also time min / max through another build of the library with the same entry points (an experiment that is not shipped),
               each build in fresh child processes that take turns, and record it under `minmax_alternative`; without the flag a
               `minmax_alternative` record already in the file is carried over, marked as such (the one committed compares the one-stage form
               that ended in atomics with the two-stage form that is shipped; the former was deleted)

    python tools/vis_bench.py [--alt-minmax-lib PATH --alt-label NAME]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W, C = 1080, 1920, 3
WARM, BLOCK, BLOCKS = 20, 25, 4
HBM_ACHIEVABLE = 6.3e12          # bytes / s: the microarchitecture notes' measured copy rate of the 8 TB/s HBM3E
CACHE_BYTES = 256 << 20
COLORS = {0: (0, 0, 0), 1: (0, 0, 142), 2: (220, 20, 60)}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n       # us per call


def alternate(fns):
    """{name: callable} -> {name: dict(us, us_min, us_max)} over BLOCKS x BLOCK calls each, the sides taking turns."""
    for f in fns.values():
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(BLOCKS):
        for k, f in fns.items():
            per[k].append(timed(f, BLOCK))
    return {k: dict(us=round(sum(v) / len(v), 2), us_min=round(min(v), 2), us_max=round(max(v), 2)) for k, v in per.items()}


class Cycle:
    """Calls fn(item) on the next of `items` each time."""

    def __init__(self, fn, items):
        self.fn, self.items, self.i = fn, items, 0

    def __call__(self):
        self.fn(self.items[self.i])
        self.i = (self.i + 1) % len(self.items)


def copies(make, nbytes):
    return [make(i) for i in range(CACHE_BYTES // nbytes + 2)]


def with_rate(stat, nbytes):
    stat = dict(stat, bytes=int(nbytes))
    stat["hbm_fraction"] = round(nbytes / (stat["us"] * 1e-6) / HBM_ACHIEVABLE, 3)
    return stat


def minmax_case(dev):
    from soccdpt_amd.utils.visualise import disparity_minmax
    frames = copies(lambda i: torch.rand((1, H, W), device=dev) * 0.08 + 0.001, H * W * 4)
    return with_rate(alternate({"minmax": Cycle(disparity_minmax, frames)})["minmax"], H * W * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minmax-only", action="store_true", help="print the min / max figure as one JSON line and stop (what the child processes run)")
    ap.add_argument("--alt-minmax-lib", default=None)
    ap.add_argument("--alt-label", default="alternative")
    ap.add_argument("--shipped-label", default="shipped")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.minmax_only:
        print(json.dumps(minmax_case(dev)))
        return
    from soccdpt_amd.lib import _call, _ptr, csrc_sha
    from soccdpt_amd.utils import visualise as V
    from tests import visualise_refs as R
    out = dict(shape=[H, W], classes=C, warmup=WARM, timed=BLOCK * BLOCKS, blocks=BLOCKS, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE, csrc_sha=csrc_sha(),
               device=torch.cuda.get_device_name(0), note="every case cycles through more than 256 MiB of distinct inputs")
    px = H * W
    prim = {}
    # ---- primitives ----
    prim["minmax"] = minmax_case(dev)
    frames = copies(lambda i: torch.rand((1, H, W), device=dev) * 0.08 + 0.001, px * 4)
    mm = V.disparity_minmax(frames[0])
    lut = V._lut(dev)
    dst = V._Rect.whole(1, H, W, dev)
    prim["colorize_given_minmax"] = with_rate(alternate({"c": Cycle(lambda d: _call("soccdpt_vis_colorize", _ptr(d), _ptr(mm), _ptr(lut), 1, H, W, _ptr(dst.buf), *dst.args,
                                                                                    device=dev), frames)})["c"], px * 7)
    prim["colorize_disparity"] = with_rate(alternate({"c": Cycle(V.colorize_disparity, frames)})["c"], px * 11)      # the frame is read twice
    del frames
    segs = copies(lambda i: torch.rand((1, C, H, W), device=dev), px * 4 * C)
    prim["color_masks"] = with_rate(alternate({"c": Cycle(lambda s: V.color_masks(s, COLORS), segs)})["c"], px * (4 * C + 3))
    del segs
    imgs = copies(lambda i: torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev), px * 3)
    prim["tile_copy"] = with_rate(alternate({"c": Cycle(lambda m: V.resize_bgr(m, (W, H)), imgs)})["c"], px * 6)
    del imgs
    small = [torch.randint(0, 256, (384, 384, 3), dtype=torch.uint8, device=dev) for _ in range(4)]
    prim["resize_384_to_camera"] = with_rate(alternate({"c": Cycle(lambda m: V.resize_bgr(m, (W, H)), small)})["c"], 384 * 384 * 3 + px * 3)
    prim["resize_384_to_camera"]["note"] = "includes building and uploading the two tap tables"
    panels = copies(lambda i: torch.randint(0, 256, (2 * H, 3 * W, 3), dtype=torch.uint8, device=dev), px * 18)
    prim["shrink_half_panel_k3"] = with_rate(alternate({"c": Cycle(lambda m: V.shrink_half(m, swap_rb=True), panels)})["c"], px * 18 + px * 18 // 4)
    del panels
    out["primitives"] = prim

    # ---- the k = 3 panel: tiles in place against separate pictures + concatenate ----
    def make(i):
        g = torch.Generator(device=dev).manual_seed(i)
        return dict(frame=torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g),
                    dp=torch.rand((H, W), device=dev, generator=g) * 0.08, dg=torch.rand((H, W), device=dev, generator=g) * 0.1,
                    sp=torch.rand((C, H, W), device=dev, generator=g), sg=torch.rand((C, H, W), device=dev, generator=g))
    sets = copies(make, px * (3 + 8 + 8 * C))

    def in_place(s):
        return V.evaluation_panel(s["frame"], s["dp"], s["sp"], COLORS, disp_gt=s["dg"], seg_gt=s["sg"])

    def concatenated(s):
        top = torch.cat([s["frame"], V.colorize_disparity(s["dp"]), V.colorize_disparity(s["dg"])], dim=1)
        bottom = torch.cat([s["frame"], V.color_masks(s["sp"][None], COLORS)[0], V.color_masks(s["sg"][None], COLORS)[0]], dim=1)
        return V.shrink_half(torch.cat([top, bottom], dim=0), swap_rb=True)
    assert torch.equal(in_place(sets[0]), concatenated(sets[0]))
    t = alternate({"in_place": Cycle(in_place, sets), "concatenate": Cycle(concatenated, sets)})
    # inputs once (the two depth frames twice: min / max, then colour), the 2H x 3W panel written once and read once, the result written
    need = px * (3 * 2 + 2 * 8 + 2 * 4 * C) + px * 18 * 2 + px * 18 // 4
    out["panel_k3"] = dict(in_place=with_rate(t["in_place"], need), concatenate=dict(t["concatenate"]), launches_in_place=11,
                           concatenate_over_in_place=round(t["concatenate"]["us"] / t["in_place"]["us"], 2))
    # ---- host baseline ----
    s = {k: v.cpu().numpy() for k, v in sets[0].items()}
    want = in_place(sets[0]).cpu().numpy()
    host = []
    for i in range(4):
        t0 = time.perf_counter()
        got = R.panel(s["frame"], s["dp"], s["sp"], COLORS, disp_gt=s["dg"], seg_gt=s["sg"])
        host.append((time.perf_counter() - t0) * 1e6)
    assert np.array_equal(got, want)
    host = host[1:]
    out["panel_k3"]["cpu_numpy"] = dict(us=round(sum(host) / len(host)), us_min=round(min(host)), us_max=round(max(host)), threads_allowed=int(os.environ["OMP_NUM_THREADS"]),
                                        threads_used=1, calls=len(host),
                                        note="tests/visualise_refs.py panel(), inputs already on the host, one warm-up call; numpy element-wise and indexing "
                                             "operations do not use the other threads, so this is a single-threaded restatement, not a tuned host path")
    out["panel_k3"]["cpu_over_gpu"] = round(out["panel_k3"]["cpu_numpy"]["us"] / t["in_place"]["us"], 1)
    # ---- min / max through another build ----
    if args.alt_minmax_lib:
        runs = {args.shipped_label: [], args.alt_label: []}
        for _ in range(2):
            for label, lib in ((args.shipped_label, None), (args.alt_label, args.alt_minmax_lib)):
                env = dict(os.environ)
                if lib:
                    env["SOCCDPT_LIB_PATH"] = os.path.abspath(lib)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--minmax-only"], env=env, check=True, capture_output=True, text=True, timeout=300)
                runs[label].append(json.loads(r.stdout.strip().splitlines()[-1]))
        out["minmax_alternative"] = dict(runs=runs, note="fresh child processes taking turns, two per build; the alternative build is not shipped")
    path = os.path.join(REPO, "profiles", "vis_cost.json")
    if "minmax_alternative" not in out and os.path.exists(path):
        old = json.load(open(path)).get("minmax_alternative")
        if old:
            out["minmax_alternative"] = dict(old, carried_over="from an earlier run of this tool; not re-measured in this one")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
