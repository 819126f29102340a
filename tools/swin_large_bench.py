"""Full-forward time of dpt_swin2_large_384 beside dpt_swin2_base_384, in one process, on synthetic weights and frames (bench.py's --model-type choices
do not include the large model).  Per model, batch size (1, 8) and arithmetic (f16, mixed, f16x3, f32): warm-up forwards, then several blocks of
forwards, each block timed by a host clock around work that ends in a device synchronise; min / median / max of the blocks' ms per forward.  No shipped
precision map exists for dpt_swin2_large_384, so its "mixed" row runs every group in x3 until a calibration has run; --calibrate derives a map from six
synthetic frames (4 select, 2 hold out), reports its cost, and times "mixed_calibrated" too.

    python tools/swin_large_bench.py [--out profiles/swin2_large_384_forward.json] [--calibrate] [--blocks 5] [--iters 10] [--modes f16,mixed,f16x3,f32]

--model-type dpt_swin_large_384 times the Swin-V1-L model instead, beside dpt_swin2_large_384, with the same protocol (default --out
profiles/swin_large_384_forward.json), and adds `kernel_shares`: the library's per-family event timing (soccdpt_profile_*) of its fp16 forward at each
batch size, with the share of the pre-norm LayerNorm and merge-LN launches in the network's kernel time.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# --model-type -> (the model timed, the model it is timed beside)
MODELS = {"dpt_swin2_large_384": (("dpt_swin2_large_384", "swin2l24_384"), ("dpt_swin2_base_384", "swin2b24_384")),
          "dpt_swin_large_384": (("dpt_swin_large_384", "swinl12_384"), ("dpt_swin2_large_384", "swin2l24_384"))}


def build(model_type, sd, precision, dev, calib):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    with contextlib.redirect_stdout(io.StringIO()):
        m = SOccDPT_V3(sigmoid=True, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, model_type=model_type, precision=precision)
        m.load_state_dict(sd, strict=False)
        return m.eval().to(dev)


def time_forward(m, x, warmup, blocks, iters):
    for _ in range(warmup):
        m(x)
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(iters):
            m(x)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / iters)
    return {"min_ms": min(ms), "median_ms": statistics.median(ms), "max_ms": max(ms), "blocks": blocks, "iters": iters}


def kernel_shares(m, x, iters):
    """Per-family event times of `iters` network forwards (ms per forward) and the share of the Swin-V1 block's own LayerNorm launches."""
    eng = m._engine(x.device)
    m.network(x)
    torch.cuda.synchronize()
    eng.profile_enable(True)
    for _ in range(iters):
        m.network(x)
    torch.cuda.synchronize()
    stats = eng.profile_collect()
    eng.profile_enable(False)
    total = sum(v["ms"] for v in stats.values())
    fam = {k: {"ms_per_forward": v["ms"] / iters, "launches_per_forward": v["launches"] / iters, "share": v["ms"] / total} for k, v in sorted(stats.items(), key=lambda kv: -kv[1]["ms"])}
    return {"kernel_ms_per_forward": total / iters, "ln_prenorm_share": fam.get("ln_prenorm", {}).get("share"), "merge_ln_share": fam.get("merge_ln", {}).get("share"),
            "window_attention_sdp_share": fam.get("window_attention_sdp", {}).get("share"), "families": fam}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-type", choices=sorted(MODELS), default="dpt_swin2_large_384")
    ap.add_argument("--out", default=None)
    ap.add_argument("--calibrate", action="store_true")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--modes", default="f16,mixed,f16x3,f32")
    ap.add_argument("--batches", default="1,8")
    args = ap.parse_args()
    subject = args.model_type
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "swin2_large_384_forward.json" if subject == "dpt_swin2_large_384" else "swin_large_384_forward.json")
    if not torch.cuda.is_available():
        raise SystemExit("tools/swin_large_bench.py measures on an MI355X: no GPU visible")
    from soccdpt_amd.lib import PREC_F16, PREC_F16X3, PREC_F32, PREC_MIXED
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    prec = {"f16": PREC_F16, "mixed": PREC_MIXED, "f16x3": PREC_F16X3, "f32": PREC_F32}
    modes = [s for s in args.modes.split(",") if s]
    batches = [int(b) for b in args.batches.split(",")]
    dev = torch.device("cuda:0")
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    res = {"what": "full forward (network + projection + occupancy), ms per forward: min / median / max over blocks of forwards ending in a device synchronise",
           "device": torch.cuda.get_device_name(0), "note": f"{subject} has no shipped precision map: 'mixed' runs every group in x3 until calibrated",
           "rows": [], "calibration": None}
    for model_type, backbone in MODELS[subject]:
        sd = synth_state_dict(backbone, alias_pretrained=True)
        xs = {B: synth_input(B, size=384, seed0=40).to(dev) for B in batches}
        for mode in modes:
            m = build(model_type, sd, prec[mode], dev, calib)
            for B in batches:
                row = dict(model=model_type, mode=mode, B=B, map=m.precision_map_source() if mode == "mixed" else None, **time_forward(m, xs[B], args.warmup, args.blocks, args.iters))
                row["frames_per_s"] = B * 1e3 / row["median_ms"]
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
            if mode == "f16" and model_type == subject and subject == "dpt_swin_large_384":
                res["kernel_shares"] = {f"B{B}": kernel_shares(m, xs[B], args.iters) for B in batches}
                print(json.dumps({k: {kk: v[kk] for kk in ("kernel_ms_per_forward", "ln_prenorm_share", "merge_ln_share", "window_attention_sdp_share")}
                                  for k, v in res["kernel_shares"].items()}), flush=True)
            if mode == "mixed" and args.calibrate and model_type == subject:
                frames = synth_input(6, size=384, seed0=200).to(dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rep = m.calibrate_precision(frames, budget=5e-4)
                torch.cuda.synchronize()
                rep = {k: (v if isinstance(v, (int, float, str, dict, type(None))) else str(v)) for k, v in rep.items()}
                res["calibration"] = {"seconds": time.perf_counter() - t0, "frames": 6, "budget": 5e-4, "source_after": m.precision_map_source(), "report": rep}
                print(json.dumps(res["calibration"]), flush=True)
                for B in batches:
                    row = dict(model=model_type, mode="mixed_calibrated", B=B, map=m.precision_map_source(), **time_forward(m, xs[B], args.warmup, args.blocks, args.iters))
                    row["frames_per_s"] = B * 1e3 / row["median_ms"]
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
            del m
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
