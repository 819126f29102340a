"""soccdpt_prec_calibrate_ex of two builds of libsoccdpt_hip.so on the same weights and frames, compared bit for bit, and its wall time, alternated.

    python tools/calib_ab.py case <name> [inv.pt]                    one calibration with the library SOCCDPT_LIB_PATH names -> one JSON line
    python tools/calib_ab.py compare <a.so> <b.so> <out.json> [runs] every (library, case) in a fresh child process -> out.json

compare: the precision-map string (soccdpt_prec_map_get), every field of soccdpt_calib_report and the inverse depth of one forward after the
calibration must be identical between the two libraries, case by case; `salt1` is run `runs` (default 5) times per library, alternating, which gives
the wall times and each library's own run-to-run identity.  Stops at the first child that fails."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name: (model type, backbone, weights, size, frames, hold-out, budget, per_pixel_p999)
CASES = {
    "salt0": ("dpt_swin2_tiny_256", "swin2t16_256", "salt0", 256, 6, 2, 5e-4, None),
    "salt1": ("dpt_swin2_tiny_256", "swin2t16_256", "salt1", 256, 6, 2, 5e-4, None),
    "trained_like": ("dpt_swin2_tiny_256", "swin2t16_256", "trained_like", 256, 6, 2, 5e-4, None),
    "salt1_per_pixel": ("dpt_swin2_tiny_256", "swin2t16_256", "salt1", 256, 6, 2, 5e-4, 6e-4),
    "hybrid384_salt1": ("dpt_hybrid_384", "vitb_rn50_384", "salt1", 384, 3, 1, 1e-3, None),
    "salt1_b2": ("dpt_swin2_tiny_256", "swin2t16_256", "salt1", 256, 2, 1, 5e-4, None),   # tests/test_calibrate_gpu.py::test_calibration_is_deterministic
}


def _hex(v):
    """exact text of a report value: floats by their bits"""
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, dict):
        return {k: _hex(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_hex(x) for x in v]
    return v


def run_case(name, inv_path=None):
    import torch
    from soccdpt_amd.lib import PREC_MIXED
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.utils.synth import named_weights, synth_input, write_synth_calib
    model_type, backbone, weights, size, B, holdout, budget, pp = CASES[name]
    dev = torch.device("cuda:0")
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, precision=PREC_MIXED, model_type=model_type)
    m.load_state_dict(named_weights(weights, backbone), strict=False)
    m = m.eval().to(dev)
    x = synth_input(B, size=size, seed0=4).to(dev)
    m.network(x[:1])                      # engine, arenas and the first prepare are not part of the timed call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rep = m.calibrate_precision(x, budget=budget, holdout=holdout, per_pixel_p999=pp)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    inv, _ = m.network(x)
    torch.cuda.synchronize()
    inv = inv.cpu()
    if inv_path:
        torch.save(inv, inv_path)
    map_string = " ".join(f"{k}={v}" for k, v in m._engine(dev).prec_map().items())
    report = _hex(rep)
    print(json.dumps({"case": name, "library": os.environ.get("SOCCDPT_LIB_PATH", "(the tree's)"), "prec_map": map_string,
                      "prec_map_sha1": hashlib.sha1(map_string.encode()).hexdigest(), "report": report,
                      "report_sha1": hashlib.sha1(json.dumps(report, sort_keys=True).encode()).hexdigest(), "forwards": rep["forwards"],
                      "inv_sha1": hashlib.sha1(inv.numpy().tobytes()).hexdigest(), "calibrate_seconds": round(seconds, 3)}))


def _child(lib, name, inv_path):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "case", name, inv_path], env={**os.environ, "SOCCDPT_LIB_PATH": lib}, capture_output=True,
                       text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f"{lib} {name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(lib, name, d["prec_map_sha1"][:10], d["report_sha1"][:10], d["inv_sha1"][:10], d["forwards"], d["calibrate_seconds"], flush=True)
    return d


def compare(lib_a, lib_b, out_path, runs=5):
    import torch
    tmp = tempfile.mkdtemp()
    out = {"libraries": {"parent": lib_a, "branch": lib_b}, "cases": {}, "all_identical": True}

    def save():
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)

    def pair(name):
        got = {}
        for side, lib in (("parent", lib_a), ("branch", lib_b)):
            d = _child(lib, name, os.path.join(tmp, f"{side}.pt"))
            got[side] = d
        inv_equal = bool(torch.equal(torch.load(os.path.join(tmp, "parent.pt")), torch.load(os.path.join(tmp, "branch.pt"))))
        return got, inv_equal

    def record(name, got, inv_equal):
        a, b = got["parent"], got["branch"]
        same = {"prec_map_identical": a["prec_map"] == b["prec_map"], "report_identical": a["report"] == b["report"],
                "fields_that_differ": sorted(k for k in a["report"] if a["report"][k] != b["report"].get(k)), "inv_torch_equal": inv_equal}
        out["cases"][name] = {"settings": dict(zip(("model_type", "backbone", "weights", "size", "frames", "holdout", "budget", "per_pixel_p999"), CASES[name])),
                              **{side: {k: d[k] for k in ("prec_map_sha1", "report_sha1", "inv_sha1", "forwards")} for side, d in got.items()},
                              "prec_map": a["prec_map"], "report": a["report"], **same}
        if not (same["prec_map_identical"] and same["report_identical"] and inv_equal):
            out["cases"][name]["branch_prec_map"], out["cases"][name]["branch_report"] = b["prec_map"], b["report"]
            out["all_identical"] = False
        save()

    # salt1, alternated: wall times, and what each library gives from one run to the next
    times, seen = {"parent": [], "branch": []}, {"parent": set(), "branch": set()}
    for i in range(runs):
        got, inv_equal = pair("salt1")
        for side, d in got.items():
            times[side].append(d["calibrate_seconds"])
            seen[side].add((d["prec_map_sha1"], d["report_sha1"], d["inv_sha1"]))
        if i == 0:
            record("salt1", got, inv_equal)
    out["run_to_run"] = {"case": "salt1", "runs_per_library": runs, "distinct_results_parent": len(seen["parent"]), "distinct_results_branch": len(seen["branch"])}
    med = {side: statistics.median(v) for side, v in times.items()}
    out["calibrate_wall_time"] = {"case": "salt1", "unit": "s", "parent": times["parent"], "branch": times["branch"], "parent_median": med["parent"],
                                  "branch_median": med["branch"], "parent_min": min(times["parent"]), "parent_max": max(times["parent"]),
                                  "branch_median_within_parent_range": min(times["parent"]) <= med["branch"] <= max(times["parent"])}
    save()
    for name in CASES:
        if name != "salt1":
            record(name, *pair(name))
    print("all identical:", out["all_identical"], "| run to run:", out["run_to_run"], "| wall time:", out["calibrate_wall_time"])
    return 0 if out["all_identical"] else 1


if __name__ == "__main__":
    if sys.argv[1] == "case":
        run_case(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(compare(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]), sys.argv[4], int(sys.argv[5]) if len(sys.argv) > 5 else 5))
