"""Cost of the per-frame occupancy mode (csrc/occ_frames.hip, SOccDPT(occupancy_per_frame=True)) against the union mode, measured in ONE process on one
device (DESIGN.md section 12 quotes the figures; the JSON goes to profiles/).  For dpt_swin2_tiny_256 and dpt_swin2_base_384 at B = 8:

  (a) the union-mode forward (SOccDPT_V3(compute_occ=True), the forward every earlier profile describes), with its run-to-run spread
  (b) the per-frame forward
  (c) the voxelise_frames launch alone (us, bytes/s of its algorithmic bytes) against the fused project_voxelise launch at the same B
  (d) occ_expand_frames against occ_expand at the same B (the same bytes stored)

Timing: HIP events around blocks of calls, every case warmed up first, the sides of a comparison taking turns block by block; a figure is the mean over
the blocks with [min-max] of the block means -- that bracket is the run-to-run spread the comparisons are judged against.  The kernels' own device
times (c, d) come from the library's per-dispatch profiler (soccdpt_profile_enable) in a pass of its own.  The two relations the mode was accepted on
are asserted at the end: (c) below project_voxelise, (d) within the spread of occ_expand.

    python tools/occ_frames_bench.py [--out profiles/occ_frames_cost.json] [--models dpt_swin2_tiny_256,dpt_swin2_base_384]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from tests.golden_inputs import proj_inputs  # noqa: E402

GRID, C, B = (256, 256, 32), 3, 8
NCELL = GRID[0] * GRID[1] * GRID[2] * C
HC, WC = 1080, 1920
dev = torch.device("cuda:0")


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n       # us per call


def alternate(fns, warm, block, blocks):
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            per[k].append(timed(f, block))
    return {k: dict(mean_us=sum(v) / len(v), min_us=min(v), max_us=max(v), blocks=[round(t, 2) for t in v]) for k, v in per.items()}


def fmt(s):
    return f"{s['mean_us']:.1f} us [{s['min_us']:.1f}-{s['max_us']:.1f}]"


def kernel_times(eng, fns, n):
    """Device time per launch of each profiler family (begin -> end of the dispatch itself), n calls of every fn."""
    eng.profile_enable(True)
    for f in fns:
        for _ in range(n):
            f()
    torch.cuda.synchronize()
    stats = eng.profile_collect()
    eng.profile_enable(False)
    return {k: dict(us_per_launch=v["ms"] * 1e3 / v["launches"], launches=v["launches"], bytes_per_launch=v["bytes"] / v["launches"]) for k, v in stats.items()}


def model_case(model_type):
    from soccdpt_amd.model.SOccDPT import SOccDPT_V3
    from soccdpt_amd.model.spec import MODEL_TYPE_TO_BACKBONE, backbone_image_size
    from soccdpt_amd.utils.synth import synth_input, synth_state_dict, write_synth_calib
    backbone = MODEL_TYPE_TO_BACKBONE[model_type]
    img = backbone_image_size(backbone)
    calib = write_synth_calib(os.path.join(tempfile.mkdtemp(), "calib.yaml"))
    sd = synth_state_dict(backbone, alias_pretrained=True)
    nets = {}
    for name, per_frame in (("union", False), ("per_frame", True)):
        with contextlib.redirect_stdout(io.StringIO()):
            m = SOccDPT_V3(sigmoid=False, load_depth=False, camera_intrinsics_yaml=calib, compute_occ=True, model_type=model_type, occupancy_per_frame=per_frame)
        m.load_state_dict(sd, strict=False)
        nets[name] = m.eval().to(dev)
    x = synth_input(B, size=img, seed0=0).to(dev)
    res = {"image": img}
    with torch.no_grad():
        out_u, out_p = nets["union"](x), nets["per_frame"](x)
        torch.cuda.synchronize()
        assert all(torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(out_u[:3], out_p[:3]))
        assert torch.equal(nets["union"].last_occ_bits, nets["per_frame"].last_occ_bits)
        rows = nets["per_frame"].last_occ_frame_bits
        res["set_bits_union"] = int((out_u[3][0] > 0).sum().item())
        res["set_bits_per_frame"] = [int((out_p[3][b] > 0).sum().item()) for b in range(B)]
        del out_u, out_p
        # (a) / (b): whole forwards, alternating; the union side appears twice so that its own repeat-to-repeat difference is on record
        t = alternate({"union": lambda: nets["union"](x), "per_frame": lambda: nets["per_frame"](x), "union_again": lambda: nets["union"](x)}, warm=10, block=20, blocks=5)
    res["forward"] = t
    print(f"{model_type} B={B}: (a) union forward {fmt(t['union'])}, repeated {fmt(t['union_again'])} | (b) per-frame forward {fmt(t['per_frame'])} "
          f"(+{t['per_frame']['mean_us'] - t['union']['mean_us']:.1f} us)")
    # (c) / (d) on this model's network outputs
    eng = nets["per_frame"]._engine(dev)
    inv, seg = nets["per_frame"].network(x)
    res.update(stage_case(eng, inv, seg, f"{model_type} network outputs"))
    del rows
    return res


def stage_case(eng, inv, seg, label):
    S = inv.shape[1]
    inv_up = torch.empty((B, HC, WC), device=dev)
    seg_up = torch.empty((B, C, HC, WC), device=dev)
    pts = torch.empty((B, HC, WC, 3), device=dev)
    union = torch.empty((eng.occ_words(),), dtype=torch.int32, device=dev)
    rows = torch.empty((B, eng.occ_words()), dtype=torch.int32, device=dev)
    occ = torch.empty((B,) + GRID + (C,), device=dev)
    project = lambda: eng.project(inv, seg, inv_up, seg_up, pts, union, clear_bits=True)             # noqa: E731  (the launch of soccdpt_forward)
    project_noocc = lambda: eng.project(inv, seg, inv_up, seg_up, pts, None)                         # noqa: E731  (the launch of soccdpt_forward_frames)
    vox = lambda: eng.voxelise_frames(inv_up, seg, rows, clear_bits=True)                            # noqa: E731
    expand = lambda: eng.occ_expand(union, B, occ)                                                   # noqa: E731
    expand_f = lambda: eng.occ_expand_frames(rows, B, occ)                                           # noqa: E731
    project()
    vox()
    torch.cuda.synchronize()
    acc = rows[0].clone()
    for b in range(1, B):
        acc |= rows[b]
    assert torch.equal(acc, union), "OR of the frame rows differs from the fused kernel's union"
    t = alternate({"project_voxelise": project, "voxelise_frames": vox, "project_without_marking": project_noocc, "occ_expand": expand,
                   "occ_expand_frames": expand_f, "occ_expand_again": expand}, warm=20, block=200, blocks=5)
    k = kernel_times(eng, [project, vox, expand, expand_f], 200)
    vb = k["voxelise_frames"]["bytes_per_launch"]
    out = {"calls_with_memset": t, "kernels": k, "voxelise_frames_TBps": vb / k["voxelise_frames"]["us_per_launch"] / 1e6,
           "occ_expand_frames_TBps": B * NCELL * 4 / k["occ_expand_frames"]["us_per_launch"] / 1e6, "occ_expand_TBps": B * NCELL * 4 / k["occ_expand"]["us_per_launch"] / 1e6}
    print(f"{label} ({S} px, B={B}): (c) voxelise_frames kernel {k['voxelise_frames']['us_per_launch']:.1f} us = {out['voxelise_frames_TBps']:.2f} TB/s of {vb / 1e6:.1f} MB "
          f"(call with its clear {fmt(t['voxelise_frames'])}) | project_voxelise kernel {k['project_voxelise']['us_per_launch']:.1f} us (call {fmt(t['project_voxelise'])}, "
          f"without marking {fmt(t['project_without_marking'])})")
    print(f"{label}: (d) occ_expand_frames kernel {k['occ_expand_frames']['us_per_launch']:.1f} us, call {fmt(t['occ_expand_frames'])} | occ_expand kernel "
          f"{k['occ_expand']['us_per_launch']:.1f} us, call {fmt(t['occ_expand'])}, repeated {fmt(t['occ_expand_again'])}")
    return out


def check(case, label, failures):
    k, t = case["kernels"], case["calls_with_memset"]
    if not k["voxelise_frames"]["us_per_launch"] < k["project_voxelise"]["us_per_launch"]:
        failures.append(f"{label}: (c) voxelise_frames {k['voxelise_frames']['us_per_launch']:.1f} us is not below project_voxelise {k['project_voxelise']['us_per_launch']:.1f} us")
    hi = max(t["occ_expand"]["max_us"], t["occ_expand_again"]["max_us"])
    if not t["occ_expand_frames"]["mean_us"] <= hi:
        failures.append(f"{label}: (d) occ_expand_frames {t['occ_expand_frames']['mean_us']:.1f} us lies above the spread of occ_expand (max block {hi:.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--models", default="dpt_swin2_tiny_256,dpt_swin2_base_384")
    args = ap.parse_args()
    from oracle import soccdpt_ref as R
    from soccdpt_amd.lib import Engine, make_config
    result = {"device": torch.cuda.get_device_name(0), "B": B, "camera": [WC, HC], "grid": list(GRID) + [C], "models": {}, "stage_inputs": {}}
    cam, cfg = R.Camera(), R.ProjConfig()
    for S, bb in ((256, "swin2t16_256"), (384, "swin2b24_384")):     # (c) / (d) on the scattered scenes of the projection tests
        eng = Engine(make_config(bb, C, 256, False, True, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cfg.grid_size, cfg.occupancy_shape(),
                                 cfg.pc_scale, cfg.pc_shift, cfg.correction_angle), dev)
        inv, seg = proj_inputs(seed=21, B=B, S=S)
        result["stage_inputs"][f"proj_inputs_seed21_{S}"] = stage_case(eng, inv.to(dev), seg.to(dev), f"proj_inputs(seed=21, S={S})")
    for mt in [m for m in args.models.split(",") if m]:
        result["models"][mt] = model_case(mt)
    failures = []
    for name, case in list(result["stage_inputs"].items()) + list(result["models"].items()):
        check(case, name, failures)
    result["relations_hold"] = not failures
    result["failures"] = failures
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    for line in failures:
        print("RELATION FAILED:", line)
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
