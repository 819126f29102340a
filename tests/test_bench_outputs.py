"""bench.py's plain run and --dump-outputs: the CPU half checks the writer (float32 files inside the byte budget, outputs above their share
written as a sample at seeded indices that depend on the name and shape only); the GPU half runs a plain bench line twice."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_BUDGET_BYTES", 64_000)
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.randn(3, 50, generator=g), "big": torch.randn(40, 1000, generator=g),
              "mask": torch.rand(20, 1000, generator=g) > 0.9, "wide": torch.randn(10, generator=g, dtype=torch.float64), "absent": None}
    b.dump_outputs(str(tmp_path / "a"), arrays)
    b.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "mask.npy", "small.npy", "wide.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    assert got["small"].dtype == np.float32 and np.array_equal(got["small"], arrays["small"].numpy().reshape(-1))
    assert got["wide"].dtype == np.float64 and np.array_equal(got["wide"], arrays["wide"].numpy())
    share = (64_000 - 256 * 4) // 4
    assert got["big"].dtype == np.float32 and got["big"].size == share // 4 < arrays["big"].numel()
    assert np.isin(got["big"], arrays["big"].numpy()).all()                       # a sample of the elements, not a reduction
    assert got["mask"].size == share // 4 and set(np.unique(got["mask"])) <= {0.0, 1.0}
    for f in files:                                                                # same input -> same indices, same files
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs_repeat(gpu_device, tmp_path):
    """`bench.py --steps K` times exactly K steps and prints the headline fields without the --full objects; --dump-outputs writes the four
    outputs of the forward, and a second run with the same arguments writes the same values (seeded inputs and weights)."""
    lines = []
    for tag in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--prewarm", "2", "--batch", "2",
                            "--dump-outputs", str(tmp_path / tag)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    d = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["higher_is_better"] is True
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) / d["value"] < 1e-3
    for k in ("roofline", "kernels", "repeats", "latency_b1", "f16_operands", "pipelined", "other_weights"):
        assert k not in d, k
    assert d["cpu_baseline"] is None and "--full" in d["cpu_baseline_note"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["inv_depth.npy", "occupancy.npy", "points.npy", "segmentation.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64_000_000
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0
        assert np.array_equal(a, b, equal_nan=True), n
