"""Device time of the occupancy-evaluation kernels (csrc/occ_eval.hip) on the default 256 x 256 x 32 x 3 grid, one line per case (DESIGN.md section 12 quotes them).
HIP events, 20 warm-up and 2000 timed calls per device case (200 for the host-side numpy comparison); the sides of a comparison alternate in blocks of 500 inside
one process, and each figure is the mean over the four blocks with their minimum and maximum in brackets.

  pack        f32 dense -> bits, 1 and 8 rows, against occ_expand (bits -> dense f32, the same bytes in the other direction) and the HBM rate
  points      packed bits -> [N,4] f64 list (count + scan + write, capacity form: no host synchronisation; and the two-call form with its one read-back)
              against (a) the torch formulation on the dense grid on the same device and (b) the numpy specification on a host copy of the dense grid
  iou         packed / packed, 8 rows

    python tools/occ_eval_bench.py
"""
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from soccdpt_amd.lib import Engine, _stream_ptr, load_library, make_config  # noqa: E402
from soccdpt_amd.utils.occupancy import occupancy_bits_to_points, occupancy_iou, occupancy_shape_f32, pack_occupancy  # noqa: E402
from tests import occ_eval_refs as R  # noqa: E402

GRID, SCALE, C = (256, 256, 32), (2.0, 2.0, 0.666), 3
NCELL = GRID[0] * GRID[1] * GRID[2] * C
WARM, BLOCK, BLOCKS, HOST_CALLS = 20, 500, 4, 200
dev = torch.device("cuda:0")


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3       # us


def alternate(fns):
    """fns: {name: callable}; -> {name: us per call} over BLOCKS x BLOCK calls each, the sides taking turns."""
    for f in fns.values():
        for _ in range(WARM):
            f()
    torch.cuda.synchronize()
    per = {k: [] for k in fns}
    for _ in range(BLOCKS):
        for k, f in fns.items():
            per[k].append(timed(f, BLOCK) / BLOCK)
    return {k: Stat(sum(v) / len(v), min(v), max(v)) for k, v in per.items()}


class Stat(float):
    """Mean over the blocks; prints as `mean [min-max]`."""
    def __new__(cls, mean, lo, hi):
        o = super().__new__(cls, mean)
        o.lo, o.hi = lo, hi
        return o

    def __format__(self, spec):
        return f"{float(self):{spec}} [{self.lo:{spec}}-{self.hi:{spec}}]"


def torch_points(occ, g64, shape64):
    """What a user would write with torch ops on the same device."""
    idx = (occ >= 0.5).nonzero()
    idx = idx[torch.sort(idx[:, 3], stable=True).indices]
    xyz = (idx[:, :3].double() / g64 * shape64).float().double()
    return torch.cat([xyz, idx[:, 3:4].double()], dim=1)


def main():
    eng = Engine(make_config("swin2t16_256", C, 256, True, True, 1920, 1080, 1250.6, 1254.8, 978.4, 562.1, GRID, occupancy_shape_f32(GRID, SCALE),
                             (10000.0, 50000.0, 800.0), (55.0, -20.0, 15.0), (7.0, 0, 0)), dev)
    rng = np.random.default_rng(0)
    # ---- pack against occ_expand ----
    for rows in (1, 8):
        dense = (torch.rand((rows,) + GRID + (C,), device=dev) < 0.01).float()
        bits = pack_occupancy(dense[0])
        out = torch.empty_like(dense)
        packed = torch.empty((rows, bits.shape[1]), dtype=torch.int32, device=dev)
        L, st = load_library(), _stream_ptr(dev)
        t = alternate({"pack": lambda: L.soccdpt_occ_pack(dense.data_ptr(), 0, rows, NCELL, 0.5, 0, packed.data_ptr(), st), "expand": lambda: eng.occ_expand(bits.reshape(-1), rows, out)})
        nbytes = rows * NCELL * 4
        print(f"pack f32 rows={rows}: {t['pack']:.1f} us, {nbytes / t['pack'] / 1e6:.2f} TB/s of the {nbytes / 1e6:.1f} MB read | occ_expand B={rows}: "
              f"{t['expand']:.1f} us, {nbytes / t['expand'] / 1e6:.2f} TB/s of the bytes written | pack / expand rate {t['expand'] / t['pack']:.2f}")
        assert torch.equal(packed, pack_occupancy(dense)) and torch.equal(packed[0], bits[0])
        del dense, out
    # ---- points from bits ----
    golden = np.load(os.path.join(REPO, "tests", "golden", "e2e_B1_tanh_oracle.npz"))["occ_bits"]
    g64 = torch.tensor(GRID, dtype=torch.float64, device=dev)
    shape64 = torch.from_numpy(occupancy_shape_f32(GRID, SCALE).astype(np.float64)).to(dev)
    for name, words in (("forward golden (707 cells)", golden), ("density 1e-2", R.pack_bits(rng.random(NCELL) < 1e-2))):
        bits = torch.from_numpy(words.view(np.int32).copy()).to(dev)
        occ = torch.from_numpy(R.unpack_bits(words, NCELL).reshape(GRID + (C,)).astype(np.float32)).to(dev)
        n = int(R.unpack_bits(words, NCELL).sum())
        assert torch.equal(occupancy_bits_to_points(bits, GRID, SCALE, C).points, torch_points(occ, g64, shape64))
        t = alternate({"bits": lambda: occupancy_bits_to_points(bits, GRID, SCALE, C, max_points=n),
                       "bits2": lambda: occupancy_bits_to_points(bits, GRID, SCALE, C),
                       "torch": lambda: torch_points(occ, g64, shape64)})
        for _ in range(3):
            R.points_from_mask(occ.cpu().numpy() >= 0.5, GRID, SCALE, C)
        t0 = time.perf_counter()
        for _ in range(HOST_CALLS):
            R.points_from_mask(occ.cpu().numpy() >= 0.5, GRID, SCALE, C)
        host = (time.perf_counter() - t0) * 1e6 / HOST_CALLS
        print(f"points {name}, N={n}: bits (count + scan + write, capacity form) {t['bits']:.1f} us | bits, two-call form with the read-back {t['bits2']:.1f} us | "
              f"torch on the dense grid {t['torch']:.1f} us ({t['torch'] / t['bits']:.1f}x) | numpy spec with the D2H copy {host:.0f} us ({host / t['bits']:.0f}x)")
    # ---- iou counts ----
    pred = torch.from_numpy(np.stack([R.pack_bits(rng.random(NCELL) < 1e-2) for _ in range(8)]).view(np.int32)).to(dev)
    gt = torch.from_numpy(np.stack([R.pack_bits(rng.random(NCELL) < 1e-2) for _ in range(8)]).view(np.int32)).to(dev)
    counts = torch.empty((8, C, 4), dtype=torch.int64, device=dev)
    L, st = load_library(), _stream_ptr(dev)
    t = alternate({"iou": lambda: L.soccdpt_occ_iou_counts(pred.data_ptr(), 8, gt.data_ptr(), 8, NCELL, C, counts.data_ptr(), st)})
    assert torch.equal(counts, occupancy_iou(pred, gt, C)["counts"])
    print(f"iou counts packed / packed rows=8: {t['iou']:.1f} us per call, memset + kernel ({2 * 8 * pred.shape[1] * 4 / 1e6:.1f} MB read)")


if __name__ == "__main__":
    main()
