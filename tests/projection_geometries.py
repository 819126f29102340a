"""Shared table, inputs and checks of the projection-stage geometry tests (tests/test_projection_geometries_cpu.py,
tests/test_projection_geometry_gpu.py): cameras, network-output sizes, grids and rotations that reach every form launch_project
(csrc/projection.hip) chooses between, with the C oracle (oracle/cref.py) as the bit-exact reference.

`python -m tests.projection_geometries G3 D0` runs the eng.project check of those rows in this process and exits non-zero on any mismatch:
the environment-selected forms (SOCCDPT_PROJECT_ROWS8 / SOCCDPT_PROJECT_ROWS1 are read once per process) are tested through it."""
from __future__ import annotations

import functools
import sys
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import cref, soccdpt_ref as R
from tests.golden_inputs import proj_inputs

ROWS4, ROWS8, ROWS1, VEC4, VEC1 = "project_rowsR_kernel<R=4>", "project_rowsR_kernel<R=8>", "project_rows_kernel", "project_kernel<3,4>", "project_kernel<3,1>"
FORMS = (ROWS4, ROWS8, ROWS1, VEC4, VEC1)
GUARD = 4096              # sentinel-filled elements before and after every guarded output
F_SENTINEL = -1234.5
I_SENTINEL = 0x5A5A5A5A


@dataclass(frozen=True)
class Geometry:
    id: str
    cam_size: Tuple[int, int]          # camera W x H
    map_hw: Tuple[int, int]            # network output h x w
    grid: Tuple[int, int, int] = (256, 256, 32)
    scale: Tuple[float, float, float] = (2.0, 2.0, 0.666)
    angles: Tuple[float, float, float] = (7.0, 0.0, 0.0)
    form: str = ROWS4                  # the form of launch_project this row must reach (no environment switch set)
    B: int = 2
    pc_scale: Tuple[float, float, float] = R.ProjConfig().pc_scale
    pc_shift: Tuple[float, float, float] = R.ProjConfig().pc_shift

    @property
    def calib(self) -> dict:
        """The default intrinsics scaled to the frame, under the keys of the calibration YAML."""
        W, H = self.cam_size
        return {"Camera.fx": 1250.6 * W / 1920.0, "Camera.fy": 1254.8 * H / 1080.0, "Camera.cx": 978.4 * W / 1920.0, "Camera.cy": 562.1 * H / 1080.0,
                "Camera.width": W, "Camera.height": H}

    @property
    def cam(self) -> R.Camera:
        c = self.calib
        return R.Camera(fx=c["Camera.fx"], fy=c["Camera.fy"], cx=c["Camera.cx"], cy=c["Camera.cy"], width=self.cam_size[0], height=self.cam_size[1])

    @property
    def cfg(self) -> R.ProjConfig:
        return R.ProjConfig(grid_size=self.grid, scale=self.scale, pc_scale=self.pc_scale, pc_shift=self.pc_shift, correction_angle=self.angles)

    @property
    def ncell(self) -> int:
        return self.grid[0] * self.grid[1] * self.grid[2] * 3


G1 = Geometry("G1", (1028, 61), (20, 240), form=ROWS4)
G2 = Geometry("G2", (452, 250), (96, 96), (64, 48, 16), angles=(7.0, 3.0, -2.0), form=ROWS1)
G3 = Geometry("G3", (640, 362), (96, 96), (64, 48, 16), (2.0, 1.5, 0.666), (7.0, 3.0, -2.0), form=ROWS4)
G4 = Geometry("G4", (200, 120), (96, 96), (64, 64, 16), form=VEC4)
G5 = Geometry("G5", (322, 181), (64, 48), (20, 12, 7), angles=(5.0, 0.0, 0.0), form=VEC1)
G6 = Geometry("G6", (64, 40), (96, 80), (33, 21, 7), (2.0, 1.5, 0.666), (7.0, 0.0, -4.0), form=VEC4)
G7 = Geometry("G7", (1920, 1080), (384, 384), angles=(7.0, 2.0, 1.0), form=ROWS1, B=1)
G3PC = Geometry("G3pc", G3.cam_size, G3.map_hw, G3.grid, G3.scale, G3.angles, form=ROWS4, pc_scale=(8000.0, 30000.0, 500.0), pc_shift=(40.0, -10.0, 5.0))
D0 = Geometry("D0", (1920, 1080), (256, 256), form=ROWS4)   # the constructor's defaults: what the rest of the suite runs (not a table row)

TABLE = (G1, G2, G3, G4, G5, G6, G7)
GEOMETRIES = {g.id: g for g in TABLE + (G3PC, D0)}

# (case id, geometry id, input kind): every row, the G3 variant with other pc constants, and the plateau inputs
CASES = tuple((g.id, g.id, "smooth") for g in TABLE) + (("G3pc", "G3pc", "smooth"), ("G1-plateau", "G1", "plateau"), ("G3-plateau", "G3", "plateau"))
CASE_IDS = tuple(c[0] for c in CASES)
_CASES = {c[0]: c for c in CASES}
_CASES["D0"] = ("D0", "D0", "default")


# ---- the dispatch rule of launch_project, restated with its float32 arithmetic ----
def eight_row_condition(Hc: int, h: int) -> bool:
    f = np.float32
    sy = f(h) / f(Hc)
    return bool(5 + int(np.ceil(f(7) * sy)) <= 7 and f(1.0) + f(7) * sy < f(3.0))


def dispatch(Wc: int, Hc: int, h: int, w: int, rows8: bool = False, rows1: bool = False) -> str:
    f = np.float32
    vec4 = Wc % 4 == 0
    sx = f(w) / f(Wc)
    if vec4 and int(f(1024.0) * sx) + 8 <= 256:
        sy = f(h) / f(Hc)
        if rows8 and not rows1 and eight_row_condition(Hc, h):
            return ROWS8
        if not rows1 and 5 + int(np.ceil(f(3) * sy)) <= 7 and f(1.0) + f(3) * sy < f(2.0):
            return ROWS4
        return ROWS1
    return VEC4 if vec4 else VEC1


def form_of(g: Geometry, rows8: bool = False, rows1: bool = False) -> str:
    return dispatch(g.cam_size[0], g.cam_size[1], g.map_hw[0], g.map_hw[1], rows8, rows1)


# ---- inputs ----
def proj_inputs_sized(seed: int, B: int, h: int, w: int):
    """golden_inputs.proj_inputs at any map size: a smooth inverse depth in about [0.005, 0.3] planted with a zero, a negative run, NaN,
    +inf and 1e-12 (at places that exist in a 20-row map), and ScaledTanh class probabilities with exact zeros."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand((B, 1, 6, 6), generator=g) * 0.29 + 0.005
    inv = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=False)[:, 0]
    inv = inv + torch.randn((B, h, w), generator=g) * 0.002
    inv[:, h // 4, w // 8] = 0.0                         # clamp path (-> 1e-8 -> depth 1e8)
    inv[:, h // 3 + 1, w // 4:w // 4 + 3] = -0.5         # negative -> clamp
    inv[0, h // 2, w // 3] = float("nan")
    inv[B - 1, (2 * h) // 3, (3 * w) // 4] = float("inf")
    inv[B - 1, (2 * h) // 3 + 1, (3 * w) // 4] = 1e-12
    logits = torch.randn((B, 3, h, w), generator=g) * 6.0
    seg = 0.5 * torch.tanh(logits) + 0.5                 # ScaledTanh -> exact zeros for logits << 0
    return inv.contiguous(), seg.contiguous()


_CLASS_SETS = (7, 2, 7, 3, 1, 7, 4, 6, 0, 5)   # bit c = class c non-zero; along x and along y: superset -> subset -> superset, disjoint sets, none


def plateau_inputs(seed: int, B: int, h: int, w: int, blocks=(4, 8)):
    """Aimed at the run-length de-duplication of the voxel marks: the inverse depth is constant over blocks of the map (depths of 4 .. 12.5 m, so
    that tens of camera pixels and several camera rows fall into one voxel) while the set of non-zero classes changes from map pixel to map pixel,
    i.e. several times inside such a run, in both directions."""
    g = torch.Generator().manual_seed(seed)
    nby, nbx = blocks
    lo = torch.rand((B, 1, nby, nbx), generator=g) * 0.17 + 0.08
    inv = F.interpolate(lo, size=(h, w), mode="nearest")[:, 0]
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    sets = torch.tensor(_CLASS_SETS)[(xx + yy) % len(_CLASS_SETS)]
    on = torch.stack([(sets >> c) & 1 for c in range(3)]).bool()                  # [3,h,w]
    seg = torch.where(on[None], torch.rand((B, 3, h, w), generator=g) * 0.5 + 0.25, torch.zeros(()))
    return inv.contiguous(), seg.contiguous()


@functools.lru_cache(maxsize=None)
def case_inputs(case_id: str):
    """(geometry, inv [B,h,w], seg [B,3,h,w]) of one case; computed once, never modified."""
    _, gid, kind = _CASES[case_id]
    geo = GEOMETRIES[gid]
    h, w = geo.map_hw
    seed = 100 + sorted(GEOMETRIES).index(gid)
    if kind == "default":
        inv, seg = proj_inputs(seed=5, B=geo.B)
    elif kind == "plateau":
        inv, seg = plateau_inputs(seed, geo.B, h, w)
    else:
        inv, seg = proj_inputs_sized(seed, geo.B, h, w)
    return geo, inv, seg


@functools.lru_cache(maxsize=None)
def case_oracle(case_id: str):
    """cref.project of the case: dict(inv_up, seg_up, points, occ_bits); computed once, never modified."""
    geo, inv, seg = case_inputs(case_id)
    return cref.project(inv, seg, cam=geo.cam, cfg=geo.cfg)


@functools.lru_cache(maxsize=None)
def case_oracle_frames(case_id: str) -> np.ndarray:
    """[B, nwords]: the oracle's grid of each frame handed to it as a batch of one."""
    geo, inv, seg = case_inputs(case_id)
    return np.stack([cref.project(inv[b:b + 1], seg[b:b + 1], cam=geo.cam, cfg=geo.cfg, want=("occ_bits",))["occ_bits"] for b in range(geo.B)])


def same(a, b) -> bool:
    """NaN-aware bitwise-value equality of two float arrays."""
    return np.array_equal(np.nan_to_num(np.asarray(a), nan=-7.0), np.nan_to_num(np.asarray(b), nan=-7.0))


def unpack(words: np.ndarray, geo: Geometry) -> np.ndarray:
    """uint32 words -> {0,1} float32 [g0,g1,g2,3] (padding bits past the last cell dropped)."""
    flat = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:geo.ncell]
    return flat.astype(np.float32).reshape(geo.grid + (3,))


def popcount(words: np.ndarray) -> int:
    return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())


def np_bits(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


# ---- GPU side ----
def make_engine(dev, geo: Geometry = D0, compute_occ: bool = True):
    from soccdpt_amd.lib import Engine, make_config
    cam, cfg = geo.cam, geo.cfg
    c = make_config("swin2t16_256", 3, 256, False, compute_occ, cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy,
                    cfg.grid_size, cfg.occupancy_shape(), cfg.pc_scale, cfg.pc_shift, cfg.correction_angle)
    return Engine(c, dev)


class Guarded:
    """A contiguous tensor that is a slice of a larger one, with GUARD sentinel elements before and after it."""

    def __init__(self, shape, dtype, dev, fill=None):
        n = int(np.prod(shape))
        self.sentinel = F_SENTINEL if dtype == torch.float32 else I_SENTINEL
        self.whole = torch.full((GUARD + n + GUARD,), self.sentinel, dtype=dtype, device=dev)
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.fill_(fill)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def guards_intact(self) -> bool:
        s = torch.tensor(self.sentinel, dtype=self.whole.dtype, device=self.whole.device)
        return bool((self.whole[:GUARD] == s).all()) and bool((self.whole[-GUARD:] == s).all())

    def untouched(self) -> bool:
        return bool((self.whole == torch.tensor(self.sentinel, dtype=self.whole.dtype, device=self.whole.device)).all())


def run_project(eng, geo: Geometry, inv, seg, dev, want=("inv_up", "seg_up", "points", "occ_bits")):
    """eng.project into guarded outputs (occ_bits pre-filled with -1 and cleared by clear_bits=True) -> {name: Guarded}."""
    B, (W, H) = inv.shape[0], geo.cam_size
    shapes = {"inv_up": (B, H, W), "seg_up": (B, 3, H, W), "points": (B, H, W, 3)}
    out = {k: Guarded(shapes[k], torch.float32, dev) for k in shapes if k in want}
    if "occ_bits" in want:
        out["occ_bits"] = Guarded((eng.occ_words(),), torch.int32, dev, fill=-1)
    get = lambda k: out[k].t if k in out else None   # noqa: E731
    eng.project(inv.to(dev), seg.to(dev), get("inv_up"), get("seg_up"), get("points"), get("occ_bits"), clear_bits=True)
    torch.cuda.synchronize()
    return out


def project_mismatches(out: dict, ref: dict) -> list:
    """Every way the guarded outputs of run_project differ from the oracle's (an empty list: bit-exact and no stray store)."""
    bad = []
    for k, gd in out.items():
        got = np_bits(gd.t) if k == "occ_bits" else gd.t.cpu().numpy()
        if k == "occ_bits":
            if not np.array_equal(got, ref[k]):
                bad.append(f"occ_bits: {int((got != ref[k]).sum())} of {got.size} words differ ({popcount(got)} bits set, oracle {popcount(ref[k])})")
        elif not same(got, ref[k]):
            d = np.nan_to_num(got, nan=-7.0) != np.nan_to_num(ref[k], nan=-7.0)
            bad.append(f"{k}: {int(d.sum())} of {d.size} values differ, first at {tuple(int(i) for i in np.argwhere(d)[0])}")
        if not gd.guards_intact():
            bad.append(f"{k}: a guard band was written")
    return bad


def check_project_case(dev, case_id: str, expect_form: Optional[str] = None, rows8: bool = False, rows1: bool = False) -> list:
    geo, inv, seg = case_inputs(case_id)
    if expect_form is not None:
        assert form_of(geo, rows8, rows1) == expect_form, (case_id, form_of(geo, rows8, rows1))
    eng = make_engine(dev, geo)
    return project_mismatches(run_project(eng, geo, inv, seg, dev), case_oracle(case_id))


# ---- reference of soccdpt_project_backward: torch autograd through the same tail ----
def project_backward_reference(inv, seg, Hc, Wc, fx, fy, cx, cy, pc_scale, w1, w2, w3, dtype=torch.float64):
    """Gradients (d_inv, d_seg) of sum(inv_up w1) + sum(seg_up w2) [+ sum(points w3)] by torch autograd in `dtype` on the CPU: bicubic
    (align_corners=False) + clamp at 1e-8 (zero gradient where clamped), nearest, points = ((v - cx) d / fx, (u - cy) d / fy, d) with the 3-pixel
    pc_scale quirk.  Also returns the raw (unclamped) up-sampled inverse depth."""
    B = inv.shape[0]
    a = inv.to(dtype).requires_grad_(True)
    s = seg.to(dtype).requires_grad_(True)
    raw = F.interpolate(a.unsqueeze(1), size=(Hc, Wc), mode="bicubic", align_corners=False)[:, 0]
    up = torch.where(raw < 1e-8, torch.full_like(raw, 1e-8), raw)
    su = F.interpolate(s, size=(Hc, Wc), mode="nearest")
    loss = (up * w1.to(dtype)).sum() + (su * w2.to(dtype)).sum()
    if w3 is not None:
        d = 1.0 / up
        vv = torch.arange(Wc, dtype=dtype)[None, None, :]
        uu = torch.arange(Hc, dtype=dtype)[None, :, None]
        P = torch.stack([(vv - float(cx)) * d / float(fx), (uu - float(cy)) * d / float(fy), d.expand(B, Hc, Wc)], dim=-1)
        scale = torch.ones((Hc * Wc, 1), dtype=dtype)
        scale[:3, 0] = torch.tensor(pc_scale, dtype=dtype)
        loss = loss + (P * scale.reshape(1, Hc, Wc, 1) * w3.to(dtype)).sum()
    loss.backward()
    return a.grad, s.grad, raw.detach()


def rel_l2(a, b) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def main(argv) -> int:
    import os
    rows8 = bool(int(os.environ.get("SOCCDPT_PROJECT_ROWS8", "0") or 0))
    rows1 = bool(int(os.environ.get("SOCCDPT_PROJECT_ROWS1", "0") or 0))
    dev = torch.device("cuda:0")
    rc = 0
    for case_id in argv:
        geo = case_inputs(case_id)[0]
        bad = check_project_case(dev, case_id, rows8=rows8, rows1=rows1)
        print(f"{case_id}: {form_of(geo, rows8, rows1)}, oracle sets {popcount(case_oracle(case_id)['occ_bits'])} bits: " + ("bit-exact" if not bad else "; ".join(bad)))
        rc |= 1 if bad else 0
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
