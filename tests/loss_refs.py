"""TEST INFRASTRUCTURE -- float64 reference, pinned inputs and element-wise bound of the training criterion (csrc/loss.hip through
soccdpt_training_loss).  Used by tests/test_loss_refs.py (CPU) and tests/test_loss_bound_gpu.py.

Reference.  oracle/loss_ref.py is dtype-generic: `evaluate(case, torch.float64)` is `loss_ref.loss_and_grads` on the float32 inputs cast to
float64, with the scale / shift it solves; `evaluate(case, torch.float32)` is the yardstick, the same call in float32.  Where the oracle does not
apply -- alpha other than 0.5, an empty seg selection (the kernel documents 0, the oracle raises / gives NaN) -- `criterion` below states the same
function directly; tests/test_loss_refs.py holds it to the oracle at every case where both apply, and the planted faults are variants of it.

Pinned inputs (`build`): tests/golden_inputs.loss_inputs, a few planted non-positive source cells so that the 1e-8 clamp is hit, the case's
variant, and then the target is nudged until, in float64,
  * sign pins: with d = m (s p + t - y), every pair of valid neighbours at steps 1, 2, 4, 8 in both directions has
    |d_q - d_i| >= 64 * 2^-24 * (|s| max|p| + |t| + max|y|) -- the float32 evaluation of one residual carries a handful of roundings of those
    magnitudes, so no float32 evaluation can take another sign() than float64 does;
  * clamp pins: |raw - 1e-8| >= 1e-6 at every up-sampled pixel, and every case but the all-positive ones holds clamped pixels;
  * conditioning: det / (a00 a11) >= 1e-3 for every image with at least two valid pixels;
  * a representative yardstick (`forced_solve_error`): the error that float32 up-sampling alone forces on scale / shift -- an exact float64
    solve over torch's own float32 up-sampled prediction -- is at most half of the bound the yardstick gives.  torch's float32 solve adds its
    own rounding to that error, and at nine pixels the two can cancel: at 2x2 -> 1x9 with seed 7 the float32 bicubic is 8e-8 off at a pixel
    of 0.024 next to the clamp (its taps cancel), which alone moves the scale of 0.0308 by 2.9e-7, while torch's float32 result happens to
    land 3.0e-8 from float64; no float32 evaluation of the up-sampling can meet 3 x that (the kernel: 3.2e-7 on MI355X).  Every other case is
    at 0.34 of its bound or less; 2x2 -> 1x9 uses seed 11 (0.05).
The cap on unpinned pairs and pixels is 0 (`pin_report`, asserted on the CPU), so the GPU test excludes no element.

Bound (`compare`), element-wise per slice, the rule of tests/test_train_aux_gpu.py:
    |kernel - ref64| <= max(3 x max over the slice of |torch f32 - ref64|, 8 * 2^-24 * max over the slice of |ref64|)
Slices of d_inv per image: the outer two source rows / columns (clamped taps), the interior, the source cells whose bicubic footprint holds a
clamped pixel.  Slices of d_seg per image and class: cells with an empty (masked) footprint -- exactly 0 --, cells at the last source row / column,
the rest; cells at q of exactly 0 or 1 (gradients of ~1e12), and any other with q (1 - q) < 2^-20, form a slice of their own, compared
relatively, element by element.  The three loss values and every scale / shift are one-element slices, the floor relative to the value."""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Tuple

import torch
import torch.nn.functional as F

from oracle import loss_ref as LR
from tests.golden_inputs import loss_inputs

U = 2.0 ** -24
SIGN_PIN = 64 * U          # x (|s| max|p| + |t| + max|y|)
CLAMP_PIN = 1e-6
COND_MIN = 1e-3
F32_FACTOR = 3.0
FLOOR = 8 * U
CLAMP = 1e-8
STEPS = (1, 2, 4, 8)
FAULTS = {"1r": "last camera row left out of the gather into source row h - 1", "1c": "last camera column left out of the gather into source column w - 1",
          "2": "step-8 stencil without its upper neighbour", "3": "M_k of the sub-grids taken as M_0", "4": "scale / shift detached (c0..c2 dropped)",
          "5": "gradient through clamped pixels", "6": "nearest source index rounded instead of floored", "7": "BCE divided by B*C*H*W instead of the masked count",
          "8": "bicubic with align_corners=True", "9": "loss_depth_w and loss_seg_w swapped", "10": "scale / shift reported for the wrong sample"}


class Case(NamedTuple):
    B: int
    C: int
    h: int
    w: int
    H: int
    W: int
    seed: int = 7
    variant: str = ""
    compute_ss: bool = True
    alpha: float = 0.5
    w_d: float = 0.5
    w_s: float = 0.5


_FIRST = (2, 3, 8, 12, 37, 53)
CASES: Dict[str, Case] = {
    # ---- shapes: the smallest at which each edge exists
    "8x12-37x53": Case(*_FIRST),                                  # non-integer ratios, h != w, odd H, W
    "8x8-64x64": Case(3, 3, 8, 8, 64, 64),                        # exact ratio 8, every sub-grid full
    "4x4-135x67": Case(1, 1, 4, 4, 135, 67, seed=11),             # ratio 33.75 / 16.75: the footprint scan windows
    "2x2-9x7": Case(1, 3, 2, 2, 9, 7, variant="col0"),            # the launcher's minimum, every tap clamped
    "2x2-1x9": Case(1, 1, 2, 2, 1, 9, seed=11, variant="col0"),   # no vertical neighbours
    "2x2-1x1": Case(1, 1, 2, 2, 1, 1, variant="negative"),        # no neighbours at all, M_k of one point; the pixel is clamped
    "2x2-1x1-positive": Case(1, 1, 2, 2, 1, 1, variant="positive"),   # the same with the pixel unclamped: one valid pixel, B = 1
    "24x16-20x13": Case(2, 3, 24, 16, 20, 13),                    # down-sampling, source cells with no footprint
    "16x8-12x40": Case(2, 3, 16, 8, 12, 40),                      # down in one axis, up in the other
    "16x16-258x257": Case(1, 3, 16, 16, 258, 257),                # > 65536 pixels: the grid-stride loops of the first two kernels
    "300x300-40x56": Case(1, 3, 300, 300, 40, 56),                # > 262144 seg cells: the BCE kernel's grid-stride loop
    # ---- variants on the first shape
    "noss": Case(*_FIRST, compute_ss=False),
    "alpha0": Case(*_FIRST, alpha=0.0),
    "w37": Case(*_FIRST, w_d=0.3, w_s=0.7),
    "w01": Case(*_FIRST, w_d=0.0, w_s=1.0),
    "mid_empty": Case(3, 3, 8, 12, 37, 53, seed=13, variant="mid_empty"),
    "m3_zero": Case(*_FIRST, variant="m3_zero"),
    "two_pixels": Case(*_FIRST, variant="two_pixels"),
    "one_pixel": Case(*_FIRST, variant="one_pixel"),
    "seg_empty": Case(*_FIRST, variant="seg_empty"),
    "class_off": Case(*_FIRST, variant="class_off"),
    "seg_sat": Case(*_FIRST, variant="seg_sat"),
    "all_positive": Case(*_FIRST, variant="positive"),
}
UNCLAMPED_CASES = ("all_positive", "2x2-1x1-positive")
SAT_VALUES = (0.0, 1.0, 1.0 - 2.0 ** -24, 2.0 ** -30)
SAT_ROWS = {2: 0.0, 4: 1.0}          # source row of class 0 -> the target over its whole footprint


# ---------------- geometry shared by the builder, the slices and the statement ----------------
def nearest_index(n_dst: int, n_src: int, rounded: bool = False) -> torch.Tensor:
    """upsample_nearest's source index: min(floor(dst * (float) n_src / n_dst), n_src - 1), float32 like ATen and the kernel."""
    x = torch.arange(n_dst, dtype=torch.float32) * (torch.tensor(float(n_src)) / torch.tensor(float(n_dst)))
    return (torch.round(x) if rounded else torch.floor(x)).long().clamp(max=n_src - 1)


def cubic_membership(n_dst: int, n_src: int) -> torch.Tensor:
    """[n_dst, n_src] bool: source index is one of the four (border-clamped) bicubic taps of the destination index."""
    real = (n_src / n_dst) * (torch.arange(n_dst, dtype=torch.float64) + 0.5) - 0.5
    ii = torch.floor(real).long().clamp(max=n_src - 1)
    memb = torch.zeros((n_dst, n_src), dtype=torch.bool)
    for j in range(-1, 3):
        memb[torch.arange(n_dst), (ii + j).clamp(0, n_src - 1)] = True
    return memb


def upsample64(ins) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(raw, clamped, p) of the float32 network output in float64."""
    H, W = ins["y_disp"].shape[-2:]
    raw = F.interpolate(ins["inv"].double().unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False)[:, 0]
    clamped = raw < CLAMP
    return raw, clamped, torch.where(clamped, torch.full_like(raw, CLAMP), raw)


def solve64(ins, c: Case, p: torch.Tensor):
    B = p.shape[0]
    if not c.compute_ss:
        return torch.ones(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    return LR.compute_scale_and_shift(p, ins["y_disp"].double(), ins["mask_disp"].double())


# ---------------- pins ----------------
def pin_report(ins, c: Case) -> dict:
    """Everything the pins ask, in float64.  `unpinned` lists (b, r, c) of the right / lower endpoint of every unpinned pair."""
    raw, clamped, p = upsample64(ins)
    s, t = solve64(ins, c, p)
    y, m = ins["y_disp"].double(), ins["mask_disp"]
    mf = m.double()
    d = mf * (s.view(-1, 1, 1) * p + t.view(-1, 1, 1) - y)
    margin = SIGN_PIN * (s.abs() * p.flatten(1).abs().amax(1) + t.abs() + y.flatten(1).abs().amax(1))
    unpinned, pairs, worst = [], 0, float("inf")
    for step in STEPS:
        ds, ms = d[:, ::step, ::step], m[:, ::step, ::step]
        for axis in (1, 2):
            n = ds.shape[axis]
            if n < 2:
                continue
            lo, hi = ds.narrow(axis, 0, n - 1), ds.narrow(axis, 1, n - 1)
            valid = ms.narrow(axis, 0, n - 1) & ms.narrow(axis, 1, n - 1)
            ratio = (hi - lo).abs() / margin.view(-1, 1, 1)
            pairs += int(valid.sum())
            if bool(valid.any()):
                worst = min(worst, float(ratio[valid].min()))
            for b, i, j in (valid & (ratio < 1.0)).nonzero().tolist():
                unpinned.append((b, (i + (axis == 1)) * step, (j + (axis == 2)) * step))
    M = mf.sum((1, 2))
    a00, a01 = (mf * p * p).sum((1, 2)), (mf * p).sum((1, 2))
    two = M >= 2
    cond = ((a00 * M - a01 * a01) / (a00 * M))[two]
    return dict(pairs=pairs, unpinned=unpinned, min_gap_over_margin=worst, margin=margin, clamp_gap=float((raw - CLAMP).abs().min()),
                unpinned_pixels=int(((raw - CLAMP).abs() < CLAMP_PIN).sum()), clamped=int(clamped.sum()), unclamped=int((~clamped).sum()),
                cond=float(cond.min()) if bool(two.any()) else float("inf"), valid=M.long().tolist())


def pin_target(ins, c: Case, rounds: int = 40) -> int:
    """Nudges y_disp (in place) at one endpoint of every unpinned pair until none is left; returns the number of nudged pixels."""
    touched = set()
    for it in range(rounds):
        rep = pin_report(ins, c)
        if not rep["unpinned"]:
            return len(touched)
        for b, r, col in set(rep["unpinned"]):
            ins["y_disp"][b, r, col] += float((3 + 2 * it) * rep["margin"][b]) * (1.0 if (r + col + it) % 2 else -1.0)
            touched.add((b, r, col))
    raise AssertionError("the sign pins did not converge: choose another seed")


# ---------------- the cases ----------------
def _variant(ins, c: Case) -> None:
    inv, seg, y, m, ys, ms = (ins[k] for k in ("inv", "seg", "y_disp", "mask_disp", "y_seg", "mask_seg"))
    v = c.variant
    if v == "positive":
        inv.copy_(inv.abs() + 0.02)
    elif v == "negative":
        inv.copy_(-inv.abs() - 0.02)
    elif v == "col0":                                   # a 2 x 2 source: the left column non-positive, the right one positive
        inv[:, :, 0] = -inv[:, :, 0].abs() - 0.02
        inv[:, :, 1] = inv[:, :, 1].abs() + 0.05
    else:                                               # a patch of non-positive cells, two cells or two camera pixels wide: the clamp is hit at every ratio
        ph, pw = max(2, 2 * -(-c.h // c.H)), max(2, 2 * -(-c.w // c.W))
        inv[:, c.h // 3: c.h // 3 + ph, c.w // 2: c.w // 2 + pw] = -0.05
    if min(c.H, c.W) < 8:                               # tiny images: every pixel valid
        m.fill_(True)
        ms.fill_(True)
    if v == "mid_empty":
        m[1] = False
    elif v == "m3_zero":
        m &= (torch.arange(c.H) % 8 != 0).view(1, -1, 1)
    elif v in ("two_pixels", "one_pixel"):              # image 1 keeps its largest prediction (and the smallest unclamped one off its row and column)
        raw = upsample64(ins)[0][1]
        i1 = divmod(int(raw.argmax()), c.W)
        keep = [i1]
        if v == "two_pixels":
            cand = raw.clone()
            cand[raw < 1e-3] = float("inf")
            cand[i1[0], :] = float("inf")
            cand[:, i1[1]] = float("inf")
            keep.append(divmod(int(cand.argmin()), c.W))
        m[1] = False
        for r, col in keep:
            m[1, r, col] = True
    elif v == "seg_empty":
        ms.fill_(False)
    elif v == "class_off":
        ms[:, 1] = False
    elif v == "seg_sat":                                # exact 0 / 1 (the ScaledTanh head produces them), 1 - 2^-24 and 2^-30, each under target 0 and 1
        ny = nearest_index(c.H, c.h)
        for row, target in SAT_ROWS.items():
            seg[:, 0, row, :len(SAT_VALUES)] = torch.tensor(SAT_VALUES, dtype=torch.float32)
            ys[:, 0, ny == row, :] = target
            ms[:, 0, ny == row, :] = True


@functools.lru_cache(maxsize=None)
def build(name: str) -> Dict[str, torch.Tensor]:
    """The case's float32 inputs, pinned.  Shared: callers must not write to them."""
    c = CASES[name]
    keys = ("inv", "seg", "y_disp", "mask_disp", "y_seg", "mask_seg")
    ins = {k: t.clone() for k, t in zip(keys, loss_inputs(B=c.B, h=c.h, w=c.w, H=c.H, W=c.W, C=c.C, seed=c.seed))}
    _variant(ins, c)
    ins["nudged"] = pin_target(ins, c)
    return ins


# ---------------- the criterion, stated directly (and its planted faults) ----------------
def criterion(ins, c: Case, dtype=torch.float64, fault: str = "") -> Dict[str, torch.Tensor]:
    """The function oracle/loss_ref.training_loss states, with alpha, the empty seg selection (0, as the kernel documents) and scale / shift
    among the results.  fault: one of FAULTS, as the kernel would commit it."""
    B, H, W, h, w = c.B, c.H, c.W, c.h, c.w
    inv = ins["inv"].detach().to(dtype).clone().requires_grad_(True)
    seg = ins["seg"].detach().to(dtype).clone().requires_grad_(True)
    y, ys = ins["y_disp"].to(dtype), ins["y_seg"].to(dtype)
    m, ms = ins["mask_disp"].to(dtype), ins["mask_seg"]
    w_d, w_s = (c.w_s, c.w_d) if fault == "9" else (c.w_d, c.w_s)
    up = F.interpolate(inv.unsqueeze(1), size=(H, W), mode="bicubic", align_corners=(fault == "8"))[:, 0]
    floor = torch.full_like(up, CLAMP)
    p = torch.where(up < CLAMP, floor + (up - up.detach()) if fault == "5" else floor, up)
    if c.compute_ss:
        s, t = LR.compute_scale_and_shift(p, y, m)
        if fault == "4":
            s, t = s.detach(), t.detach()
    else:
        s, t = torch.ones(B, dtype=dtype), torch.zeros(B, dtype=dtype)
    ssi = s.view(-1, 1, 1) * p + t.view(-1, 1, 1)
    zero = torch.zeros((), dtype=dtype)
    M0 = m.sum()
    ld = (m * (ssi - y) ** 2).sum() / (2 * M0) if M0 > 0 else zero
    if c.alpha > 0:
        for step in STEPS:
            ms_k = m[:, ::step, ::step]
            Mk = M0 if fault == "3" else ms_k.sum()
            if Mk == 0:
                continue
            diff = ms_k * (ssi[:, ::step, ::step] - y[:, ::step, ::step])
            lower = diff[:, 1:, :].detach() if (fault == "2" and step == 8) else diff[:, 1:, :]
            gx = (diff[:, :, 1:] - diff[:, :, :-1]).abs() * (ms_k[:, :, 1:] * ms_k[:, :, :-1])
            gy = (lower - diff[:, :-1, :]).abs() * (ms_k[:, 1:, :] * ms_k[:, :-1, :])
            ld = ld + c.alpha * (gx.sum() + gy.sum()) / Mk
    iy, ix = nearest_index(H, h, fault == "6"), nearest_index(W, w, fault == "6")
    seg_up = seg[:, :, iy][:, :, :, ix]
    n = B * c.C * H * W if fault == "7" else int(ms.sum())
    ls = F.binary_cross_entropy(seg_up[ms], ys[ms], reduction="sum") / n if int(ms.sum()) > 0 else zero
    loss = w_d * ld + w_s * ls
    G = torch.autograd.grad(loss, up, retain_graph=True, allow_unused=True)[0] if loss.requires_grad else None
    G = torch.zeros_like(up) if G is None else G
    back = lambda g: torch.autograd.grad(up, inv, g, retain_graph=True)[0]
    d_inv = back(G)
    if fault in ("1r", "1c"):
        last = torch.zeros_like(G)
        d_inv = d_inv.clone()
        if fault == "1r":
            last[:, H - 1, :] = G[:, H - 1, :]
            d_inv[:, h - 1, :] -= back(last)[:, h - 1, :]
        else:
            last[:, :, W - 1] = G[:, :, W - 1]
            d_inv[:, :, w - 1] -= back(last)[:, :, w - 1]
    d_seg = torch.autograd.grad(loss, seg, allow_unused=True)[0] if loss.requires_grad else None
    d_seg = torch.zeros_like(seg) if d_seg is None else d_seg
    s, t = s.detach(), t.detach()
    if fault == "10":
        s, t = s.roll(1), t.roll(1)
    return dict(loss=loss.detach(), loss_disp=ld.detach(), loss_seg=ls.detach(), scale=s, shift=t, d_inv=d_inv.detach(), d_seg=d_seg.detach())


def oracle_applies(name: str) -> bool:
    return CASES[name].alpha == 0.5 and int(build(name)["mask_seg"].sum()) > 0


def oracle(name: str, dtype) -> Dict[str, torch.Tensor]:
    """oracle/loss_ref.loss_and_grads in `dtype`, plus the scale / shift it solves."""
    c, ins = CASES[name], build(name)
    cast = lambda t: t.to(dtype) if t.is_floating_point() else t
    args = [cast(ins[k]) for k in ("inv", "seg", "y_disp", "mask_disp", "y_seg", "mask_seg")]
    r = LR.loss_and_grads(*args, loss_depth_w=c.w_d, loss_seg_w=c.w_s, compute_ss=c.compute_ss)
    if c.compute_ss:
        p = LR.upsample_heads(args[0], args[1], c.H, c.W)[0]
        r["scale"], r["shift"] = LR.compute_scale_and_shift(p, args[2], args[3].to(dtype))
    else:
        r["scale"], r["shift"] = torch.ones(c.B, dtype=dtype), torch.zeros(c.B, dtype=dtype)
    return r


@functools.lru_cache(maxsize=None)
def evaluate(name: str, dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """float64: the reference; float32: the yardstick.  Shared: callers must not write to the tensors."""
    return oracle(name, dtype) if oracle_applies(name) else criterion(build(name), CASES[name], dtype)


def forced_solve_error(name: str) -> float:
    """The largest, over images and {scale, shift}, of |exact solve over torch's float32 up-sampling - ref64| / the yardstick's bound."""
    c, ins = CASES[name], build(name)
    if not c.compute_ss:
        return 0.0
    ref, yard = evaluate(name, torch.float64), evaluate(name, torch.float32)
    p32 = LR.upsample_heads(ins["inv"], ins["seg"], c.H, c.W)[0].double()
    solved = dict(zip(("scale", "shift"), LR.compute_scale_and_shift(p32, ins["y_disp"].double(), ins["mask_disp"].double())))
    worst = 0.0
    for k, v in solved.items():
        for b in range(c.B):
            r = float(ref[k][b])
            forced, bound = abs(float(v[b]) - r), max(F32_FACTOR * abs(float(yard[k][b]) - r), FLOOR * abs(r))
            worst = max(worst, forced / bound if bound > 0 else (0.0 if forced == 0 else float("inf")))
    return worst


# ---------------- slices and the bound ----------------
@functools.lru_cache(maxsize=None)
def slices(name: str) -> Dict[str, List[Tuple[str, torch.Tensor, bool]]]:
    """{output: [(label, bool mask of the output's shape, relative)]}; empty slices are left out."""
    c, ins = CASES[name], build(name)
    out: Dict[str, List[Tuple[str, torch.Tensor, bool]]] = {"d_inv": [], "d_seg": []}

    def add(key, label, mask, relative=False):
        if bool(mask.any()):
            out[key].append((label, mask, relative))

    clamped = upsample64(ins)[1].double()
    foot = torch.matmul(torch.matmul(cubic_membership(c.H, c.h).double().t(), clamped), cubic_membership(c.W, c.w).double()) > 0     # [B, h, w]
    rr, cc = torch.arange(c.h).view(-1, 1), torch.arange(c.w).view(1, -1)
    border = (rr < 2) | (rr >= c.h - 2) | (cc < 2) | (cc >= c.w - 2)
    for b in range(c.B):
        img = torch.zeros((c.B, c.h, c.w), dtype=torch.bool)
        img[b] = True
        add("d_inv", f"img{b}.border", img & border)
        add("d_inv", f"img{b}.interior", img & ~border)
        add("d_inv", f"img{b}.clampfoot", img & foot)
    ny, nx = F.one_hot(nearest_index(c.H, c.h), c.h).double(), F.one_hot(nearest_index(c.W, c.w), c.w).double()
    count = torch.matmul(torch.matmul(ny.t(), ins["mask_seg"].double()), nx)                                                        # [B, C, h, w]
    q = ins["seg"].double()
    sat = (q * (1 - q) < 2.0 ** -20) & (count > 0)          # 0, 1, 1 - 2^-24, 2^-30: gradients of 1e6 ... 1e12 times the others
    last = ((rr == c.h - 1) | (cc == c.w - 1)).expand(c.B, c.C, c.h, c.w)
    for b in range(c.B):
        for k in range(c.C):
            sel = torch.zeros((c.B, c.C, c.h, c.w), dtype=torch.bool)
            sel[b, k] = True
            add("d_seg", f"img{b}.class{k}.empty", sel & (count == 0))
            add("d_seg", f"img{b}.class{k}.last", sel & (count > 0) & last & ~sat)
            add("d_seg", f"img{b}.class{k}.rest", sel & (count > 0) & ~last & ~sat)
            add("d_seg", f"img{b}.class{k}.saturated", sel & sat, True)
    return out


class Row(NamedTuple):
    label: str
    err: float
    torch_err: float
    bound: float
    ok: bool


def _row(label, got, ref, yard, relative=False) -> Row:
    got, ref, yard = got.double().reshape(-1), ref.double().reshape(-1), yard.double().reshape(-1)
    if relative:                      # |kernel - ref| <= max(3 x max |torch - ref| / |ref|, 8 u) |ref| per element; a zero reference must be met exactly
        scale = ref.abs()
        safe = torch.where(scale > 0, scale, torch.ones_like(scale))
        torch_err = float(((yard - ref).abs() / safe).max())
        bound = max(F32_FACTOR * torch_err, FLOOR)
        excess = (got - ref).abs() - bound * scale
        err = float(((got - ref).abs() / safe).max())
        return Row(label, err, torch_err, bound, bool(torch.isfinite(got).all()) and bool((excess <= 0).all()))
    err, torch_err = float((got - ref).abs().max()), float((yard - ref).abs().max())
    bound = max(F32_FACTOR * torch_err, FLOOR * float(ref.abs().max()))
    return Row(label, err, torch_err, bound, err <= bound)           # a NaN fails


def compare(name: str, got: Dict[str, torch.Tensor]) -> List[Row]:
    """One Row per slice of d_inv and d_seg, per loss value and per image's scale and shift."""
    ref, yard = evaluate(name, torch.float64), evaluate(name, torch.float32)
    rows = []
    for key in ("d_inv", "d_seg"):
        for label, mask, relative in slices(name)[key]:
            rows.append(_row(f"{key}.{label}", got[key].cpu()[mask], ref[key][mask], yard[key][mask], relative))
    for key in ("loss", "loss_disp", "loss_seg"):
        rows.append(_row(key, got[key].cpu(), ref[key], yard[key]))
    for key in ("scale", "shift"):
        for b in range(CASES[name].B):
            rows.append(_row(f"{key}.img{b}", got[key].cpu()[b], ref[key][b], yard[key][b]))
    return rows


def worst(rows: List[Row]) -> Row:
    """The slice with the largest error / bound (a missed zero bound counts as infinite)."""
    ratio = lambda r: (r.err / r.bound) if r.bound > 0 else (0.0 if r.err == 0 else float("inf"))
    return max(rows, key=ratio)
