"""References, inputs, case tables and a-priori bounds for the fused Adam step (csrc/adam.hip through soccdpt_adam_step), one launch at a time.
tests/test_adam_refs.py shows on the CPU that the bounds admit float32 evaluations of the update (op by op like torch, and with the kernel's fmas) and refuse
named defects; tests/test_adam_gpu.py holds every element the kernel writes to them.

The contract (adam.hip's header and launcher): the scalar bookkeeping is done in float64 from the hyper-parameters as they arrive (doubles) and the step count,
and cast to float32 ONCE:
    one_minus_b1 = f32(1 - b1)   b2 = f32(b2)   one_minus_b2 = f32(1 - b2)   wd = f32(wd)   eps = f32(eps)
    step_size = f32(lr / (1 - b1^t))            inv_bc2_sqrt = f32(1 / sqrt(1 - b2^t))
`scalars` derives them here from (lr, betas, eps, wd, step); nothing is read from the library.  Per element, in exact arithmetic on those float32 scalars and
the float32 p, g, m, v (`ref_step`, float64):
    g' = g + wd p      m' = m + one_minus_b1 (g' - m)      v' = b2 v + one_minus_b2 g'^2
    p' = p - step_size * m' / (sqrt(v') inv_bc2_sqrt + eps)

The bounds (`ref_step` returns them beside the values).  u = 2^-24 is the unit roundoff of float32 (round to nearest), TINY = 2^-149 the spacing of the
subnormals (a result below 2^-126 carries an absolute error of up to TINY / 2 instead of a relative one; gfx950 keeps f32 subnormals).  An evaluation in float32
differs from the exact value by the roundings of its own operations and by what its operands' errors propagate to; both are accumulated term by term, on the
float64 values, for the union of the two evaluation orders that have to pass (the kernel's and torch's):

    E_g = u (|wd p| + |g'|)                      the product and the sum (the kernel's single fma rounds once: u |g'|); 0 when wd == 0: g' is g itself
    E_m = one_minus_b1 E_g                       propagated
        + LERP_ROUNDINGS u (|g' - m| + E_g)      d = g' - m, its product with the weight, and (torch.lerp's form for a weight >= 0.5) the weight's complement:
                                                 at most three roundings, each relative to at most |d|
        + u |m'| + 4 TINY                        the final sum
    E_v = one_minus_b2 (2 |g'| E_g + E_g^2)      propagated
        + u b2 v                                 b2 * v
        + 2 u one_minus_b2 g'^2                  (one_minus_b2 * g') * g' (the kernel's fma spares the second)
        + u v' + 4 TINY                          the final sum
    E_s = sqrt(v') - sqrt(v' - E_v)              the root of an operand off by E_v (the lower side is the larger one; sqrt(v' + E_v) where E_v >= v')
        + SQRT_U sqrt(v')                        the root itself: HIP documents sqrtf to 1 ulp = 2 u (it is correctly rounded by default, like torch's)
    E_den = E_s inv_bc2_sqrt
        + (u + SCALAR_FORM) sqrt(v') inv_bc2_sqrt   the product; SCALAR_FORM = 2 u admits torch's division by f32(sqrt(1 - b2^t)) in place of the multiplication
                                                 by f32(1 / sqrt(1 - b2^t)): the two scalars' reciprocals differ by at most 2 u relative
        + u den                                  the sum with eps (spared where the compiler contracts it into the product)
    E_q = (E_m + |q| E_den) / (den - E_den)      q = m' / den from operands off by E_m and E_den
        + DIV_U |q|                              the division: HIP documents 1 ulp = 2 u (correctly rounded by default)
    E_p = step_size E_q + u |step_size q|        the product
        + u |p'| + 4 TINY                        the final difference
Every E is then multiplied by SECOND_ORDER = 1 + 2^-16 for the products of two relative errors that the first-order terms above leave out (each is below
2^-22 of a first-order term).  No figure here was sized from what the kernel gives.

What the bounds can tell apart: they are a few u of each quantity, so a scalar formed in float32 from 0.999f (1.3e-5 relative in 1 - b2, the trap the
launcher's comment names) is outside E_v by two orders of magnitude after ONE step; the compounded comparison against torch in float32 cannot see it.  Every
step is checked on its own: step k's reference starts from the p, m, v the launch of step k - 1 wrote.

Values outside the bounds' regime are held separately (SPECIAL): g = 0 with m = v = 0 (nothing changes, bit for bit), g^2 underflowing to 0 (v' is exactly 0,
the denominator exactly eps; the general bound still holds there and is used), g^2 overflowing (v' = +inf, the update exactly 0, m' inside its bound).
`check_special` states these as exact properties of the result, not as a comparison with an emulation's bits (which of the two possible contractions the
compiler takes is not fixed): the GPU test checks the kernel's output against the properties, and the CPU test shows that every float32 emulation
(kernel-style with and without contraction, plain, torch's op chain) has them and that a v' that is merely tiny or merely large does not.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
LERP_ROUNDINGS = 3
SQRT_U = 2 * U
DIV_U = 2 * U
SCALAR_FORM = 2 * U
SECOND_ORDER = 1 + 2.0 ** -16

CHUNK = 48                    # tensors per launch (kAdamChunk)
BLOCK = 256
GRID_CAP = 512                # blocks per tensor: 131072 elements per trip of the grid-stride loop

Hyper = namedtuple("Hyper", "lr b1 b2 eps wd")
Scalars = namedtuple("Scalars", "omb1 b2 omb2 wd ss ibs eps")


def f32(x):
    """The float32 nearest to the Python float x, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float64).float())


def scalars(h, step):
    """The launcher's contract: float64 bookkeeping, one cast each."""
    bc1 = 1.0 - h.b1 ** step
    bc2 = 1.0 - h.b2 ** step
    return Scalars(f32(1.0 - h.b1), f32(h.b2), f32(1.0 - h.b2), f32(h.wd), f32(h.lr / bc1), f32(1.0 / math.sqrt(bc2)), f32(h.eps))


# ---------------- the float64 reference and its bounds ----------------
def ref_step(p, g, m, v, s):
    """float32 p, g, m, v and Scalars -> {"p" | "m" | "v": (float64 reference, float64 bound)}."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    wdp = s.wd * p
    g1 = g + wdp
    Eg = U * (wdp.abs() + g1.abs()) if s.wd != 0 else torch.zeros_like(g1)
    d = g1 - m
    m1 = m + s.omb1 * d
    Em = s.omb1 * Eg + LERP_ROUNDINGS * U * (d.abs() + Eg) + U * m1.abs() + 4 * TINY
    gg = g1 * g1
    v1 = s.b2 * v + s.omb2 * gg
    Ev = s.omb2 * (2 * g1.abs() * Eg + Eg * Eg) + U * s.b2 * v + 2 * U * s.omb2 * gg + U * v1 + 4 * TINY
    sq = v1.sqrt()
    Es = torch.where(v1 > Ev, Ev / (sq + (v1 - Ev).clamp(min=0).sqrt()), (v1 + Ev).sqrt()) + SQRT_U * sq
    den = sq * s.ibs + s.eps
    Eden = Es * s.ibs + (U + SCALAR_FORM) * sq * s.ibs + U * den
    assert bool((den - Eden > 0).all()), "the denominator's interval reaches 0: the bound does not cover this input"
    q = m1 / den
    Eq = (Em + q.abs() * Eden) / (den - Eden) + DIV_U * q.abs()
    upd = s.ss * q
    p1 = p - upd
    Ep = s.ss * Eq + U * upd.abs() + U * p1.abs() + 4 * TINY
    return {"p": (p1, Ep * SECOND_ORDER), "m": (m1, Em * SECOND_ORDER), "v": (v1, Ev * SECOND_ORDER)}


def check_step(got, inp, s, what):
    """got / inp: {"p" | "m" | "v" (| "g")} float32 -> {name: worst error / bound}; raises AssertionError where an element is outside its bound."""
    from tests.fused_refs import check_bound
    ref = ref_step(inp["p"], inp["g"], inp["m"], inp["v"], s)
    return {k: check_bound(got[k], ref[k][0], ref[k][1], f"{what} {k}") for k in ("p", "m", "v")}


def worst(got, inp, s):
    """{name: (error / bound, index, error, bound)} of the worst element, for the measured table."""
    ref = ref_step(inp["p"], inp["g"], inp["m"], inp["v"], s)
    out = {}
    for k in ("p", "m", "v"):
        err = (got[k].double() - ref[k][0]).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / ref[k][1])
        i = int(ratio.argmax()) if ratio.numel() else 0
        out[k] = (float(ratio[i]), i, float(err[i]), float(ref[k][1][i])) if ratio.numel() else (0.0, 0, 0.0, 0.0)
    return out


# ---------------- float32 evaluations, and the same with one defect each ----------------
def _fma(a, b, c):
    """fmaf on float32 tensors: the product is exact in float64; the sum is rounded to float64 and then to float32 (a double rounding can differ from fmaf's
    single one in the last bit once in ~2^29 elements, far inside what the bounds allow)."""
    return (a.double() * b.double() + c.double()).float()


ELEMENT_DEFECTS = ("bias correction with step - 1", "1 - b2 formed in float32 from 0.999f", "weight decay applied decoupled", "eps inside the root",
                   "eps added before the 1/sqrt(bc2) scaling")
TABLE_DEFECTS = ("grid-stride tail untouched", "tensor k uses tensor k - 1's length", "the second chunk reuses the first chunk's pointers")


def emulate(p, g, m, v, h, step, style="kernel", contract=True, defect=None):
    """One step in float32 -> {"p", "m", "v"}.  style "kernel": adam_kernel's expressions (its fmas; `contract` also fuses the two places the compiler may);
    "plain": the same expressions with every operation rounded on its own; "torch": _single_tensor_adam's chain of ATen ops."""
    assert defect is None or defect in ELEMENT_DEFECTS, defect
    t = lambda x: torch.tensor(x, dtype=torch.float32)
    bstep = step - 1 if defect == ELEMENT_DEFECTS[0] else step
    bc1 = 1.0 - h.b1 ** bstep
    bc2 = 1.0 - h.b2 ** bstep
    with_zero = lambda f: f() if bc1 != 0 and bc2 != 0 else float("inf")
    ss = t(with_zero(lambda: h.lr / bc1))
    ibs = t(with_zero(lambda: 1.0 / math.sqrt(bc2)))
    omb1, b2, eps, wd = t(1.0 - h.b1), t(h.b2), t(h.eps), t(h.wd)
    omb2 = (t(1.0) - t(h.b2)) if defect == ELEMENT_DEFECTS[1] else t(1.0 - h.b2)
    decoupled = defect == ELEMENT_DEFECTS[2]
    if decoupled:
        p = p * t(1.0 - h.lr * h.wd)
    if style == "kernel":
        g1 = _fma(wd, p, g) if (h.wd != 0 and not decoupled) else g
        m1 = _fma(omb1, g1 - m, m)
        v1 = _fma(omb2 * g1, g1, b2 * v)
        root = v1.sqrt()
    elif style == "plain":          # the kernel's expressions with no fused operation at all
        g1 = g + wd * p if (h.wd != 0 and not decoupled) else g
        m1 = m + omb1 * (g1 - m)
        v1 = b2 * v + (omb2 * g1) * g1
        root = v1.sqrt()
    else:
        g1 = g.add(p, alpha=h.wd) if (h.wd != 0 and not decoupled) else g
        m1 = torch.lerp(m, g1, 1.0 - h.b1)
        v1 = torch.addcmul(v * b2, g1, g1, value=float(omb2))
        root = v1.sqrt()
    if defect == ELEMENT_DEFECTS[3]:
        den = (v1 + eps).sqrt() * ibs
    elif defect == ELEMENT_DEFECTS[4]:
        den = (root + eps) * ibs
    elif style in ("kernel", "plain"):
        den = _fma(root, ibs, eps) if (contract and style == "kernel") else root * ibs + eps
    else:
        den = root / t(math.sqrt(bc2)) + eps if bc2 != 0 else root * ibs + eps
    if style in ("kernel", "plain"):
        q = m1 / den
        p1 = _fma(-ss, q, p) if (contract and style == "kernel") else p - ss * q
    else:
        p1 = torch.addcdiv(p, m1, den, value=-float(ss))
    return {"p": p1, "m": m1, "v": v1}


def emulate_launches(tensors, h, step, defect=None, **kw):
    """soccdpt_adam_step over a list of {"p", "g", "m", "v"}: the launcher's tables of CHUNK tensors (empty ones take no slot) and the kernel's grid-stride
    loop, with one of TABLE_DEFECTS -> list of {"p", "m", "v"}."""
    assert defect is None or defect in TABLE_DEFECTS, defect
    out = [{k: t[k].clone() for k in ("p", "m", "v")} for t in tensors]
    live = [i for i, t in enumerate(tensors) if t["p"].numel()]
    for base in range(0, len(live), CHUNK):
        chunk = live[base: base + CHUNK]
        nmax = max(tensors[i]["p"].numel() for i in chunk)
        threads = min((nmax + BLOCK - 1) // BLOCK, GRID_CAP) * BLOCK
        for k, i in enumerate(chunk):
            src = i
            if defect == TABLE_DEFECTS[2] and base > 0:
                src = live[k]                                   # table slot k of the first chunk
            n = tensors[src]["p"].numel()
            if defect == TABLE_DEFECTS[1] and k > 0:
                n = min(n, tensors[chunk[k - 1]]["p"].numel())      # a longer length would run past the end; the shorter one leaves a tail
            if defect == TABLE_DEFECTS[0]:
                n = min(n, threads)
            t = tensors[src]
            new = emulate(t["p"][:n], t["g"][:n], t["m"][:n], t["v"][:n], h, step, **kw)
            for key in ("p", "m", "v"):
                out[src][key][:n] = new[key]
    return out


# ---------------- inputs ----------------
def build(n, seed, step, gexp=(-18.0, 18.0)):
    """n elements: p ~ N(0, 1); |g| = 10^U(gexp) with a random sign, so that g^2 is finite and non-zero; at step 1 m = v = 0 as the optimiser has them, later
    m and v of g's own magnitude (m of either sign, so that g' - m both adds and cancels)."""
    gen = torch.Generator().manual_seed(1000 * seed + 17)
    r = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    mag = 10.0 ** (gexp[0] + (gexp[1] - gexp[0]) * r())
    g = mag * torch.where(r() < 0.5, -1.0, 1.0)
    if step == 1:
        m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    else:
        m = mag * (2 * r() - 1)
        v = mag * mag * (0.25 + 3.75 * r())
    return {"p": p.float(), "g": g.float(), "m": m.float(), "v": v.float()}


def cat(tensors, key):
    return torch.cat([t[key].reshape(-1) for t in tensors]) if tensors else torch.zeros(0)


def cat_all(tensors, keys=("p", "g", "m", "v")):
    return {k: cat(tensors, k) for k in keys}


# ---------------- the case tables ----------------
DEFAULT = Hyper(1e-3, 0.9, 0.999, 1e-8, 1e-2)
BETAS_EPS = [(0.9, 0.999, 1e-8), (0.0, 0.999, 1e-8), (0.9, 0.0, 1e-3), (0.5, 0.9, 1e-8)]
HYPERS = [Hyper(lr, b1, b2, eps, wd) for (b1, b2, eps) in BETAS_EPS for lr in (1e-3, 1.0) for wd in (0.0, 1e-2)]
STEPS = [1, 1000, 100000]                 # each followed by the next one (2, 1001, 100001) from what the first launch wrote
HYPER_N = 1001

SIZES = [1, 255, 256, 257, GRID_CAP * BLOCK, GRID_CAP * BLOCK + 1, 256 * 256 * 9]          # ... 131072, 131073 (the cap and one past it), 589824
MIXED_CHUNK = [GRID_CAP * BLOCK + 1, 1, 300, 70000, 0, 257, 2 * GRID_CAP * BLOCK + 5]      # one launch: blocks beyond a short tensor's end idle; an empty one
COUNTS = [0, 1, 48, 49, 96, 97]
COUNT_SIZES = [1, 300, 17, 257, 600, 64, 1000, 255]                                        # cycled; neighbours always differ in length


def count_case(n_tensors, step=2, seed=50):
    return [build(COUNT_SIZES[i % len(COUNT_SIZES)], seed + i, step) for i in range(n_tensors)]


# g = 0 on zero state; g^2 below the smallest subnormal (1e-30^2 * 1e-3) on zero v; g^2 above FLT_MAX
SPECIAL_N = 300


def special(kind):
    t = build(SPECIAL_N, 77, 1)
    sign = torch.where(torch.arange(SPECIAL_N) % 2 == 0, 1.0, -1.0)
    if kind == "zero":
        t["g"] = torch.zeros(SPECIAL_N) * sign                 # +0 and -0
    elif kind == "underflow":
        t["g"] = (1e-30 * sign).float()
    elif kind == "overflow":
        t["g"] = (1e30 * sign).float()
        t["m"] = (1e29 * sign.flip(0)).float()
        t["v"] = torch.full((SPECIAL_N,), 1e30)
    else:
        raise KeyError(kind)
    return t


SPECIAL = ("zero", "underflow", "overflow")
SPECIAL_HYPER = Hyper(1e-3, 0.9, 0.999, 1e-8, 0.0)          # wd 0: g' is g


def check_special(kind, got, inp, s):
    """The exact properties of each special regime, and the bounds where they apply."""
    bits = lambda x: x.contiguous().view(torch.int32)
    if kind == "zero":
        assert torch.equal(bits(got["p"]), bits(inp["p"])), "g = 0 on zero state: p changed"
        assert bool((got["m"] == 0).all()) and bool((got["v"] == 0).all())
    elif kind == "underflow":
        assert bool((bits(got["v"]) == 0).all()), "g^2 underflows: v' must be +0"
        check_step(got, inp, s, "underflow")
        # the denominator is eps itself: p' = p - step_size * (m' / eps), whatever the compiler fused, to the roundings of q, the product and the difference
        q = got["m"].double() / s.eps
        ref = inp["p"].double() - s.ss * q
        assert bool(((got["p"].double() - ref).abs() <= (DIV_U + U) * (s.ss * q).abs() + U * ref.abs() + 4 * TINY).all())
    else:
        assert bool((got["v"] == float("inf")).all()), "g^2 overflows: v' must be +inf"
        assert torch.equal(bits(got["p"]), bits(inp["p"])), "v' = inf: the update must be exactly 0"
        from tests.fused_refs import check_bound
        ref = ref_step(inp["p"], inp["g"], inp["m"], inp["v"], s)
        check_bound(got["m"], *ref["m"], "overflow m")
