"""References, inputs, case tables and a-priori bounds for the evaluation-metric kernels (csrc/metrics.hip through soccdpt_metrics_depth and
soccdpt_metrics_iou).  tests/test_metrics_refs.py shows on the CPU that the bounds admit float32 emulations of the kernels' arithmetic (with and without
contraction) and refuse named defects; tests/test_metrics_kernels_gpu.py holds the kernels to them.

The depth check is split the way the training tests pin masks, so that neither half inherits the other's conditioning:

(a) Scale and shift, out[7 + 2b], out[8 + 2b].  The kernel's contract: per image five sums over the pixels whose mask byte is non-zero,
        s0 = sum f32(p p)   s1 = sum p   s2 = sum 1   s3 = sum f32(p t)   s4 = sum t,
    accumulated in float64 (per thread, per block, one atomic per block: the order varies, the result to ~npix 2^-53 relative), each cast to float32 ONCE, and
    the 2x2 system solved in float32 like the reference:  det = a00 a11 - a01^2;  det == 0 -> (0, 0), else
        scale = (a11 b0 - a01 b1) / det      shift = (-a01 b0 + a00 b1) / det.
    `ref_scale_shift` forms the five float64 sums of the float32-rounded products, casts them, and evaluates the solve on those float32 values in float64.
    With u = 2^-24 (unit roundoff), each two-product difference x y - z w evaluated in float32 is off by at most
        E(x y - z w) = (u + 2 CAST) (|x y| + |z w|) + u |x y - z w|
    -- one rounding per product (a contraction spares one of them) and one for the difference, plus CAST = 2 u per factor for the case that the device's
    float64 sum lies on the other side of a float32 rounding boundary than ours (one ulp = 2 u of that factor) -- and the quotient by
        E(n / d) = (E_n + |n / d| E_d) / (|d| - E_d) + u |n / d|          (IEEE division: hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
    This IS the conditioning of det: E_det / |det| grows as the variance of p under the mask vanishes against its mean square.  The inputs keep
    E_det / |det| below 1e-4 (checked on the CPU), except the images whose det is exactly 0 by construction (an empty mask; one masked pixel, where
    a00 a11 = f32(p p) and a01^2 rounds to the same float32): there scale and shift must be exactly 0.  A NaN under the mask gives NaN for both.

(b) The seven metrics, out[0..6], from the scale and shift THE LAUNCH RETURNED (so (a)'s conditioning does not enter).  Per masked pixel, in float64 from the
    float32 p, g and the returned float32 scale, shift:  q = scale p + shift, d = g - q, and the terms |d| / g, d^2 / g, d^2, (ln g - ln q)^2 and
    r = max(g / q, q / g).  Their float32 evaluation errors, term by term:
        E_q  = u (|scale p| + |q|)        the product and the sum; 0 where both the fused and the unfused float32 evaluation are exact
        E_d  = E_q + u |d|
        E_dd = 2 |d| E_d + E_d^2 + u d^2
        abs_rel term: E_d / |g| + u |d / g|              sq_rel term: E_dd / |g| + u d^2 / |g|              rmse term: E_dd
        E_l  = LOG_U (|ln g| + |ln q|) + E_q / (|q| - E_q) + u |l|,  l = ln g - ln q;  LOG_U = 6 u: logf to 3 ulp, the weaker of the two published
               figures (HIP's math table says 1 ulp, the OpenCL C profile the device library is built to says 3)
        rmse_log term: 2 |l| E_l + E_l^2 + u l^2
    The terms are added in float64 (ACC = npix 2^-52 of the sum of magnitudes, generous), divided by the masked count, rooted for rmse / rmse_log in float64
    (the root's sensitivity: E / (sqrt(x) + sqrt(x - E))) and cast to float32 once (u).  A sum that is not finite gives exactly 0, like the reference's NaN /
    inf -> 0.
    a1, a2, a3 are counts: a pixel whose float64 ratio r is within E_r = max(E(g / q), E(q / g)) of 1.25, 1.25^2 or 1.25^3 is undecided; the kernel's count
    must lie between the decided hits and the decided hits plus the undecided ones.  Where E_q is 0 both quotients are single IEEE divisions of exact
    operands, so the float32 ratio is known exactly and every such pixel is decided (the EXACT case below pins `<` against `<=` with it).  At most 1 in 1000
    masked pixels of a case may be undecided (checked on the CPU for the committed inputs).  A NaN ratio is a decided miss.

IoU: the counts are integers, so out[b] is one fixed float32 expression, sum over c of f32(inter) / (f32(union) + 1e-7f), in order, divided by f32(C):
compared bitwise (`ref_iou`).

Masked-out pixels: the kernels test the mask byte and never read a masked-out value into a sum.  The reference multiplies by the mask, so a NaN or inf
outside the mask poisons ITS sums.  That divergence is deliberate (metrics.hip's header); the POISON variant of every case must give the same bits.
"""
from collections import namedtuple

import torch

U = 2.0 ** -24
CAST = 2 * U
LOG_U = 6 * U
ACC = 2.0 ** -52
MAX_DET_ERROR = 1e-4
MAX_UNDECIDED = 1e-3
THRESHOLDS = (1.25, 1.5625, 1.953125)          # exact in float32
BLOCK = 256
PER_THREAD = 8
GRID_CAP = 512
MAX_B = 256

f32 = lambda x: x.float().double()


def _fma(a, b, c):
    """fmaf on float32 tensors (the product is exact in float64; see adam_refs._fma)."""
    return (a.double() * b.double() + c.double()).float()


# ---------------- (a) scale and shift ----------------
def masked_sums(pred, gt, mask):
    """[B, 5] float64 sums of the float32-rounded products over the pixels whose mask byte is non-zero."""
    m = (mask != 0)
    z = lambda t: torch.where(m, t.double(), torch.zeros((), dtype=torch.float64)).flatten(1).sum(1)
    return torch.stack([z(pred * pred), z(pred), m.flatten(1).sum(1).double(), z(pred * gt), z(gt)], 1)


def _diff_of_products(x, y, z, w):
    v = x * y - z * w
    return v, (U + 2 * CAST) * ((x * y).abs() + (z * w).abs()) + U * v.abs()


def ref_scale_shift(pred, gt, mask):
    """-> (scale, shift, E_scale, E_shift, det, E_det) float64 [B]; where det == 0 the expectation is exactly (0, 0), where it is NaN, NaN."""
    a00, a01, a11, b0, b1 = f32(masked_sums(pred, gt, mask)).unbind(1)
    det, Edet = _diff_of_products(a00, a11, a01, a01)
    n0, En0 = _diff_of_products(a11, b0, a01, b1)
    n1, En1 = _diff_of_products(a00, b1, a01, b0)
    # "exactly 0" is decided where the kernel decides it, in float32: solve_lsq writes det as fmaf(a00, a11, -__fmul_rn(a01, a01)), the second product
    # rounded on its own.  For one masked pixel (a00 = rn(p p), a11 = 1, a01 = p) that is the same 0 as the unfused rn(a00 a11) - rn(a01 a01) evaluated
    # here.  An fma over the SECOND product, fma(-a01, a01, a00 a11), would leave rn(p p) - p p != 0 and break this case; the kernel's explicit
    # operations rule it out whatever the compiler's contraction setting.
    a32 = [v.float() for v in (a00, a01, a11)]
    zero = (a32[0] * a32[2] - a32[1] * a32[1]) == 0
    safe = torch.where(zero, torch.ones_like(det), det)
    out = []
    for n, En in ((n0, En0), (n1, En1)):
        x = n / safe
        E = (En + x.abs() * Edet) / (safe.abs() - Edet) + U * x.abs()
        out.append((torch.where(zero, torch.zeros_like(x), x), torch.where(zero, torch.zeros_like(E), E)))
    return out[0][0], out[1][0], out[0][1], out[1][1], torch.where(zero, torch.zeros_like(det), det), Edet


def check_scale_shift(out, pred, gt, mask, what):
    """out: the launch's float32 [7 + 2B].  -> worst error / bound."""
    B = pred.shape[0]
    scale, shift, Es, Et, det, Edet = ref_scale_shift(pred, gt, mask)
    worst = 0.0
    for name, got, ref, E in (("scale", out[7::2], scale, Es), ("shift", out[8::2], shift, Et)):
        got = got.double()
        for b in range(B):
            g, r, e, d = float(got[b]), float(ref[b]), float(E[b]), float(det[b])
            if d != d:
                assert g != g, f"{what}: {name}[{b}] is {g}, a NaN under the mask must give NaN"
            elif d == 0:
                assert g == 0, f"{what}: {name}[{b}] is {g}; det is exactly 0, it must be 0"
            else:
                assert float(Edet[b]) <= MAX_DET_ERROR * abs(d), f"{what}: image {b} is too close to cancellation for the bound (E_det / |det| = {float(Edet[b]) / abs(d):.2e})"
                assert abs(g - r) <= e, f"{what}: {name}[{b}] = {g!r}, expected {r!r}, bound {e:.3e} (error {abs(g - r):.3e})"
                worst = max(worst, abs(g - r) / e)
    return worst


# ---------------- (b) the seven metrics from the returned scale and shift ----------------
Terms = namedtuple("Terms", "ref bound lo hi undecided n")


def ref_metrics(scale, shift, pred, gt, mask):
    """scale, shift: float32 [B] as the launch returned them -> Terms: ref, bound float64 [4] for abs_rel, sq_rel, rmse, rmse_log (bound 0 and ref 0 where the
    float64 sum is not finite), lo / hi float32 [3] for a1..a3, the undecided fraction [3], the masked count."""
    B = pred.shape[0]
    m = (mask != 0)
    pred, gt, m = pred.flatten(1), gt.flatten(1), m.flatten(1)
    s, t = scale.reshape(B, 1).float(), shift.reshape(B, 1).float()
    p32, g32 = pred.float(), gt.float()
    sp = s.double() * p32.double()
    q = (sp + t.double())[m]
    q_unfused, q_fused = (s * p32 + t)[m], _fma(s.expand_as(p32), p32, t.expand_as(p32))[m]
    exact_q = (q_unfused.double() == q) & (q_fused.double() == q)
    Eq = torch.where(exact_q, torch.zeros_like(q), U * (sp[m].abs() + q.abs()))
    g = g32.double()[m]
    n = int(m.sum())
    d = g - q
    Ed = Eq + U * d.abs()
    dd = d * d
    Edd = 2 * d.abs() * Ed + Ed * Ed + U * dd
    lg, lq = g.log(), q.log()
    l = lg - lq
    El = LOG_U * (lg.abs() + lq.abs()) + Eq / (q.abs() - Eq) + U * l.abs()
    terms = [(d.abs() / g, Ed / g.abs() + U * (d / g).abs(), False), (dd / g, Edd / g.abs() + U * dd / g.abs(), False), (dd, Edd, True),
             (l * l, 2 * l.abs() * El + El * El + U * l * l, True)]
    ref, bound = [], []
    for v, E, root in terms:
        x = v.sum() / n if n else torch.tensor(float("nan"), dtype=torch.float64)
        Ex = (E.sum() + ACC * n * v.abs().sum()) / n if n else torch.tensor(0.0, dtype=torch.float64)
        if root:
            Ex = Ex / (x.sqrt() + (x - Ex).clamp(min=0).sqrt()) if float(x) > 0 else Ex.sqrt()
            x = x.sqrt()
        if not bool(torch.isfinite(x)):
            x, Ex = torch.zeros((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
        ref.append(x)
        bound.append(Ex + U * x.abs())
    # the ratios: where q is exact in float32 the kernel's ratio is the maximum of two IEEE quotients of exact operands
    r = torch.maximum(g / q, q / g)
    Er = torch.maximum(g.abs() * Eq / (q.abs() * (q.abs() - Eq)) + U * (g / q).abs(), Eq / g.abs() + U * (q / g).abs())
    Er = torch.where(torch.isfinite(Er) & (q.abs() > Eq), Er, torch.full_like(Er, float("inf")))
    # g == 0 under the mask: g / q is a zero and q / g an infinity of q's sign, exactly, as long as that sign is certain
    Er = torch.where((g == 0) & (q.abs() > Eq), torch.zeros_like(Er), Er)
    q32, gm32 = q_unfused, g32[m]
    r32 = torch.where((gm32 / q32 != gm32 / q32) | (q32 / gm32 != q32 / gm32), torch.full_like(q32, float("nan")), torch.maximum(gm32 / q32, q32 / gm32)).double()
    r = torch.where(exact_q, r32, r)
    Er = torch.where(exact_q, torch.zeros_like(Er), Er)
    nan = r != r
    lo, hi, und = [], [], []
    for T in THRESHOLDS:
        hit = ~nan & (r + Er < T)
        miss = nan | (r - Er >= T)
        u_ = ~hit & ~miss
        lo.append(float(torch.tensor(int(hit.sum()) / n if n else 0.0, dtype=torch.float64).float()))
        hi.append(float(torch.tensor((int(hit.sum()) + int(u_.sum())) / n if n else 0.0, dtype=torch.float64).float()))
        und.append(int(u_.sum()) / n if n else 0.0)
    return Terms(torch.stack(ref), torch.stack(bound), lo, hi, und, n)


def check_metrics(out, pred, gt, mask, what):
    """The seven metrics of a launch's out against the float64 terms from the scale and shift in the same out.  -> worst error / bound."""
    T = ref_metrics(out[7::2], out[8::2], pred, gt, mask)
    worst = 0.0
    names = ("abs_rel", "sq_rel", "rmse", "rmse_log")
    for k in range(4):
        g, r, e = float(out[k]), float(T.ref[k]), float(T.bound[k])
        assert abs(g - r) <= e, f"{what}: {names[k]} = {g!r}, expected {r!r}, bound {e:.3e} (error {abs(g - r):.3e})"
        if e > 0:
            worst = max(worst, abs(g - r) / e)
    for k in range(3):
        assert max(T.undecided) <= MAX_UNDECIDED, f"{what}: {T.undecided} of the masked pixels are undecided"
        assert T.lo[k] <= float(out[4 + k]) <= T.hi[k], f"{what}: a{k + 1} = {float(out[4 + k])!r}, expected within [{T.lo[k]!r}, {T.hi[k]!r}]"
    return worst


def check_depth(out, pred, gt, mask, what):
    return check_scale_shift(out, pred, gt, mask, what), check_metrics(out, pred, gt, mask, what)


# ---------------- IoU ----------------
def ref_iou(pred, gt, defect=None):
    """pred, gt float32 [B, C, npix] -> float32 [B], the kernels' expression."""
    assert defect is None or defect in IOU_DEFECTS, defect
    B, C = pred.shape[:2]
    pm, tm = (pred >= 0.5, gt >= 0.5) if defect == IOU_DEFECTS[0] else (pred > 0.5, gt > 0.5)
    inter = (pm & tm).flatten(2).sum(2)
    uni = pm.flatten(2).sum(2) + tm.flatten(2).sum(2) if defect == IOU_DEFECTS[1] else (pm | tm).flatten(2).sum(2)
    iou = torch.zeros(B, dtype=torch.float32)
    for c in range(C):
        iou = iou + inter[:, c].float() / (uni[:, c].float() + torch.tensor(1e-7, dtype=torch.float32))
    return iou / torch.tensor(float(B if defect == IOU_DEFECTS[2] else C), dtype=torch.float32)


IOU_DEFECTS = ("IoU with >=", "union counted as p + t", "class mean divided by B")


# ---------------- float32 emulation of the depth kernels, and the same with one defect ----------------
DEPTH_DEFECTS = ("mask ignored", "image 0's mask used for all images", "image 0's scale used for all images", "<= at an accuracy threshold",
                 "rmse without the root", "mean over all pixels instead of masked ones", "grid-stride tail dropped")


def _solve(sums, contract):
    a00, a01, a11, b0, b1 = sums.float().unbind(1)
    if contract:
        sub = lambda x, y, z, w: _fma(x, y, -(z * w))
    else:
        sub = lambda x, y, z, w: x * y - z * w
    det = sub(a00, a11, a01, a01)
    n0, n1 = sub(a11, b0, a01, b1), sub(a00, b1, a01, b0)
    ok = det != 0
    one = torch.ones_like(det)
    return torch.where(ok, n0 / torch.where(ok, det, one), torch.zeros_like(det)), torch.where(ok, n1 / torch.where(ok, det, one), torch.zeros_like(det))


def emulate_depth(pred, gt, mask, contract=False, defect=None):
    """lsq_sums_kernel, masked_err_kernel and depth_finalize_kernel in float32 / float64 as the kernels have them -> float32 [7 + 2B]."""
    assert defect is None or defect in DEPTH_DEFECTS, defect
    B = pred.shape[0]
    pred, gt = pred.float().flatten(1), gt.float().flatten(1)
    m = (mask != 0).flatten(1)
    npix = pred.shape[1]
    if defect == DEPTH_DEFECTS[0]:
        m = torch.ones_like(m)
    if defect == DEPTH_DEFECTS[1]:
        m = m[:1].expand_as(m)
    if defect == DEPTH_DEFECTS[6]:
        m = m.clone()
        m[:, min((npix + BLOCK * PER_THREAD - 1) // (BLOCK * PER_THREAD), GRID_CAP) * BLOCK:] = False
    scale, shift = _solve(masked_sums(pred, gt, m), contract)
    s, t = scale.view(B, 1), shift.view(B, 1)
    if defect == DEPTH_DEFECTS[2]:
        s, t = s[:1].expand(B, 1), t[:1].expand(B, 1)
    q = _fma(s.expand_as(pred), pred, t.expand_as(pred)) if contract else s * pred + t
    d = gt - q
    # torch.maximum propagates a NaN where fmaxf drops it; g / q is NaN exactly where q / g is (0 / 0, inf / inf, a NaN operand), so the two agree
    thr = torch.maximum(gt / q, q / gt)
    lg = gt.log() - q.log()
    S = lambda v: v.double()[m].sum()
    n = float(m.sum())
    cmp = (lambda a, b: a <= b) if defect == DEPTH_DEFECTS[3] else (lambda a, b: a < b)
    acc = [S(d.abs() / gt), S(d * d / gt), S(d * d), S(lg * lg)] + [S(cmp(thr, T).float()) for T in THRESHOLDS]
    if defect == DEPTH_DEFECTS[5]:
        n = float(m.numel())
    with_n = lambda x: x / n if n else torch.tensor(float("nan"), dtype=torch.float64)
    v = [with_n(acc[0]), with_n(acc[1]), with_n(acc[2]) if defect == DEPTH_DEFECTS[4] else with_n(acc[2]).sqrt(), with_n(acc[3]).sqrt()] + [with_n(a) for a in acc[4:]]
    v = [x if bool(torch.isfinite(x)) else torch.zeros((), dtype=torch.float64) for x in v]
    out = torch.empty(7 + 2 * B, dtype=torch.float32)
    out[:7] = torch.stack(v).float()
    out[7::2], out[8::2] = scale, shift
    return out


# ---------------- inputs ----------------
def healthy(B, npix, seed, keep=0.7):
    """p ~ U(0.2, 3): variance / mean square ~ 0.25, det far from cancellation; g = (0.7 p + 0.3) e^(0.3 N) > 0: about half of the ratios inside 1.25;
    each image with its own scale so that a scale taken from another image shows."""
    gen = torch.Generator().manual_seed(7000 + seed)
    p = 0.2 + 2.8 * torch.rand(B, npix, generator=gen, dtype=torch.float64)
    k = 0.5 + torch.arange(B, dtype=torch.float64).view(B, 1) % 7 * 0.25
    g = (k * p + 0.3) * torch.exp(0.3 * torch.randn(B, npix, generator=gen, dtype=torch.float64))
    mask = (torch.rand(B, npix, generator=gen) < keep).to(torch.uint8)
    mask[:, :2] = 1          # at least two masked pixels with distinct p per image: det != 0 unless a case asks otherwise (npix 1: det is exactly 0)
    return p.float(), g.float(), mask


def exact_case():
    """Small integers: every product and sum is exact in float32, the residuals are orthogonal to (p, 1) so the fit is scale 1, shift 0 EXACTLY, and the ratios
    sit exactly on the thresholds: (p, 1.25 p) with (p, 0.75 p), (p, 1.5625 p) with (p, 0.4375 p), (p, 1.953125 p) with (p, 0.046875 p).  A ratio equal to a
    threshold is a miss (`<`)."""
    p, g = [], []
    for base, up, down in ((4, 1.25, 0.75), (16, 1.5625, 0.4375), (64, 1.953125, 0.046875)):
        for k in (1, 2, 3):
            p += [base * k, base * k]
            g += [base * k * up, base * k * down]
    p += [5.0, 7.0, 100.0]          # masked out
    g += [5.0, 7.0, 100.0]
    mask = torch.ones(len(p), dtype=torch.uint8)
    mask[-3:] = 0
    return torch.tensor([p], dtype=torch.float32), torch.tensor([g], dtype=torch.float32), mask.view(1, -1)


def depth_case(name):
    """-> (pred [B, npix], gt, mask uint8)."""
    if name.startswith("npix "):
        return healthy(1, int(name[5:]), 1)
    if name.startswith("B "):
        return healthy(int(name[2:]), 37, 2)
    if name == "exact thresholds":
        return exact_case()
    if name == "empty and single":          # image 1: empty mask; image 2: exactly one masked pixel (det exactly 0 -> aligned prediction 0, shared sums)
        p, g, m = healthy(4, 300, 3)
        m[1] = 0
        m[2] = 0
        m[2, 123] = 1
        return p, g, m
    if name == "all empty":
        p, g, m = healthy(3, 300, 4)
        return p, g, torch.zeros_like(m)
    if name == "non-positive gt":
        p, g, m = healthy(2, 300, 5)
        g[0, 0], g[0, 1], g[1, 7] = 0.0, -1.5, -0.0
        return p, g, m
    if name == "negative aligned":          # outliers drag the fit: several aligned predictions fall below 0
        p, g, m = healthy(2, 300, 6)
        g = (3.0 - p.double() * 1.2).abs().float() + 0.05
        p[:, :40] = p[:, :40] * 4
        m[:, :40] = 1
        return p, g, m
    if name == "mask bytes":
        p, g, m = healthy(2, 300, 7)
        m = m * torch.tensor([1, 2, 255, 128], dtype=torch.uint8).repeat(75).view(1, 300)
        return p, g, m
    if name == "nan under the mask":
        p, g, m = healthy(1, 300, 8)
        p[0, 0] = float("nan")
        return p, g, m
    raise KeyError(name)


DEPTH_NPIX = [1, 63, 255, 256, 257, 2049, GRID_CAP * BLOCK * PER_THREAD + 1]
DEPTH_B = [1, 2, 65, MAX_B]
DEPTH_CASES = [f"npix {n}" for n in DEPTH_NPIX] + [f"B {b}" for b in DEPTH_B] + ["exact thresholds", "empty and single", "all empty", "non-positive gt",
                                                                              "negative aligned", "mask bytes", "nan under the mask"]


def poison(pred, gt, mask):
    """NaN and +-inf at every masked-out pixel of both operands."""
    out = (mask == 0)
    vals = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(pred.numel() // 3 + 1)[: pred.numel()].view(pred.shape)
    return torch.where(out, vals, pred), torch.where(out, vals.flip(-1), gt)


IOU_CASES = {"npix 1": (3, 1, 1), "npix 257 C 4": (2, 4, 257), "B 65": (65, 4, 70), "B 300": (300, 1, 70), "npix 2049": (1, 3, 2049)}


def iou_case(name):
    """-> pred, gt float32 [B, C, npix]: values around 0.5 with exactly 0.5, the next float above it, NaN and +-inf among them; the last image's class 0 has an
    empty union."""
    B, C, npix = IOU_CASES[name]
    gen = torch.Generator().manual_seed(8000 + B * 7 + C)
    special = torch.tensor([0.5, 0.5 + 2.0 ** -24, float("nan"), float("inf"), float("-inf"), 0.5 - 2.0 ** -25, 1.0, 0.0])
    pick = lambda: torch.where(torch.rand(B, C, npix, generator=gen) < 0.4, special[torch.randint(0, 8, (B, C, npix), generator=gen)],
                               torch.rand(B, C, npix, generator=gen))
    p, t = pick(), pick()
    p[-1, 0], t[-1, 0] = 0.25, 0.5
    return p, t
