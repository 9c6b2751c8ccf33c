"""Float64 reference for csrc/kd_loss_region.hip (kd_seg_region_loss_fwd_bwd): the hard-label loss wf * Focal + wt * Tversky of
DESIGN.md section 3 with the KL term of the segmentation loss riding along, its values and dL/dlogits in closed form, and the
rounding-error bound each kernel output must meet, in the conventions of tests/_fp64_loss_ref.py:

    err = C_BOUND * n_seq * U * sum |t_i|

Every function evaluates in the inputs' dtype (float64: the reference; float32: the self-check of
tests/test_fp64_region_loss_ref_host.py that a plain fp32 evaluation of the same formulas meets the same bound), scalars enter
as the fp32 values the C ABI receives (`spec`, `f32`).  The softmax, its bounds (`_softmax`: an absolute bound of log p, a
relative bound of p), the KL value and the KL part of the gradient are those of _fp64_loss_ref.seg_loss, called with every
label ignored.  Reductions take n_seq from `seg_layout` (iterations per thread + 6 wave steps + 4 waves); the kernel sums the
slab and forms everything after it (the quotients, the Tversky indices, the gradient coefficients) in double, so the terms
counted below for those steps are what the fp32 self-check needs, not the kernel.

What does not take the plain form:
  * the focal factor (1 - p_y)^gamma multiplies log p_y, whose float64 value is itself wrong in RELATIVE terms when p_y -> 1
    (log of a sum that rounds to 1): the product is bounded through the absolute bound of log p_y times the factor, which
    vanishes with (1 - p_y)^gamma; 1 - p_y is the sum of the other classes' probabilities, so its bound is relative;
  * a non-integer gamma goes through powf, bounded as exp(e * log(x)): a relative error of 3 operations on e * |log x| + 1;
  * a quotient x / y of two bounded values is bounded to first order: e_x / y + |x / y| * e_y / y;
  * the Tversky denominator D = (1 - a - b) TP + a A + b N + s is linear in the two fp32 sums TP and A, so their bounds enter
    with |1 - a - b| and a; the count N is an exact integer (below 2^24 per class at every size used)."""
import collections

import torch

import _fp64_loss_ref as L
from _fp64_loss_ref import TINY, _bound, _softmax, f32, seg_layout, seg_n_seq  # noqa: F401  (re-exported for the tests)

DEFAULTS = dict(gamma=2.0, wf=1.0, wt=1.0, a=0.7, b=0.3, s=1.0)
KEYS = ("gamma", "wf", "wt", "a", "b", "s")


def spec(**kw):
    """the six parameters as the fp32 values the kernel receives"""
    d = dict(DEFAULTS)
    d.update(kw)
    return {k: f32(d[k]) for k in KEYS}


def _pow(x, e):
    """x^e for x in [0, 1] as the kernel forms it -> (value, relative bound of the operation itself)"""
    if e == 0:
        return torch.ones_like(x), 0.0
    if e == 1:
        return x, 0.0
    if e == 2:
        return x * x, _bound(1, 1.0)
    return x ** e, _bound(3, e * torch.log(x.clamp_min(TINY)).abs() + 1)


def region_loss(zs, zt, target, cw, ignore_index, T, alpha, gs, n_seq, sp, want_grad=True, mutate=None):
    """zs, zt [B, NC, HW] (zt None: no KL), target int64 [B, HW], cw [NC] or None, sp = spec(...), gs = gscale * gscale_dev[0].
    -> {"vals": (v, err)} with v = (L_hard, KL, sum w, Focal, Tversky, TI_0 .. TI_{NC-1}) and, with want_grad,
    {"dzs": (g, err)}, g = gs * d(L_hard + alpha*T^2*KL)/dzs.  A term whose weight is 0 is not evaluated and reads 0.  No kept
    pixel and wf > 0: Focal and L_hard are NaN (0/0) with NaN bounds, the caller asserts the NaN.
    mutate: "swap_ab" / "no_mean" evaluate a wrong formula on purpose (the mutation check of the host test)."""
    B, NC, HW = zs.shape
    dt, dev = zs.dtype, zs.device
    gamma, wf, wt, a, b, s = (sp[k] for k in KEYS)
    if mutate == "swap_ab":
        a, b = b, a
    y = target.reshape(B, 1, HW)
    keep = (y != ignore_index) & (y >= 0) & (y < NC)
    ys = torch.where(keep, y, torch.zeros_like(y))
    kf = keep.to(dt)
    oh = torch.zeros_like(zs).scatter_(1, ys, 1.0) * kf
    w = (torch.ones(NC, dtype=dt, device=dev) if cw is None else cw.to(dt))[ys] * kf          # [B, 1, HW]
    zero = torch.zeros((), dtype=dt, device=dev)
    klr = L.seg_loss(zs, zt, torch.full_like(target, ignore_index), cw, ignore_index, T, alpha, gs, n_seq, want_grad)
    kl, e_kl = klr["losses"][0][1], klr["losses"][1][1]
    p, lp, e_lp, rel_p = _softmax(zs, 1.0)
    py, lpy = (p * oh).sum(1, keepdim=True), (lp * oh).sum(1, keepdim=True)
    om = (p * (kf - oh)).sum(1, keepdim=True)                    # 1 - p_y: the other classes' probabilities, NC - 2 additions
    rel_om = rel_p + _bound(max(NC - 2, 0), 1.0)
    sw = w.sum()
    e_sw = _bound(n_seq, sw)
    e_l2 = e_sw + _bound(1, sw)

    # ---- focal value
    f, ops_f = _pow(om, gamma)
    rel_f = gamma * rel_om + ops_f
    focal, e_focal = zero, zero
    if wf > 0:
        t = w * f * (-lpy)                                           # >= 0
        fnum = t.sum()
        # log p_y enters with its absolute bound times the factor; the factor with its relative bound; the two products and
        # the fused add on top of the reduction
        e_fnum = (w * f * e_lp + t * rel_f + TINY * w).sum() + _bound(n_seq + 3, fnum)
        focal = fnum / sw
        e_focal = (e_fnum + focal.abs() * e_sw) / sw + _bound(1, focal.abs())

    # ---- Tversky value and the per-class gradient coefficients
    TI = torch.zeros(NC, dtype=dt, device=dev)
    e_TI, tv, e_tv = torch.zeros_like(TI), zero, zero
    if wt > 0:
        TP, A, N = (p * oh).sum((0, 2)), (p * kf).sum((0, 2)), oh.sum((0, 2))
        e_p = rel_p * p + TINY
        e_TP = (e_p * oh).sum((0, 2)) + _bound(n_seq, TP)
        e_A = (e_p * kf).sum((0, 2)) + _bound(n_seq, A)
        FP, FN = A - TP, N - TP
        Un, D = TP + s, TP + a * FP + b * FN + s
        e_D = abs(1.0 - a - b) * e_TP + a * e_A + _bound(6, TP + a * (A + TP) + b * (N + TP) + s)
        TI = Un / D
        e_raw = e_TP / D + TI * e_D / D + _bound(2, TI)             # the sum TP + s, the division
        e_TI = e_raw + _bound(1, TI)                                # stored as fp32
        mean = TI.sum() if mutate == "no_mean" else TI.sum() / NC
        tv = 1.0 - mean
        e_tv = e_raw.sum() / NC + _bound(NC + 2, mean + 1.0)        # NC - 1 additions, the division, the difference, the store
        coef = wt if mutate == "no_mean" else wt / NC
        ns = a * FP + b * (N + s)                                   # D - U (1 - b) without its cancellation (FN + TP = N)
        e_ns = a * (e_A + e_TP) + _bound(4, a * (A + TP) + b * (N + s))
        qs = -coef * ns / (D * D)
        e_qs = coef * (e_ns / D ** 2 + 2 * ns * e_D / D ** 3) + _bound(5, qs.abs())
        no = Un * a
        qo = coef * no / (D * D)
        e_qo = coef * ((a * e_TP + _bound(2, no)) / D ** 2 + 2 * no * e_D / D ** 3) + _bound(5, qo.abs())
    hard = wf * focal + wt * tv
    e_hard = wf * e_focal + wt * e_tv + _bound(3, wf * focal.abs() + wt * tv.abs())
    out = {"vals": (torch.cat([torch.stack([hard, kl, sw, focal, tv]), TI]),
                    torch.cat([torch.stack([e_hard, e_kl, e_l2, e_focal, e_tv]), e_TI]))}
    if not want_grad:
        return out

    g, e_g = klr["dzs"]                                             # the KL part (zero without a teacher) and its bound
    ga = g.abs()
    if wf > 0:
        if gamma == 0:
            F, e_F = -torch.ones_like(om), torch.zeros_like(om)
        else:
            pw1, ops1 = _pow(om, gamma - 1.0)
            t1 = gamma * py * pw1 * lpy                              # <= 0, like -f: the bracket has no cancellation
            e_t1 = t1.abs() * (rel_p + (gamma - 1.0) * rel_om + ops1) + gamma * py * pw1 * e_lp + _bound(3, t1.abs()) + TINY
            F = t1 - f
            e_F = e_t1 + f * rel_f + TINY + _bound(1, t1.abs() + f)
        r_sw = torch.where(sw > 0, e_l2 / sw.clamp_min(1e-300), torch.zeros_like(sw))        # the kernel divides by vals[2]
        c = torch.where(keep, wf * w * gs / sw, torch.zeros_like(w))
        d = oh * om - (kf - oh) * p                                 # [j == y] - p_j with 1 - p_y as `om`
        rel_d = oh * rel_om + (kf - oh) * rel_p
        gf = c * F * d
        # the coefficient's five operations (wf w, gs, / sum w, F, d) on top of the bounds of its factors
        e_f = c.abs() * (e_F * d.abs() + F.abs() * (rel_d * d.abs() + TINY)) + (r_sw + _bound(5, 1.0)) * gf.abs()
        g, ga, e_g = g + gf, ga + gf.abs(), e_g + e_f
    if wt > 0:
        sel = oh > 0
        q = torch.where(sel, qs.view(1, NC, 1), qo.view(1, NC, 1))
        e_q = torch.where(sel, e_qs.view(1, NC, 1), e_qo.view(1, NC, 1)) + _bound(1, q.abs())         # read back as fp32
        dot, adot = (p * q).sum(1, keepdim=True), (p * q.abs()).sum(1, keepdim=True)
        e_dot = (p * e_q).sum(1, keepdim=True)
        gt = gs * p * (q - dot) * kf                                # softmax Jacobian: p_j (q_j - sum_c p_c q_c)
        gta = abs(gs) * p * (q.abs() + adot) * kf
        e_p = rel_p * p + TINY
        e_t = abs(gs) * kf * (p * (e_q + e_dot) + e_p * (q.abs() + adot) + p * rel_p * adot) + _bound(NC + 4, gta)
        g, ga, e_g = g + gt, ga + gta, e_g + e_t
    out["dzs"] = (g, e_g + _bound(2, ga))                           # the two fused adds that join the three parts
    return out


def autograd_loss(zs, zt, target, cw, ignore_index, T, alpha, sp):
    """L_hard + alpha*T^2*KL written with stock torch ops for torch.autograd (zs requires grad) -> (total, hard, focal, tversky)"""
    B, NC, HW = zs.shape
    gamma, wf, wt, a, b, s = (sp[k] for k in KEYS)
    keep = (target != ignore_index) & (target >= 0) & (target < NC)
    p = torch.softmax(zs, 1).permute(0, 2, 1)[keep]                 # [K, NC]
    yk = target[keep]
    oh = torch.nn.functional.one_hot(yk, NC).to(zs.dtype)
    w = torch.ones(NC, dtype=zs.dtype) if cw is None else cw
    wk = w[yk]
    logp = torch.log_softmax(zs, 1).permute(0, 2, 1)[keep]
    om = (p * (1 - oh)).sum(1)
    fac = torch.ones_like(om) if gamma == 0 else om ** gamma
    focal = (wk * fac * -(logp * oh).sum(1)).sum() / wk.sum()
    TP, A, N = (p * oh).sum(0), p.sum(0), oh.sum(0)
    tv = 1 - ((TP + s) / (TP + a * (A - TP) + b * (N - TP) + s)).mean()
    hard = (wf * focal if wf > 0 else 0) + (wt * tv if wt > 0 else 0)
    kl = 0.0
    if zt is not None:
        kl = torch.nn.functional.kl_div(torch.log_softmax(zs / T, 1), torch.log_softmax(zt / T, 1), reduction="sum",
                                        log_target=True) / (B * HW)
    return hard + alpha * T * T * kl, hard, focal, tv


# ---- inputs and cases shared by the host self-check and tests/test_gpu_region_loss.py -----------------------------------------

GAP = 40.0


def region_inputs(B, NC, HW, seed, device, ignore_index=-1, weights=True, teacher=True, absent=False):
    """logits N(0, 3^2); about 20 % of the labels ignore_index, 3 % each NC + 1 and -7; a leading block of pixels whose label's
    logit stands GAP above (even pixels: p_y ~ 1) or below (odd pixels: p_y ~ 4e-18) the others; absent: no pixel of class NC-1"""
    g = torch.Generator(device=device).manual_seed(seed)
    zs = torch.randn(B, NC, HW, generator=g, device=device) * 3.0
    zt = torch.randn(B, NC, HW, generator=g, device=device) * 3.0 if teacher else None
    y = torch.randint(0, NC, (B, HW), generator=g, device=device)
    r = torch.rand(B, HW, generator=g, device=device)
    for lo, hi, bad in ((0.0, 0.2, ignore_index), (0.2, 0.23, NC + 1), (0.23, 0.26, -7)):
        y = torch.where((r >= lo) & (r < hi), torch.full_like(y, bad), y)
    npix = B * HW
    k = max(2, min(512, npix // 3))
    i = torch.arange(npix, device=device)
    blk = (i < k).view(B, HW)
    yb = (i % NC).view(B, HW)
    y = torch.where(blk, yb, y)
    if absent:
        y = torch.where(y == NC - 1, torch.zeros_like(y), y)
        yb = torch.where(yb == NC - 1, torch.zeros_like(yb), yb)
    sign = torch.where(i % 2 == 0, GAP, -GAP).view(B, 1, HW)
    at = torch.zeros_like(zs).scatter_(1, yb.view(B, 1, HW), 1.0)
    zs = torch.where(blk.view(B, 1, HW), zs / 3.0 + at * sign, zs)
    cw = torch.rand(NC, generator=g, device=device) * 3 + 0.2 if weights else None
    return zs, zt, y, cw


# pixel counts: the ladder of _fp64_loss_ref (a few pixels, one partial block, the 1024 x 256 grid cap - 1, the cap, the cap + 1
# where a thread takes a second iteration) and a ragged third iteration over B = 3 frames of an odd HW
LADDER = {k: L.SEG_LADDER[k] for k in ("few", "partial_block", "cap-1", "cap", "cap+1")}
LADDER["ragged"] = (3, 203891)
X4 = L.SEG_X4
PSETS = {"default": {}, "gamma1": {"gamma": 1.0}, "gamma0": {"gamma": 0.0}, "wf0": {"wf": 0.0}, "wt0": {"wt": 0.0},
         "dice": {"a": 0.5, "b": 0.5}, "gdev": {}}
# (ignore_index, T) per variant; the "gdev" set adds a host gradient scale of 2.5 and a device upstream gradient of 0.5
VARIANTS = [(-1, 4.0), (255, 1.0), (-1, 1.0), (255, 4.0)]
Case = collections.namedtuple("Case", "size NC weights teacher grad pset absent variant")
CROSS = [(nc, w, t, g) for nc in (2, 3, 4) for w in (True, False) for t in (True, False) for g in (True, False)]
PRUNED = [(2, True, True, True), (3, False, True, True), (4, True, False, True), (3, True, True, False)]


def _cases():
    names, out = list(PSETS), []
    for si, size in enumerate(("few", "partial_block")):
        for i, c in enumerate(CROSS):
            out.append(Case(size, *c, names[(i + 3 * si) % len(names)], i % 3 == 0, i + si))
    for si, size in enumerate(("cap-1", "cap", "cap+1", "ragged")):
        for i, c in enumerate(PRUNED):
            out.append(Case(size, *c, names[(4 * si + i) % len(names)], (si + i) % 2 == 1, si + i))
    return out


CASES = _cases()
X4_CASE = Case(X4, 2, True, True, True, "default", False, 0)
ALPHA = 0.7


def case_id(c):
    return "%s-NC%d-w%d-t%d-g%d-%s" % (c.size if isinstance(c.size, str) else "x4", c.NC, c.weights, c.teacher, c.grad, c.pset)


def case_setup(c, device):
    """-> (tensors (zs, zt, y, cw), call arguments dict) of a case"""
    B, HW = LADDER[c.size] if isinstance(c.size, str) else c.size
    ign, T = VARIANTS[c.variant % 4]
    npix = B * HW
    t = region_inputs(B, c.NC, HW, npix % 997 + 10 * c.NC + c.variant, device, ign, c.weights, c.teacher, c.absent)
    gscale, gdev = (2.5, 0.5) if c.pset == "gdev" else (1.0, None)
    return t, dict(B=B, HW=HW, npix=npix, ign=ign, T=f32(T), alpha=f32(ALPHA), gscale=gscale, gdev=gdev,
                   gs=f32(gscale) * (1.0 if gdev is None else f32(gdev)), sp=spec(**PSETS[c.pset]), n_seq=seg_n_seq(npix))


def case_reference(c, tensors, a, dtype=torch.float64, **kw):
    zs, zt, y, cw = tensors
    cv = lambda t: None if t is None else t.to(dtype)
    return region_loss(cv(zs), cv(zt), y, cv(cw), a["ign"], a["T"], a["alpha"], a["gs"], a["n_seq"], a["sp"], want_grad=c.grad, **kw)
