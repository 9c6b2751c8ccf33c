"""Float64 references for the loss, metric and optimiser kernels of csrc/kd_loss.hip, with the rounding-error bound each
kernel output must meet, in the convention of tests/_fp64_tail_ref.py:

    err = C_BOUND * n_seq * U * sum |t_i|

Every function takes the kernel's fp32 inputs (any device) and evaluates in the inputs' dtype: float64 for the reference,
float32 for the self-check that a plain fp32 evaluation meets the same bound (tests/test_fp64_loss_ref_host.py).  Scalars
(T, alpha, the gradient scale, the AdamW hyper-parameters) enter as the fp32 values the kernel receives (`f32`).
`expf` / `logf` / `sqrtf` each count as one operation of the chain.  Where a rounded intermediate feeds a nonlinear step its
error enters through the derivative: an absolute error of an exponent is a relative error of the exponential, a relative
error of the softmax denominator an absolute error of its logarithm (hence the `+ 1` among the terms of a log-softmax).
Reductions take n_seq from the launch layout (`seg_n_seq`, `mse_n_seq`): iterations per thread + 6 wave steps + 4 waves;
the slab and final sums are double and add nothing.  The KD total is specified as fp32 operations in a fixed order and
compared bit for bit; the confusion matrix is integer."""
import math

import numpy as np
import torch

from _fp64_tail_ref import C_BOUND, U

TINY = 2.0 ** -126       # smallest normal fp32: the absolute error of a value that left the normal range (or was flushed)


def f32(x):
    """the fp32 value a `float` argument of the C ABI arrives as"""
    return float(np.float32(x))


def _bound(n_seq, terms):
    return C_BOUND * n_seq * U * terms


# ---- launch layouts -------------------------------------------------------------------------------------------------------

def seg_layout(npix):
    """(grid, iterations per thread) of the loss and metric kernels: 256 threads, at most 1024 blocks"""
    grid = min(-(-npix // 256), 1024)
    return grid, -(-npix // (grid * 256))


def seg_n_seq(npix):
    return seg_layout(npix)[1] + 6 + 4


def mse_layout(n):
    """(grid, iterations per thread) of the MSE kernel: one float4 per thread and iteration, at most 2048 blocks"""
    n4 = n // 4
    grid = max(1, min(-(-n4 // 256), 2048))
    return grid, -(-n4 // (grid * 256))


def mse_n_seq(n):
    return 4 * mse_layout(n)[1] + 6 + 4


def adamw_layout(n):
    grid = min(-(-n // 256), 2048)
    return grid, -(-n // (grid * 256))


def tail_mask(n, grid, iters, device, per=256):
    """the elements a grid-stride loop handles last or at its edges: the last (ragged) iteration, the last block, 0, n-1"""
    i = torch.arange(n, device=device)
    sel = (i >= (iters - 1) * grid * per) | ((i // per) % grid == grid - 1)
    sel[0] = sel[-1] = True
    return sel


# ---- segmentation loss ----------------------------------------------------------------------------------------------------

def _softmax(z, invT):
    """z [B, NC, HW] -> (p, logp, e_lp, rel_p): temperature softmax over dim 1 as the kernel forms it (x = z*invT - max,
    p = exp(x) / s, logp = x - log s) with the absolute bound of logp and the relative bound of p, both [B, 1, HW]"""
    NC = z.shape[1]
    x = z * invT
    A = x.abs().amax(1, keepdim=True)
    x = x - x.amax(1, keepdim=True)
    e = torch.exp(x)
    s = e.sum(1, keepdim=True)
    ls = torch.log(s)
    # exponent: product and difference of values up to A (absolute 2A); exp; NC-1 adds: relative error of s, absolute of log s;
    # logf and the two differences act on |x| + ls <= 2A + ls
    e_lp = _bound(NC + 5, 2 * A + ls + 1)
    rel_p = _bound(NC + 4, 2 * A + 1)            # exponent, exp, the sum, the division
    return e / s, x - ls, e_lp, rel_p


def seg_loss(zs, zt, target, cw, ignore_index, T, alpha, gs, n_seq, want_grad=True):
    """zs, zt [B, NC, HW] (zt None: CE only), target int64 [B, HW], cw [NC] or None; T, alpha fp32 values, gs = the upstream
    gradient gscale * gscale_dev[0] (two fp32 values multiplied: one operation, counted below).
    -> losses [3] = (weighted-mean CE, per-pixel-mean KL, weight sum) and dzs = gs * d(CE + alpha*T^2*KL)/dzs.
    Labels equal to ignore_index, negative or >= NC are dropped from CE and still take part in KL.  No kept pixel: CE is
    0/0 = NaN (as torch's), its bound NaN; the caller asserts the NaN."""
    B, NC, HW = zs.shape
    dt = zs.dtype
    npix = B * HW
    invT = float(np.float32(1.0) / np.float32(T))
    y = target.reshape(B, 1, HW)
    keep = (y != ignore_index) & (y >= 0) & (y < NC)
    ys = torch.where(keep, y, torch.zeros_like(y))
    oh = torch.zeros_like(zs).scatter_(1, ys, 1.0) * keep
    w = (torch.ones(NC, dtype=dt, device=zs.device) if cw is None else cw.to(dt))[ys] * keep       # [B, 1, HW]
    p1, lp1, e_lp1, rel_p1 = _softmax(zs, 1.0)
    nll = -(lp1 * oh).sum(1, keepdim=True)
    swn, sw = (w * nll).sum(), w.sum()
    e_swn = (w * e_lp1).sum() + _bound(n_seq + 1, (w * nll.abs()).sum())
    e_sw = _bound(n_seq, sw)
    ce = swn / sw
    e_ce = (e_swn + ce.abs() * e_sw) / sw + _bound(1, ce.abs())
    e_l2 = e_sw + _bound(1, sw)
    kl, e_kl = torch.zeros((), dtype=dt, device=zs.device), torch.zeros((), dtype=dt, device=zs.device)
    if zt is not None:
        ps, lps, e_lps, rel_ps = _softmax(zs, invT)
        pt, lpt, e_lpt, rel_pt = _softmax(zt, invT)
        d = lpt - lps
        t = pt * d
        skl = t.sum()
        e_skl = (pt * (e_lpt + e_lps) + (rel_pt + _bound(NC + 2, 1.0)) * t.abs() + TINY * d.abs()).sum() + _bound(n_seq + NC, t.abs().sum())
        kl = skl / npix
        e_kl = e_skl / npix + _bound(1, kl.abs())
    out = {"losses": (torch.stack([ce, kl, sw]), torch.stack([e_ce, e_kl, e_l2]))}
    if want_grad:
        r_sw = torch.where(sw > 0, e_l2 / sw.clamp_min(1e-300), torch.zeros_like(sw))     # the kernel divides by losses[2]
        c = torch.where(keep, w * gs / sw, torch.zeros_like(w))                            # 0 / 0 of an all-ignored batch: unused
        g = c * (p1 - oh)
        ga = c * (p1 + oh)
        e_g = c * (rel_p1 * p1 + TINY) + r_sw * ga          # TINY: a probability that underflowed
        if zt is not None:
            klc = gs * alpha * T / npix
            g = g + klc * (ps - pt)
            ga = ga + abs(klc) * (ps + pt)
            e_g = e_g + abs(klc) * (rel_ps * ps + rel_pt * pt + 2 * TINY)
        # the coefficient (gs, its products and the division) and the fused multiply-add into the sum
        out["dzs"] = (g, e_g + _bound(6, ga))
    return out


# ---- feature MSE ----------------------------------------------------------------------------------------------------------

def mse_value(a, b, n_seq, dtype=None, chunk=1 << 26):
    """mean((a-b)^2) over flat a, b evaluated in `dtype` (default: the inputs'), converted and summed in chunks of `chunk`
    elements (the float64 copies of a 2^31-element case do not fit otherwise).  Per term: the difference, its square (twice
    its relative error), the fused add."""
    a, b = a.reshape(-1), b.reshape(-1)
    n, dt = a.numel(), dtype or a.dtype
    s = torch.zeros((), dtype=dt, device=a.device)
    for o in range(0, n, chunk):
        d = a[o:o + chunk].to(dt) - b[o:o + chunk].to(dt)
        s = s + (d * d).sum()
    v = s / n
    return {"loss": (v, _bound(n_seq + 4, v))}                  # + the division by n


def mse_grad(a, b, gcoef, gdev=1.0):
    """da = gcoef * gscale_dev[0] * (a - b): the coefficient product, the difference (exact inputs: relative), the product"""
    g = (gcoef * gdev) * (a - b)
    return {"da": (g, _bound(3, g.abs()))}


# ---- KD total -------------------------------------------------------------------------------------------------------------

def kd_total(ce, kl, mse_c, mse_l, ckl, beta):
    """total = ce + ckl * kl + beta * (mse_c + mse_l), every operation rounded to fp32 in this order; a missing MSE is 0.
    Returns a numpy.float32: the comparison is bit-exact."""
    F = np.float32
    t = F(F(ce) + F(F(ckl) * F(kl)))
    m = F(F(0.0 if mse_c is None else mse_c) + F(0.0 if mse_l is None else mse_l))
    return F(t + F(F(beta) * m))


# ---- AdamW ----------------------------------------------------------------------------------------------------------------

def bias_corrections(b1, b2, step, round32=True):
    """(1 - b1^step, sqrt(1 - b2^step)) evaluated in double from the given betas; round32: as the kernels receive them"""
    bc1, bc2s = 1.0 - math.pow(b1, step), math.sqrt(1.0 - math.pow(b2, step))
    return (f32(bc1), f32(bc2s)) if round32 else (bc1, bc2s)


def adamw_tick(state, b1, b2):
    """state (lr, step, bc1, bc2sqrt) -> the state after adamw_tick_kernel, as float64 values and their bound (the step
    count is exact; each correction is one rounding of a double)"""
    t = state[1] + 1.0
    bc1, bc2s = bias_corrections(b1, b2, t, round32=False)
    return [state[0], t, bc1, bc2s], [0.0, 0.0, _bound(1, bc1), _bound(1, bc2s)]


def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, ginv):
    """One step of torch.optim.AdamW's arithmetic on flat tensors:
        gi = g * ginv;  p *= 1 - lr * wd;  m = b1 m + (1 - b1) gi;  v = b2 v + (1 - b2) gi^2;
        p -= (lr / bc1) * m / (sqrt(v) / bc2s + eps)
    with a bound per element.  denom is a sum of non-negative terms and the one cancellation (b1 m + (1 - b1) gi) is
    covered by sum|t_i|, so no element is excluded."""
    gi = g * ginv
    pd = p * (1.0 - lr * wd)
    ta, tb = b1 * m, (1.0 - b1) * gi
    mi = ta + tb
    e_m = _bound(4, ta.abs() + tb.abs())                       # gi, 1 - b1, the products, the sum
    vi = b2 * v + (1.0 - b2) * gi * gi
    e_v = _bound(6, vi)                                        # gi twice, 1 - b2, two products, the sum
    sq = vi.sqrt()
    denom = sq / bc2s + eps
    e_den = 0.5 * torch.where(vi > 0, e_v / sq.clamp_min(1e-300), torch.zeros_like(vi)) / bc2s + _bound(3, denom)
    u = (lr / bc1) * (mi / denom)
    e_u = (lr / bc1) * (e_m / denom + mi.abs() * e_den / (denom * denom)) + _bound(3, u.abs())
    return {"p": (pd - u, e_u + _bound(4, pd.abs() + u.abs())),   # lr * wd, 1 - ., the product, the difference
            "m": (mi, e_m), "v": (vi, e_v)}


# ---- argmax + confusion ---------------------------------------------------------------------------------------------------

def confusion(z, target, M, ignore_index):
    """z [B, NC, HW], target int64 [B, HW] or None -> (pred [B, HW], conf [M, M]) int64.  pred is the argmax over all NC classes,
    the first maximum wins (+-inf compare as numbers, -0.0 == +0.0); a pixel counts at [t, pred] when t != ignore_index and
    0 <= t < M and pred < M (SegmentationMetrics.update of the reference: M is the matrix width, not the class count)."""
    best = torch.zeros(z.shape[0], z.shape[2], dtype=torch.int64, device=z.device)
    bv = z[:, 0]
    for j in range(1, z.shape[1]):
        up = z[:, j] > bv
        best = torch.where(up, torch.full_like(best, j), best)
        bv = torch.where(up, z[:, j], bv)
    conf = torch.zeros(M, M, dtype=torch.int64, device=z.device)
    if target is not None:
        keep = (target != ignore_index) & (target >= 0) & (target < M) & (best < M)
        conf = torch.bincount(target[keep] * M + best[keep], minlength=M * M).view(M, M)
    return best, conf


# ---- inputs shared by the host self-check and tests/test_gpu_loss_kernels.py ------------------------------------------------

def seg_inputs(B, NC, HW, seed, device, ignore_index=-1, scale=3.0, weights=True, teacher=True):
    """logits of the given scale, labels in 0..NC-1 with about 3 % each of NC, -7 and ignore_index, class weights"""
    g = torch.Generator(device=device).manual_seed(seed)
    zs = torch.randn(B, NC, HW, generator=g, device=device) * scale
    zt = torch.randn(B, NC, HW, generator=g, device=device) * scale if teacher else None
    y = torch.randint(0, NC, (B, HW), generator=g, device=device)
    r = torch.rand(B, HW, generator=g, device=device)
    for k, bad in enumerate((NC, -7, ignore_index)):
        y = torch.where((r >= 0.03 * k) & (r < 0.03 * (k + 1)), torch.full_like(y, bad), y)
    cw = torch.rand(NC, generator=g, device=device) * 3 + 0.2 if weights else None
    return zs, zt, y, cw


def adamw_inputs(n, seed, device):
    """parameters, gradients spanning 1e-12 .. 1e3 with exact zeros, non-zero moments (v >= 0)"""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda: torch.randn(n, generator=g, device=device)
    p = r()
    grad = r().sign() * 10.0 ** (torch.rand(n, generator=g, device=device) * 15 - 12)
    grad = torch.where(torch.rand(n, generator=g, device=device) < 0.05, torch.zeros_like(grad), grad)
    m = r() * 0.1
    v = (r() * 0.1) ** 2
    v = torch.where(torch.rand(n, generator=g, device=device) < 0.05, torch.zeros_like(v), v)
    return p, grad, m, v


def confusion_inputs(B, NC, HW, seed, device, ignore_index=-1):
    """logits on a coarse grid (many exact ties) with +-inf, -0.0 and +0.0 sprinkled in; labels -7 .. 4 and ignore_index"""
    g = torch.Generator(device=device).manual_seed(seed)
    z = torch.randint(-2, 3, (B, NC, HW), generator=g, device=device).float() * 0.5
    r = torch.rand(B, NC, HW, generator=g, device=device)
    for k, val in enumerate((float("inf"), float("-inf"), -0.0, 0.0)):
        z = torch.where((r >= 0.02 * k) & (r < 0.02 * (k + 1)), torch.full_like(z, val), z)
    y = torch.randint(0, 5, (B, HW), generator=g, device=device)
    r = torch.rand(B, HW, generator=g, device=device)
    y = torch.where(r < 0.05, torch.full_like(y, -7), y)
    y = torch.where((r >= 0.05) & (r < 0.12), torch.full_like(y, ignore_index), y)
    return z, y


# ---- sizes, from each launch layout -------------------------------------------------------------------------------------------
# (B, HW) per pixel count: a few pixels, one partial block, cap*256 - 1, cap*256, cap*256 + 1, a ragged third iteration, the
# benchmarked 256 x 64 x 64; HW is no multiple of 256 where the count allows it, so frame boundaries fall inside a block
SEG_LADDER = {"few": (2, 3), "partial_block": (3, 61), "cap-1": (3, 87381), "cap": (4, 65536), "cap+1": (5, 52429),
              "ragged": (2, 305837), "bench": (256, 4096)}
SEG_X4 = (256, 65536)                                   # the x4 head's 256 x 256 x 256
MSE_LADDER = {"few": 8, "partial_block": 3380, "cap-1": 2097148, "cap": 2097152, "cap+1": 2097156, "ragged": 4893356}
MSE_BENCH = 256 * 128 * 64 * 64
MSE_HUGE = 2 ** 31 + 4 * 1031                           # int32 element indices wrap here
ADAMW_LADDER = {"few": 5, "partial_block": 700, "cap-1": 524287, "cap": 524288, "cap+1": 524289, "ragged": 1223339}
PARAM_COUNTS = (528132, 573442, 494978)                 # the three published models
