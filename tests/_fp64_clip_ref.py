"""Float64 reference for global-norm gradient clipping inside the device AdamW step (kd_grad_sumsq_partials and
kd_adamw_step_clip_dev of csrc/kd_loss.hip), with the rounding-error bound each output must meet, in the convention of
tests/_fp64_loss_ref.py:

    err = C_BOUND * n_seq * U * sum |t_i|

Every function evaluates in the dtype of its tensor inputs: float64 for the reference, float32 for the self-check
(tests/test_fp64_clip_ref_host.py).  Scalars (ginv, max_norm) enter as the fp32 values the kernel receives.

The sum of squares takes n_seq from the launch layout (`sumsq_layout`): a thread adds 4 squares per iteration with one fused
multiply-add each, a wave adds its 64 lanes in 6 steps; the 4 waves of a block, the per-block partials and the final sum are
double and add nothing.  The norm is ginv * sqrt(sum) evaluated in double and rounded once: half the relative error of the
sum plus one rounding.  The coefficient min(1, max_norm / (norm + 1e-6)) is two fp32 operations on top of the norm's error
(min is 1-Lipschitz), the gradient scale ginv * coef one more.  The update itself is R.adamw_step with the gradient scale in
the place of ginv."""
import math

import torch

import _fp64_loss_ref as R
from _fp64_loss_ref import _bound, f32

CAP = 2048                     # blocks at most
PER = 256 * 4                  # elements a block takes per iteration: 256 threads, one float4 each
NORM_EPS = f32(1e-6)           # the fp32 constant the kernel adds to the norm (clip_grad_norm_ adds 1e-6)


def sumsq_layout(n):
    """(grid, iterations per thread) of the sum-of-squares kernel"""
    n4 = n // 4
    grid = max(1, min(-(-n4 // 256), CAP))
    return grid, -(-n4 // (grid * 256))


def sumsq_n_seq(n):
    return 4 * sumsq_layout(n)[1] + 6


def sumsq(g, n_seq):
    """sum g_i^2 over flat g in g's dtype (every term is non-negative: sum|t_i| is the sum itself)"""
    s = (g * g).sum()
    return s, _bound(n_seq, s)


def sumsq_kernel_order(g):
    """The kernel's summation order in g's dtype -> the per-block partials as float64 [grid]: thread chains over iterations and
    the four components (w, z, y, x innermost first, as the nested fused multiply-adds evaluate), the 6-step butterfly of a
    wave, then double."""
    n = g.numel()
    grid, iters = sumsq_layout(n)
    x = torch.zeros(iters * grid * PER, dtype=g.dtype)
    x[:n] = g.reshape(-1).cpu()
    x = x.view(iters, grid, 256, 4)
    s = torch.zeros(grid, 256, dtype=g.dtype)
    for it in range(iters):
        for c in (3, 2, 1, 0):
            s = s + x[it, :, :, c] * x[it, :, :, c]
    s = s.view(grid, 4, 64)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, lane ^ o]
    w = s[:, :, 0].double()
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def clip_scalars(s, e_s, ginv, max_norm, norm_eps=NORM_EPS):
    """sum of squares `s` with bound `e_s` (0-d tensors) -> {"norm", "coef", "gscale"}: (value, bound) each.
    norm = ginv * sqrt(s);  coef = min(1, max_norm / (norm + norm_eps));  gscale = ginv * coef."""
    norm = ginv * s.sqrt()
    rel_s = torch.where(s > 0, e_s / s.clamp_min(1e-300), torch.zeros_like(s))
    e_norm = 0.5 * rel_s * norm.abs() + _bound(1, norm.abs())
    d = norm + norm_eps
    c = max_norm / d
    e_c = c * e_norm / d + _bound(2, c)                          # the sum and the division
    coef = c.clamp_max(1.0)
    e_coef = torch.where(c - e_c > 1.0, torch.zeros_like(c), e_c)   # clamped on both sides of the bound: exactly 1
    gs = ginv * coef
    return {"norm": (norm, e_norm), "coef": (coef, e_coef), "gscale": (gs, abs(ginv) * e_coef + _bound(1, gs.abs()))}


def clipped_step(p, g, m, v, lr, b1, b2, eps, wd, step, ginv, max_norm, norm_eps=NORM_EPS, round32=True):
    """One clipped AdamW step number `step` (1-based) on flat tensors, all in g's dtype: the scalars of clip_scalars and
    R.adamw_step with gscale in the place of ginv.  A non-finite norm skips the step: the state comes back unchanged."""
    s, e_s = sumsq(g, sumsq_n_seq(g.numel()))
    sc = clip_scalars(s, e_s, ginv, max_norm, norm_eps)
    if not math.isfinite(float(sc["norm"][0])):
        z = torch.zeros_like(p)
        return {"p": (p, z), "m": (m, z), "v": (v, z), "skipped": True, **sc}
    bc1, bc2s = R.bias_corrections(b1, b2, step, round32=round32)
    out = R.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, sc["gscale"][0])
    return {**out, "skipped": False, **sc}


def tail_only(g, mode):
    """g with everything zeroed except: "first" element 0, "last" element n-1, "ragged" the float4s of the last (ragged)
    iteration -- or of the last block where there is a single iteration -- so that a dropped or doubled element costs O(1)"""
    n = g.numel()
    if mode == "all":
        return g
    keep = torch.zeros(n, dtype=torch.bool, device=g.device)
    if mode == "first":
        keep[0] = True
    elif mode == "last":
        keep[n - 1] = True
    else:
        grid, iters = sumsq_layout(n)
        i4 = torch.arange(n, device=g.device) // 4
        keep = i4 >= (iters - 1) * grid * 256 if iters > 1 else i4 // 256 == grid - 1
    out = torch.where(keep, g, torch.zeros_like(g))
    if float(out.abs().max()) == 0.0:                            # the kept element happened to be an exact zero
        out[n - 1 if mode == "last" else 0] = 0.75
    return out


def grad_inputs(n, seed, device):
    """gradients of mixed magnitude (1e-6 .. 1e1) with exact zeros, as a flat fp32 tensor"""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n, generator=g, device=device) * 10.0 ** (torch.rand(n, generator=g, device=device) * 7 - 6)
    return torch.where(torch.rand(n, generator=g, device=device) < 0.05, torch.zeros_like(x), x)


# ---- sizes, from the launch layout ----------------------------------------------------------------------------------------------
# a few elements, one partial block, cap*per - 4, cap*per, cap*per + 4, a ragged third iteration, and the three published
# parameter counts rounded up to a multiple of 4
CLIP_LADDER = {"few": 8, "partial_block": 3380, "cap-4": CAP * PER - 4, "cap": CAP * PER, "cap+4": CAP * PER + 4,
               "ragged": 2 * CAP * PER + 699052}
for _i, _c in enumerate(R.PARAM_COUNTS):
    CLIP_LADDER[f"model{_i}"] = -(-_c // 4) * 4
TAIL_MODES = ("all", "first", "last", "ragged")
