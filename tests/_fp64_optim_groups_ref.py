"""Float64 reference for parameter groups and the EMA weight copy in the device AdamW step (kd_adamw_step_groups_dev of
csrc/kd_loss.hip), in the convention of tests/_fp64_loss_ref.py and built on its adamw_step, bias_corrections and _bound:

    err = C_BOUND * n_seq * U * sum |t_i|

The grouped step is R.adamw_step with lr and weight_decay as per-element tensors expanded from the segment table (ascending
segment ends in float4 units, one group per segment): the arithmetic per element does not change, so its operation counts hold.

The EMA update is e_new = d * e + (1 - d) * p_new with d the fp32 value the tick kernel left in ema_state[0] (an exact input).
The kernel rounds 1 - d, the product (1 - d) * p_new and the fused multiply-add: three roundings; a plain fp32 evaluation rounds
d * e as well.  n_seq = 4 covers both, over the terms |d e| + |(1 - d) p_new|.  d = 0 and d = 1 are exact in the kernel (it stores
p_new, or leaves e alone): the tests compare those bit for bit.

The warm-up schedule is d_t = min(decay, (1 + t) / (10 + t)) with t the step count after the tick; `ema_decay_at` evaluates it
in fp32 operations (each rounded once, as the header states) or exactly."""
import numpy as np
import torch

import _fp64_loss_ref as R
from _fp64_loss_ref import _bound, f32

EMA_N_SEQ = 4


# ---- the segment table ------------------------------------------------------------------------------------------------------

def segment_table(numels, group_of):
    """Tensor sizes in flat-buffer order and the group of each -> (ends, groups) as lists: every tensor is padded to a multiple
    of 4 floats (the padding belongs to it), consecutive tensors of one group share a segment, ends are in float4 units."""
    ends, groups, pos = [], [], 0
    for n, gi in zip(numels, group_of):
        pos += -(-n // 4)
        if n == 0:
            continue
        if groups and groups[-1] == gi:
            ends[-1] = pos
        else:
            ends.append(pos)
            groups.append(gi)
    return ends, groups


def expand(ends, groups, values, device="cpu", dtype=torch.float64):
    """per-element tensor [4 * ends[-1]] holding values[group] of the segment each element lies in"""
    out = torch.empty(4 * ends[-1], dtype=dtype, device=device)
    lo = 0
    for e, gi in zip(ends, groups):
        out[4 * lo:4 * e] = values[gi]
        lo = e
    return out


def grouped_step(p, g, m, v, ends, groups, lrs, wds, b1, b2, eps, bc1, bc2s, ginv):
    """One AdamW step on flat tensors (all in p's dtype) with lr = lrs[group], weight_decay = wds[group] per element;
    the scalars enter as the fp32 values the kernel reads (f32).  -> R.adamw_step's {"p", "m", "v"}: (value, bound)."""
    lr = expand(ends, groups, [f32(x) for x in lrs], p.device, p.dtype)
    wd = expand(ends, groups, [f32(x) for x in wds], p.device, p.dtype)
    return R.adamw_step(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, ginv)


# ---- the EMA ----------------------------------------------------------------------------------------------------------------

def ema_decay_at(decay, t, warmup, round32=True):
    """d_t for the step count t after the tick.  round32: the kernel's fp32 operations (1 + t, 10 + t, the quotient: one
    rounding each; min is exact); otherwise the exact value in double."""
    if not warmup:
        return f32(decay) if round32 else float(decay)
    if round32:
        one, ten, tt = np.float32(1.0), np.float32(10.0), np.float32(t)
        return float(min(np.float32(decay), (one + tt) / (ten + tt)))
    return min(float(decay), (1.0 + t) / (10.0 + t))


def ema_update(e, p_new, d):
    """e_new = d * e + (1 - d) * p_new in e's dtype -> (value, bound)"""
    ta, tb = d * e, (1.0 - d) * p_new
    return ta + tb, _bound(EMA_N_SEQ, ta.abs() + tb.abs())


# ---- tables for tests/test_gpu_optim_groups.py --------------------------------------------------------------------------------

def launch_layout(n):
    """(grid, iterations per thread) of the update kernel: 256 threads, one float4 each, at most 2048 blocks"""
    n4 = n // 4
    grid = max(1, min(-(-n4 // 256), 2048))
    return grid, -(-n4 // (grid * 256))


def tables_for(n, G):
    """{name: (ends, groups)} over n / 4 float4s for G groups: one segment; a split after the first float4 and before the last;
    a boundary at a workgroup edge (float4 256) and at the iteration edge (grid * 256); 300 segments of alternating groups with
    lengths 1 .. k float4s (more segments than a workgroup has threads).  A table that does not fit the size is left out."""
    n4 = n // 4
    grid = launch_layout(n)[0]
    out = {"one": ([n4], [G - 1])}
    if G == 1:
        return out

    def alt(cuts):
        cuts = sorted({c for c in cuts if 0 < c < n4}) + [n4]
        return cuts, [i % G for i in range(len(cuts))]

    if n4 >= 2:
        out["first"] = alt([1])
        out["last"] = alt([n4 - 1])
    if n4 > 256:
        out["wg_edge"] = alt([256])
    if n4 > grid * 256:
        out["iter_edge"] = alt([grid * 256])
    if n4 >= 300:
        k = max(1, min(7, 2 * n4 // 300 - 1))                      # 299 * (k + 1) / 2 < n4: the 300th segment is not empty
        cuts, pos = [], 0
        for i in range(299):
            pos += 1 + i % k
            cuts.append(pos)
        out["many"] = alt(cuts)
        assert len(out["many"][0]) == 300
    return out
