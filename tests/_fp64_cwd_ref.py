"""Float64 reference of the channel-wise distillation feature term (kd_feat_cwd_fwd_bwd, csrc/kd_loss_cwd.hip), written from its
definition, with the rounding-error bound each kernel output must meet, in the convention of tests/_fp64_loss_ref.py:

    err = C_BOUND * n_seq * U * sum |t_i|

    x = X / tau,   phi(X)[b,i,c] = exp(x - M) / S,  M = max_i x,  S = sum_i exp(x - M),  log phi = (x - M) - log S
    val = tau^2 / (B*C) * sum_{b,c} sum_i phi(t) (log phi(t) - log phi(s)),     ds = k (phi(s) - phi(t))

`cwd` takes the kernel's fp32 inputs as [B, HW, C] (the NHWC matrix, any device) and evaluates in the inputs' dtype: float64 for
the reference, float32 for the self-check that a plain fp32 evaluation meets the same bound (tests/test_fp64_cwd_ref_host.py).
tau and the gradient coefficient enter as the fp32 values the kernel receives (`f32`).  `expf` / `logf` / the reciprocal each
count as one operation.  No tolerance is picked by hand and there is no outlier allowance.

Operation count, from the kernel's launch layout (`layout`: a thread owns 4 channels and every `slots`-th row of a chunk of
slots * 64 rows, in register steps of 8 rows; the slots of a chunk are joined in order, then the chunks of an image):

  exponent   x - M of an exponential: x = X * (1/tau) is the reciprocal and the product (2 operations on |x|, none when tau is a
             power of two: both are exact then), the maximum's the same, the difference (1 on M - x): an ABSOLUTE error of the
             exponent, so a RELATIVE one of the exponential.
  S          a term reaches the image's sum as exp(x - m_1) exp(m_1 - m_2) ... exp(m_k - M) with x <= m_1 <= ... <= M: the m_j are
             fp32 numbers, the exponents telescope exactly and their differences add up to M - x, so the roundings of all the
             differences together stay within the one operation on M - x above; every link adds its expf and its product
             (relative): n_chain = steps of a thread (<= 8) + the slot join + the chunk join links.  The additions: rows of a
             thread + the slots that hold a row (adding an exact 0 rounds nothing) + the chunks (n_sum).
             rel(S) = sum_i phi_i * (exponent error of i) + bound(1 + 2 n_chain + n_sum, 1).
  stats      [max, log S, of s then of t] (the log-sum-exp of x is max + log S; the kernel never forms that sum).  The maximum:
             the operations of x (relative).  log S: rel(S) enters absolutely, + logf.
  log phi    the exponent's error, the error of log S, the last difference (1 operation on |log phi|).
  phi        the exponent's error and rel(S) (relative), expf, the reciprocal, the product (3); + TINY when it left the normal range.
  val        per term phi(t) d, d = log phi(t) - log phi(s): phi(t) times the two log-probability errors, |d| times the error of
             phi(t), the difference and the fused multiply-add; the sum over 4 * rows of a thread + 6 wave steps + 3 waves
             (n_val); the workgroup values are summed in double; the coefficient and the conversion (1).
  ds         k = gcoef * gscale_dev[0] (1), the difference of the two probabilities (1, after their own errors), the product (1).
"""
import math

import torch

from _fp64_loss_ref import TINY, _bound, f32
from _fp64_tail_ref import C_BOUND, U  # noqa: F401  (the constants of `_bound`)

THREADS, BATCH, NBATCH = 256, 8, 8
ROWS_PER_THREAD = BATCH * NBATCH
MAX_C = 512


def layout(HW, C):
    """(groups, slots, rows per chunk, chunks per image) of the statistics and the point-wise kernel"""
    groups = C // 4
    slots = THREADS // groups
    chunk_rows = slots * ROWS_PER_THREAD
    return groups, slots, chunk_rows, -(-HW // chunk_rows)


def ws_bytes(B, HW, C):
    return 4 * B * layout(HW, C)[3] * (4 * C + 1)


def n_seq(HW, C):
    """(n_chain, n_sum, n_val) of an image of HW rows: see the module docstring"""
    _, slots, chunk_rows, nchunk = layout(HW, C)
    rows = min(HW, chunk_rows)                    # of the fullest chunk
    per_thread = -(-rows // slots)
    n_chain = min(NBATCH, -(-per_thread // BATCH)) + 2
    n_sum = per_thread + min(slots, rows) + nchunk
    n_val = 4 * per_thread + 6 + 3
    return n_chain, n_sum, n_val


def _n_x(tau):
    """operations behind x = X * (1 / tau): the reciprocal and the product, none when tau is a power of two (both exact)"""
    return 0 if math.frexp(tau)[0] == 0.5 else 2


def _column_softmax(z, tau, HW, C, lse_rel=0.0):
    """z [B, HW, C] -> dict of M, L = log S [B, 1, C] with their bounds, lp and p [B, HW, C] with the absolute bound of lp and the
    relative bound of p.  lse_rel: a relative perturbation of the log-sum-exp M + L (a negative control)"""
    n_chain, n_sum, _ = n_seq(HW, C)
    x = z / tau
    M = x.amax(1, keepdim=True)
    d = x - M
    e = torch.exp(d)
    S = e.sum(1, keepdim=True)
    p = e / S
    L = torch.log(S)
    L = L + lse_rel * (M + L)
    e_exponent = _bound(_n_x(tau), x.abs() + M.abs()) + _bound(1, d.abs())
    rel_S = (p * e_exponent).sum(1, keepdim=True) + _bound(1 + 2 * n_chain + n_sum, 1.0)
    e_L = rel_S + _bound(1, L.abs())
    lp = d - L
    e_lp = e_exponent + e_L + _bound(1, lp.abs())
    rel_p = e_exponent + rel_S + _bound(3, 1.0)
    return {"M": M, "e_M": _bound(_n_x(tau), M.abs()), "L": L, "e_L": e_L, "lp": lp, "e_lp": e_lp, "p": p, "rel_p": rel_p}


def cwd(s, t, tau, k, want_grad=True, lse_rel=0.0, coef_power=2, snap=None):
    """s, t [B, HW, C]; tau the fp32 value; k = gcoef * gscale_dev[0] as the exact product of the two fp32 values.
    -> {"stats": ([B, C, 4], bound), "val": (scalar, bound), "ds": ([B, HW, C], bound)}.
    Negative controls: lse_rel perturbs the student's log-sum-exp (max + log S) relatively, coef_power = 1 uses tau in place of tau^2, snap (a dtype)
    rounds the inputs to that dtype first."""
    B, HW, C = s.shape
    if snap is not None:
        s, t = s.to(snap).to(s.dtype), t.to(snap).to(t.dtype)
    _, _, n_val = n_seq(HW, C)
    a, b = _column_softmax(s, tau, HW, C, lse_rel), _column_softmax(t, tau, HW, C)
    stats = torch.stack([a["M"][:, 0], a["L"][:, 0], b["M"][:, 0], b["L"][:, 0]], 2)
    e_stats = torch.stack([a["e_M"][:, 0], a["e_L"][:, 0].expand(B, C), b["e_M"][:, 0], b["e_L"][:, 0].expand(B, C)], 2)
    d = b["lp"] - a["lp"]
    term = b["p"] * d
    e_term = b["p"] * (b["e_lp"] + a["e_lp"]) + (b["rel_p"] * b["p"] + TINY) * d.abs() + _bound(2, term.abs())
    coef = tau ** coef_power / (B * C)
    val = coef * term.sum()
    e_val = coef * (e_term.sum() + _bound(n_val, term.abs().sum())) + _bound(1, val.abs())
    out = {"stats": (stats, e_stats), "val": (val, e_val), "phi_s": a["p"], "phi_t": b["p"]}
    if want_grad:
        g = k * (a["p"] - b["p"])
        e_g = abs(k) * (a["rel_p"] * a["p"] + b["rel_p"] * b["p"] + 2 * TINY) + _bound(3, abs(k) * (a["p"] + b["p"]))
        out["ds"] = (g, e_g)
    return out


# ---- inputs shared by the host self-check and tests/test_gpu_cwd_loss.py ------------------------------------------------------

def cwd_inputs(B, HW, C, seed, device, scene="normal"):
    """student and teacher matrices [B, HW, C] (the teacher a noisy copy of the student, as a trained pair is):
    "normal": N(0, 1.5^2); "wide": N(0, 8^2); "spikes": N(0, 2^2) with about 0.1 % of the entries at +-80 (a third of the
    columns of a 1024-row image hold a +80: at a small tau every other probability of such a column underflows); "relu": max(0, N(0, 2^2)) (about half the entries exactly 0) with, in every image,
    channel 0 all 0, channel 1 all 1.5 (HW >= 1), channel 2 with its maximum 9.0 tied at three rows and channel 3 tied between
    the first and the last row"""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(B, HW, C, generator=g)
    sd = {"normal": 1.5, "wide": 8.0, "spikes": 2.0, "relu": 2.0}[scene]
    s = r() * sd
    t = s * 0.7 + r() * (0.6 * sd)
    if scene == "spikes":
        for z in (s, t):
            u = torch.rand(B, HW, C, generator=g)
            z[u < 0.0005] = 80.0
            z[(u >= 0.0005) & (u < 0.001)] = -80.0
    if scene == "relu":
        s, t = s.clamp_min(0.0), t.clamp_min(0.0)
        for z in (s, t):
            z[:, :, 0] = 0.0
            z[:, :, 1] = 1.5
            z[:, [0, HW // 3, HW - 2], 2] = 9.0
            z[:, [0, HW - 1], 3] = z[:, :, 3].amax(1, keepdim=True) + 0.25
    return s.to(device).contiguous(), t.to(device).contiguous()


# (B, HW, C, tau, scene): one row; fewer rows than slots and two channel groups; HW one past a power of two with C no multiple of
# 32 (252 live threads); underflowing teacher probabilities; the workload's HW and C; one float4 column over many rows (256 slots);
# an odd batch of wide rows (4 slots)
CASES = [(1, 1, 4, 1.0, "normal"), (2, 63, 8, 4.0, "normal"), (3, 257, 36, 1.0, "wide"), (2, 1024, 128, 0.5, "spikes"),
         (2, 4096, 128, 4.0, "relu"), (1, 16384, 4, 1.0, "normal"), (5, 100, 256, 2.0, "normal")]


def case_id(c):
    return "B%d-HW%d-C%d-tau%g-%s" % c


def case_setup(case, device):
    """-> (s, t, tau (the fp32 value), gcoef, gdev or None, k): every second case passes part of the coefficient on the device"""
    B, HW, C, tau, scene = case
    i = CASES.index(case)
    s, t = cwd_inputs(B, HW, C, 300 + i, device, scene)
    tau = f32(tau)
    gcoef, gdev = f32(tau / (B * C)), None
    if i % 2:
        gcoef, gdev = f32(gcoef * 2.5), f32(0.3)
    return s, t, tau, gcoef, gdev, gcoef * (1.0 if gdev is None else gdev)
