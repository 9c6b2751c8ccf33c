"""Float64 references for the training backward of the LiDAR point MLP (4 -> 64 -> 128 -> feature_dim): kd_lidar_l2_dgrad /
kd_lidar_l2_wgrad (pw_gemm_kernel<4, 2, ...>, pw_stream_kernel<.., 4, 2, ..>, pw_wgrad_kernel<.., 3, 1, ..>), kd_lidar_l1_dgrad /
kd_lidar_l1_wgrad (pw_gemm_kernel<2, 3, ...>, pw_wgrad_kernel<.., 2, 2, ..>) and the one-kernel forms kd_lidar_l2_bwd /
kd_lidar_l1_bwd (csrc/kd_lidar_bwd.hip).  Same conventions as tests/_fp64_gemm_ref.py, whose rules for n_seq apply: every function
takes the kernel's fp32 inputs (any device; evaluated in the inputs' dtype -- float64 for the truth, float32 for the self-check of
the bound) and returns {name: (value, err)} with err = C_BOUND * n_seq * U * sum |t_i|.

What is specific to these kernels:

  table rebuild        G = (rows[m] >= 0 && v > 0 && v == grid[rows[m]][c]) ? share[rows[m]][c] : 0 with v = max(fmaf(Y2, sc2, sh2), 0):
                       a selection, exact.  The holder flag is taken from z rounded ONCE to fp32 (z32), clamped, compared in fp32.
  layer 0 recomputed   kd_l0_raw is four fmas on the 16-byte point (5 terms, 5 roundings counted as in _fp64_lidar_ref.l0_fwd), kd_affine
                       one more.  a0 = max(z0, 0) is a rounded operand: its terms are (|pt| . |w0| + |b0|) |sc0| + |sh0| and its six
                       roundings are added to the n_seq of the product it enters.  The act0 mask of G0 is taken from the same chain
                       evaluated with one fp32 rounding per fma (l0_fp32), whatever dtype the rest is evaluated in.
  xhat of layer 0      (x0 - mean0) * invstd0 with x0 itself rounded five times: its terms are (|pt| . |w0| + |b0| + |mean0|) |invstd0|
                       (NOT |xhat|: the recomputed x0 cancels), n_seq + 5 + 2.
  moments              m1[j][c] = sum_m G0[m][c] * pt[m][j] is one fma per row like s1 (n + n_part); the general kernel keeps one
                       slab row per tile and kd_slab_reduce_tall_launch sums them in double, rounding twice (+ 2); the one-kernel
                       form sums its workgroups' rows with kd_slab_reduce_launch (+ slab rows + SLAB_SPLIT).
  one-kernel forms     a workgroup owns the 32-row chunks b, b + G, ...; a thread of the vector waves adds 4 (layer 2) / 2 (layer 1)
                       rows per chunk across its chunks, then 8 / 16 row groups are added through LDS; a matrix wave keeps its dW
                       accumulators for all the workgroup's chunks (32 accumulations per chunk), then G slab rows + SLAB_SPLIT.

`mut` (a set of names) makes a function compute a WRONG reading of the contract; only tests/test_fp64_lidar_mlp_ref_host.py sets
it, to show that each of them leaves the bound."""
import torch

import _fp64_gemm_ref as R
from _fp64_conv_ref import C_BOUND, SLAB_SPLIT, U, act_in, coeffs, dyeff, folded, mask32, rnd, z32     # noqa: F401
from _fp64_gemm_ref import SPLIT_TERMS
from _fp64_tail_ref import _bound

INT_MIN = -2 ** 31
LB_CH = 32              # rows of a chunk of the one-kernel forms (LBCH)
LB_MAX_WG = 256         # lb_grid: at most one workgroup per CU
SUBNORMAL = 2.0 ** -140


def _cdiv(a, b):
    return -(-a // b)


# ---- launch layouts ------------------------------------------------------------------------------------------------------------

def l2_dgrad_layout(M, N2, K1, form, split=True):
    """kd_lidar_l2_dgrad: pro 4 / epi 2 over a reduction of N2 into K1 columns; "stream" only where the instance exists (128 -> 128)"""
    return R.gemm_layout(M, N2, K1, 4, 2, False, form if split else "tiled")


def l1_dgrad_layout(M, N1, K0):
    """kd_lidar_l1_dgrad: pro 2 / epi 3, tiled in every mode (stream_cfg has no epi 3).  The moment slab has one row per TILE
    (bm rows), summed in double by kd_slab_reduce_tall_launch: two more roundings"""
    lay = dict(R.tiled_layout(M, K0, 2))
    assert R.stream_cfg(N1, K0, 2, 3, False) is None
    tiled, waves = _cdiv(M, 128), (_cdiv(M, 32) + 8 if _cdiv(M, 32) < 2048 else 2048)
    lay.update(m1_rows=_cdiv(M, lay["bm"]), n_m1=lay["n_part"] + 2, m1_ws_bytes=max(tiled, waves) * 4 * K0 * 4)
    return lay


def fused_layout(M, layer, N=128, K=None):
    """lb_grid and the chunk ownership of lidar_l2_bwd_kernel (layer 2) / lidar_l1_bwd_kernel (layer 1): 32-row chunks,
    G = min(nchunk, 256) workgroups = slab rows, chunk c to workgroup c mod G; the longest chain is workgroup 0's"""
    K = K if K is not None else (128 if layer == 2 else 64)
    nchunk = _cdiv(M, LB_CH)
    G = min(nchunk, LB_MAX_WG)
    nit = _cdiv(nchunk, G)
    per_chunk, groups = (4, 8) if layer == 2 else (2, 16)
    ws = (G * N * K + 128) * 4 if layer == 2 else G * (N * K + 4 * K) * 4
    return dict(form="fused", grid=G, rows=G, nchunk=nchunk, nit=nit, nit_min=nchunk // G, n_part=per_chunk * nit + groups,
                n_m1=per_chunk * nit + groups + G + SLAB_SPLIT, n_red=LB_CH * nit + G + SLAB_SPLIT, ws_bytes=ws)


def slab_row_of(M, lay, device="cpu"):
    if lay["form"] == "fused":
        return (torch.arange(M, device=device) // LB_CH) % lay["grid"]
    return R.slab_row_of(M, lay, device)


# ---- layer 0 as the kernels evaluate it ------------------------------------------------------------------------------------------

def l0_fp32(pts, w0, b0):
    """kd_l0_raw: fmaf(w.w, pt.w, fmaf(w.z, pt.z, fmaf(w.y, pt.y, fmaf(w.x, pt.x, b)))), each fma the exact product and sum
    rounded once to fp32 -> [M, K0] float32"""
    p, w = pts.double(), w0.double()
    x = b0.double()[None, :].expand(pts.shape[0], -1)
    for j in range(4):
        x = (p[:, j:j + 1] * w[None, :, j] + x).float().double()
    return x.float()


def _l0(pts, w0, b0):
    return pts @ w0.t() + b0, pts.abs() @ w0.abs().t() + b0.abs()


# ---- references ------------------------------------------------------------------------------------------------------------------

def table_grad(Y2, rows, grid, share, sc2, sh2, mut=()):
    """G [M, C2]: the scatter-max gradient rebuilt from the per-cell tables.  Exact (err 0): share is selected, never rounded."""
    v = z32(Y2, sc2, sh2).clamp_min(0)
    rl = rows.long().clamp_min(0)
    hold = v == grid.float()[rl]
    if "vpos" not in mut:
        hold = hold & (v > 0)
    if "offgrid" not in mut:
        hold = hold & (rows >= 0)[:, None]
    if "tie" in mut:        # the first of two neighbouring holders of one cell loses its share
        nxt = torch.zeros_like(hold)
        nxt[:-1] = hold[1:] & (rows[1:] == rows[:-1])[:, None] & (rows[:-1] >= 0)[:, None]
        hold = hold & ~nxt
    G = torch.where(hold, share[rl], torch.zeros((), dtype=share.dtype, device=share.device))
    return {"G": (G, torch.zeros_like(G))}


def _row_sums(v, vt, w, wt, n1, n2, slab_row, nrows):
    """(s1, s2) = (sum v, sum v * w) per slab row and in total; the slab rows are added in float64 by the caller"""
    z = lambda: torch.zeros(nrows, v.shape[1], dtype=v.dtype, device=v.device)
    s1, t1 = z().index_add_(0, slab_row, v), z().index_add_(0, slab_row, vt)
    s2, t2 = z().index_add_(0, slab_row, v * w), z().index_add_(0, slab_row, vt * wt)
    e1, e2 = _bound(n1, t1), _bound(n2, t2)
    return {"s1_rows": (s1, e1), "s2_rows": (s2, e2), "s1": (s1.sum(0), e1.sum(0)), "s2": (s2.sum(0), e2.sum(0))}


def l2_backward(Y2, rows, grid, share, al, be, ga, sc2, sh2, Wt, Y1, sc1, sh1, mean1, inv1, slab_row, nrows, n_part, n_red, mut=()):
    """dy = al*G + be*Y2 + ga (kd_bwd_operand without a mask: 2 roundings), Wt [K1, N2]
    G1 = (dy . Wt^T) * relu'(fmaf(Y1, sc1, sh1))                          n_seq: 2 + N2 + SPLIT_TERMS
    s1 = sum G1, s2 = sum G1 * (Y1 - mean1) * inv1 per slab row           n_seq: n + n_part, n + 2 + n_part
    dW2 [N2, K1] = dy^T . relu(fmaf(Y1, sc1, sh1))                        n_seq: 2 + 1 + SPLIT_TERMS + n_red"""
    G = table_grad(Y2, rows, grid, share, sc2, sh2, mut)["G"][0]
    e, et, n_e = dyeff(G, Y2, al, be, ga, None, None, 0)
    n = n_e + Y2.shape[1] + SPLIT_TERMS
    v, vt = e @ Wt.t(), et @ Wt.abs().t()
    m = (z32(Y1, sc1, sh1) >= 0).to(v.dtype) if "act1_ge" in mut else mask32(Y1, sc1, sh1, 1)
    a, at = act_in(Y1, sc1, sh1, 1)
    if "lastrow" in mut:
        m = m.clone()
        m[-1] = 0
        e, et = e[:-1], et[:-1]
        a, at = a[:-1], at[:-1]
    v, vt = v * m, vt * m
    xh = (Y1 - mean1) * inv1
    out = _row_sums(v, vt, xh, xh.abs(), n + n_part, n + 2 + n_part, slab_row, nrows)
    out["G1"] = (v, _bound(n, vt))
    out["dW"] = (e.t() @ a, _bound(n_e + 1 + SPLIT_TERMS + n_red, et.t() @ at))
    return out


def l1_backward(G, Y1, al, be, ga, msc, msh, mact, Wt, pts, w0, b0, sc0, sh0, mean0, inv0, slab_row, nrows, n_part, n_m1, n_red, mut=()):
    """dy1 = al*(G*mask(fmaf(Y1, msc, msh))) + be*Y1 + ga (mact 0: no mask; 2 roundings), Wt [K0, N1], x0 = layer 0 of the point
    G0 = (dy1 . Wt^T) * relu'(fmaf(x0, sc0, sh0))                         n_seq: 2 + N1 + SPLIT_TERMS
    s1 = sum G0, s2 = sum G0 * (x0 - mean0) * inv0 per slab row           n_seq: n + n_part, n + 5 + 2 + n_part
    m1 [4, K0] = sum_m G0 * pt                                            n_seq: n + n_m1
    dW1 [N1, K0] = dy1^T . relu(fmaf(x0, sc0, sh0))                       n_seq: 2 + 5 + 1 + SPLIT_TERMS + n_red"""
    e, et, n_e = dyeff(G, Y1, al, be, ga, msc if mact else None, msh, mact)
    n = n_e + Y1.shape[1] + SPLIT_TERMS
    m = (z32(l0_fp32(pts, w0, b0), sc0, sh0) > 0).to(G.dtype)
    x0, x0t = _l0(pts, w0, b0)
    a, at = act_in(x0, sc0, sh0, 1)
    at = torch.where(at > 0, x0t * sc0.abs() + sh0.abs(), at)
    v, vt = (e @ Wt.t()) * m, (et @ Wt.abs().t()) * m
    p = pts
    if "lastrow" in mut:
        v, vt = v.clone(), vt.clone()
        v[-1], vt[-1] = 0, 0
        e, et, a, at = e[:-1], et[:-1], a[:-1], at[:-1]
    out = _row_sums(v, vt, (x0 - mean0) * inv0, (x0t + mean0.abs()) * inv0.abs(), n + n_part, n + 5 + 2 + n_part, slab_row, nrows)
    out["G0"] = (v, _bound(n, vt))
    m1 = p.t() @ v
    if "m1_coord" in mut:
        m1 = m1.clone()
        m1[2] = 0
    out["m1"] = (m1, _bound(n + n_m1, p.abs().t() @ vt))
    out["dW"] = (e.t() @ a, _bound(n_e + 5 + 1 + SPLIT_TERMS + n_red, et.t() @ at))
    return out


# ---- inputs (shared by the GPU suite and the host self-check) ----------------------------------------------------------------------

def scene(M, C2, C1, order="tail", seed=1, device="cpu"):
    """The inputs of the layer-2 backward with the cases a table rebuild can get wrong, deterministically (per device).

    rows: sorted by cell, the off-grid rows last ("tail": as kd_lidar_sort_points leaves them) or first ("head").  grid is the
    per-cell maximum of the reference's own fp32 v, so holder equality is exact by construction.  From M = 128 on:
      (a) every off-grid row carries the Y2 of row 0 of cell 0, which holds cell 0's maximum in every channel, and a rows entry
          of -1, -2 or INT_MIN: only the `rows >= 0` test keeps it from taking cell 0's share;
      (b) cells 1, 2, 3 hold 2, 3 and 40 bit-identical rows (rows 3 .. 47 of the cell-sorted order: the 40 span a chunk boundary);
      (c) cell 4 has every pre-activation below zero in channels 0 .. 3 and the pre-activations +0, -0 and negative ones in
          channel SUB_CH: maximum 0, share non-zero;
      (d) channel SUB_CH has sc2 = 1, sh2 = 0 and cell 5's maximum there is the subnormal 2^-140 (its other rows: -1, 0, -2^-140);
      (e) cell 7 and the last two cells are empty and their share rows NaN;
      (f) half of layer 1's pre-activations are below zero, channel OFF_CH entirely;
      (g) channel ZERO_CH of layer 1 has sh1 = 0 and Y1 = 0 in every seventh row: pre-activations that are exactly zero.
    Below 128 rows: random cells, an eighth of the rows off-grid, (e) - (g) only."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed((1000003 * seed + 31 * M + C2 + 7 * C1) % (2 ** 31))
    full = M >= 128
    cells = max(12, M // 9)
    n_off = max(3, M // 16) if full else M // 8
    n_in = M - n_off
    SUB_CH, OFF_CH, ZERO_CH = 5, 3, 6
    if full:
        sizes = [3, 2, 3, 40, 5, 4]
        head = torch.repeat_interleave(torch.arange(6, device=dev), torch.tensor(sizes, device=dev))
        rest = torch.randint(6, cells - 2, (n_in - sum(sizes),), generator=g, device=dev)
        rest = torch.where(rest == 7, rest + 1, rest)
        cell = torch.cat([head, rest.sort().values])
    else:
        cell = torch.randint(0, cells - 2, (n_in,), generator=g, device=dev).sort().values
    Y2, Y1 = rnd(g, M, C2), rnd(g, M, C1)
    sc2, sh2 = torch.rand(C2, generator=g, device=dev) + 0.5, rnd(g, C2) * 0.2
    sc1, sh1 = torch.rand(C1, generator=g, device=dev) + 0.5, rnd(g, C1) * 0.2
    mean1, inv1 = rnd(g, C1) * 0.1, torch.rand(C1, generator=g, device=dev) + 0.5
    al, be, ga = folded(g, C2)
    Wt = rnd(g, C1, C2) / C2 ** 0.5
    sh1[OFF_CH] = -100.0
    sh1[ZERO_CH] = 0.0
    Y1[::7, ZERO_CH] = 0.0
    if full:
        sc2[SUB_CH], sh2[SUB_CH] = 1.0, 0.0
        Y2[0] = Y2[0:3].amax(0)                                           # (a): sc2 > 0, so row 0 holds every maximum of cell 0
        Y2[3:5], Y2[5:8], Y2[8:48] = Y2[3].clone(), Y2[5].clone(), Y2[8].clone()      # (b)
        Y2[48:53, 0:4] = -(sh2[0:4] / sc2[0:4]) - 0.1 - Y2[48:53, 0:4].abs()           # (c)
        Y2[48:53, SUB_CH] = torch.tensor([0.0, -0.0, -1.0, -2.0, -3.0], device=dev)
        Y2[53:57, SUB_CH] = torch.tensor([SUBNORMAL, -1.0, 0.0, -SUBNORMAL], device=dev)   # (d)
        Y2[n_in:] = Y2[0]
    off = torch.tensor([-1, -2, INT_MIN], device=dev).repeat(_cdiv(max(n_off, 1), 3))[:n_off]
    rows = torch.cat([cell, off]).to(torch.int32)
    v = z32(Y2, sc2, sh2).clamp_min(0)
    grid = torch.zeros(cells, C2, device=dev)
    grid.index_reduce_(0, cell, v[:n_in], "amax", include_self=True)
    share = rnd(g, cells, C2)
    share = share + 0.5 * torch.where(share < 0, -torch.ones_like(share), torch.ones_like(share))
    occupied = torch.zeros(cells, dtype=torch.bool, device=dev)
    occupied[cell] = True
    share[~occupied] = float("nan")
    at = lambda i: i
    if order == "head":
        perm = torch.cat([torch.arange(n_in, M, device=dev), torch.arange(n_in, device=dev)])
        Y2, Y1, rows = Y2[perm].contiguous(), Y1[perm].contiguous(), rows[perm].contiguous()
        at = lambda i: i + n_off
    return dict(Y2=Y2, rows=rows, grid=grid, share=share, al=al, be=be, ga=ga, sc2=sc2, sh2=sh2, Wt=Wt, Y1=Y1, sc1=sc1, sh1=sh1, mean1=mean1,
                inv1=inv1, full=full, cells=cells, n_in=n_in, n_off=n_off, at=at, off_rows=slice(0, n_off) if order == "head" else slice(n_in, M),
                tie_rows=slice(at(3), at(48)), zero_rows=slice(at(48), at(53)), sub_row=at(53), sub_cell=5, SUB_CH=SUB_CH, OFF_CH=OFF_CH,
                ZERO_CH=ZERO_CH)


L2_KEYS = ("Y2", "rows", "grid", "share", "al", "be", "ga", "sc2", "sh2", "Wt", "Y1", "sc1", "sh1", "mean1", "inv1")


def l2_args(sc, dtype=None):
    """the positional arguments of l2_backward from a scene (rows stay integers)"""
    return tuple(sc[k] if k == "rows" or dtype is None else sc[k].to(dtype) for k in L2_KEYS)


def l1_inputs(M, N1, K0, seed=1, device="cpu"):
    """G, Y1 [M, N1]; points as a LiDAR frame scales them; layer 0 (w0 [K0, 4], b0); the folded BatchNorm-1 backward, its mask's
    (msc, msh); Wt [K0, N1]; (sc0, sh0, mean0, inv0).  Every 11th point is the origin and channel 2 has b0 = sh0 = 0: act0's
    pre-activation is exactly zero there."""
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed((1000003 * seed + 31 * M + N1 + 7 * K0 + 1) % (2 ** 31))
    d = dict(G=rnd(g, M, N1), Y1=rnd(g, M, N1), pts=rnd(g, M, 4) * torch.tensor([20.0, 20.0, 2.0, 0.3], device=dev),
             w0=rnd(g, K0, 4) * 0.1, b0=rnd(g, K0) * 0.1, Wt=rnd(g, K0, N1) / N1 ** 0.5)
    d["al"], d["be"], d["ga"] = folded(g, N1)
    d["msc"], d["msh"] = coeffs(g, N1, 1)[:2]
    d["sc0"], d["sh0"], d["mean0"], d["inv0"] = coeffs(g, K0, 1)
    d["sh0"] = d["sh0"] * 1.5
    d["pts"][::11] = 0.0
    d["b0"][2], d["sh0"][2] = 0.0, 0.0
    return d


def l1_args(d, mact, dtype=None):
    c = lambda t: t if dtype is None else t.to(dtype)
    return (c(d["G"]), c(d["Y1"]), c(d["al"]), c(d["be"]), c(d["ga"]), c(d["msc"]), c(d["msh"]), mact, c(d["Wt"]), c(d["pts"]), c(d["w0"]),
            c(d["b0"]), c(d["sc0"]), c(d["sh0"]), c(d["mean0"]), c(d["inv0"]))
