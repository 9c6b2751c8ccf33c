"""References for the LiDAR branch kernels of csrc/kd_lidar.hip (binning, compaction, scatter-max forward / backward, layer 0)
and for the two GEMM forms that only the LiDAR branch uses (layer 1 over the recomputed layer 0, layer 2 with the scatter-max
epilogue).  Plain numpy / torch; nothing here imports the library under test.

Three kinds of statement, and no other tolerance:
  * EXACT (bit equality): the cell of a point (every step of the binning is one IEEE fp32 operation), the activated value
    clamp(fma(y, sc, sh)) (float64 evaluation rounded once, with the count of elements where that could differ from the
    fused operation), the grid (a maximum of fp32 values) and the per-point gradient dout / holders (one correctly rounded
    fp32 division);
  * BOUNDED: sums and layer 0, {name: (value, err)} with err = C_BOUND * n_seq * U * sum|t_i| exactly as in _fp64_tail_ref.py --
    evaluated in the dtype of the inputs, so that a plain fp32 evaluation can be held against the same bound;
  * float64 values for the GEMM forms, compared under the GEMM family's own 2e-5 / 1e-4 rules by the caller."""
import numpy as np
import torch

from _fp64_tail_ref import C_BOUND, SLAB_SPLIT, U  # noqa: F401  (re-exported: the callers take all three from here)

RELU, RELU6 = 1, 2
F32 = np.float32


def _bound(n_seq, terms):
    return C_BOUND * n_seq * U * terms


# ---- launch layout ------------------------------------------------------------------------------------------------------

def cg_layout(rows, C, max_blocks=2048):
    """mirror of kd_cg_layout -> (groups, slots, grid)"""
    groups = C // 4
    slots = max(1, 256 // groups)
    grid = max(1, min(-(-rows // slots), max_blocks))
    return groups, slots, grid


def cg_iters(rows, C, max_blocks=2048):
    """rows one (block, slot) walks: the grid-stride iterations"""
    _, slots, grid = cg_layout(rows, C, max_blocks)
    return -(-rows // (grid * slots))


# ---- comparisons (shared by the GPU tests and by the host test that feeds them a deliberately wrong reference) -------------

def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def check_exact(what, got, want):
    """bit equality of two arrays of the same 4- or 8-byte dtype (NaN == NaN by bits, +0 != -0)"""
    got, want = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    view = np.int32 if got.dtype.itemsize == 4 else (np.int64 if got.dtype.itemsize == 8 else got.dtype)
    bad = got.view(view) != want.view(view)
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ; first at flat index {i}: got {got.reshape(-1)[i]!r}, "
                             f"reference {want.reshape(-1)[i]!r}")


def check_bound(what, got, ref):
    """|got - value| <= err element-wise; an unwritten (NaN) element fails"""
    val, err = ref
    got = got.detach().double().reshape(val.shape).to(val.device)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements never written"
    d = (got - val.double()).abs()
    bad = d > err.double()
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        r = (d / err.double().clamp_min(1e-300)).max().item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {val.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                             f"got {got.reshape(-1)[i].item():.9g}, reference {val.reshape(-1)[i].item():.9g}, "
                             f"bound {err.reshape(-1)[i].item():.3g}")


# ---- binning (lidar_encoder.py:46-55, 69-71) ---------------------------------------------------------------------------

def bev_cells(pts, H, W, x0, x1, y0, y1, swap=None):
    """pts [P, >=2] fp32 -> int64 [P]: iy*W + ix, or -1 for a point outside the range (NaN included).  fp32 arithmetic in the
    reference model's order: xn = (x - x0) / (x1 - x0), valid iff 0 <= xn <= 1 (same for y), ix = trunc(xn * (W-1)) clamped
    to [0, W-1].  swap: a deliberately wrong implementation, for the host test that shows which grids make it visible --
    "factors": x scaled by H-1 and y by W-1; "ranges": x normalised with the y range and y with the x range."""
    p = _np(pts).astype(F32, copy=False)
    fw, fh = (F32(H - 1), F32(W - 1)) if swap == "factors" else (F32(W - 1), F32(H - 1))
    if swap == "ranges":
        x0, x1, y0, y1 = y0, y1, x0, x1
    with np.errstate(all="ignore"):
        xn = (p[:, 0] - F32(x0)) / (F32(x1) - F32(x0))
        yn = (p[:, 1] - F32(y0)) / (F32(y1) - F32(y0))
        valid = (xn >= 0) & (xn <= 1) & (yn >= 0) & (yn <= 1)
        fx = np.where(valid, xn * fw, F32(0))
        fy = np.where(valid, yn * fh, F32(0))
    assert fx.dtype == F32 and fy.dtype == F32
    ix = np.clip(np.trunc(fx).astype(np.int64), 0, W - 1)
    iy = np.clip(np.trunc(fy).astype(np.int64), 0, H - 1)
    return np.where(valid, iy * W + ix, -1)


def grid_rows(pts, B, N, H, W, rng):
    """row of the [B*H*W, C] grid for each of the B*N points (frame * H*W + cell), -1 for an out-of-range point"""
    cell = bev_cells(pts, H, W, *rng)
    return np.where(cell >= 0, (np.arange(B * N) // N) * (H * W) + cell, -1)


def edge_points(H, W, x0, x1, y0, y1):
    """the constructed edge set of the binning test, fp32 [n, 4]: both range ends and their fp32 neighbours, the fp32 values
    nearest every interior cell boundary k / (W-1) with one ulp on each side, +-0, denormals, +-1e30, +-Inf, NaN -- each put
    into x (y random in range) and into y (x random in range)."""
    def axis(lo, hi, n):
        lo32, hi32 = F32(lo), F32(hi)
        v = [lo32, hi32]
        for e in (lo32, hi32):
            v += [np.nextafter(e, F32(-np.inf)), np.nextafter(e, F32(np.inf))]
        if n > 1:
            k = np.arange(1, n - 1, dtype=np.float64)
            b = (lo + (hi - lo) * k / (n - 1)).astype(F32)
            v += list(b) + list(np.nextafter(b, F32(-np.inf))) + list(np.nextafter(b, F32(np.inf)))
        v += [F32(0.0), F32(-0.0), F32(1e-45), F32(-1e-45), F32(1e-39), F32(-1e-39), F32(1e30), F32(-1e30), F32(np.inf), F32(-np.inf),
              F32(np.nan)]
        return np.array(v, dtype=F32)
    rs = np.random.RandomState(H * 1000 + W)
    ex, ey = axis(x0, x1, W), axis(y0, y1, H)
    a = np.zeros((len(ex) + len(ey), 4), dtype=F32)
    a[:len(ex), 0] = ex
    a[:len(ex), 1] = rs.uniform(y0, y1, len(ex)).astype(F32)
    a[len(ex):, 0] = rs.uniform(x0, x1, len(ey)).astype(F32)
    a[len(ex):, 1] = ey
    a[:, 2:] = rs.randn(len(a), 2).astype(F32)
    return a


def binning_points(H, W, rng, n_random=20000):
    """the input of the binning test: n_random points around the range (a quarter of them outside) followed by edge_points"""
    x0, x1, y0, y1 = rng
    rs = np.random.RandomState(7 * H + W + int(x1))
    r = rs.randn(n_random, 4).astype(F32)
    r[:, 0] = rs.uniform(x0 - 0.15 * (x1 - x0), x1 + 0.15 * (x1 - x0), n_random).astype(F32)
    r[:, 1] = rs.uniform(y0 - 0.15 * (y1 - y0), y1 + 0.15 * (y1 - y0), n_random).astype(F32)
    return np.concatenate([r, edge_points(H, W, x0, x1, y0, y1)], 0)


def swapped_axis_fraction(pts, H, W, rng, swap):
    """fraction of the points valid under the true binning whose cell a swapped implementation (see bev_cells) gets wrong: what
    a test grid / range must make visible.  "factors" shows on a non-square grid only, "ranges" on an asymmetric range only."""
    cell = bev_cells(pts, H, W, *rng)
    sw = bev_cells(pts, H, W, *rng, swap=swap)
    valid = cell >= 0
    return float((cell[valid] != sw[valid]).mean())


# ---- activation ------------------------------------------------------------------------------------------------------------

def activated(y, sc, sh, act):
    """-> (v fp32 = clamp(fma(y, sc, sh)) as the kernels decide with it, count).  The product of two fp32 numbers is exact in
    float64; the sum is rounded to float64 and then once more to fp32.  The two roundings can differ from the single one of the
    fused operation only where the float64 sum is INEXACT and sits on an fp32 midpoint (low 29 mantissa bits 0x10000000) -- an
    exact sum on a midpoint is rounded once, like the fused operation (it happens whenever sc has a short mantissa) -- or lies
    below the fp32 normal range, where the rounding position moves.  `count` is the number of such elements; callers require 0."""
    a, b = y.double() * sc.double(), sh.double().expand(y.shape)
    z = a + b
    t = z - a
    inexact = ((a - (z - t)) + (b - t)) != 0                  # the rounding error of a + b, itself computed exactly (TwoSum)
    bits = z.contiguous().view(torch.int64)
    risky = (((bits & 0x1FFFFFFF) == 0x10000000) & inexact) | ((z != 0) & (z.abs() < 2.0 ** -126))
    v = z.float().clamp_min(0)
    if act == RELU6:
        v = v.clamp_max(6)
    else:
        assert act == RELU
    return v, int(risky.sum())


# ---- scatter-max -----------------------------------------------------------------------------------------------------------

def _segments(rows):
    rows = np.asarray(rows, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    order = order[rows[order] >= 0]
    r = rows[order]
    first = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]])) if len(r) else np.zeros(0, np.int64)
    return order, first, r[first] if len(r) else np.zeros(0, np.int64)


def scatter_max(rows, v, ncells):
    """rows int64 [P] (grid row or -1), v fp32 [P, C] >= 0 -> (grid fp32 [ncells, C]: per-row maximum, 0 for an empty row;
    holder bool [P, C]: v > 0 and v == the maximum of its row; counts int64 [ncells, C]: holders per (row, channel)).
    Exact: a maximum of fp32 values has no rounding."""
    v = np.ascontiguousarray(_np(v))
    assert v.dtype == F32
    rows = np.asarray(rows, dtype=np.int64)
    order, first, ids = _segments(rows)
    grid = np.zeros((ncells, v.shape[1]), dtype=F32)
    counts = np.zeros((ncells, v.shape[1]), dtype=np.int64)
    holder = np.zeros(v.shape, dtype=bool)
    if len(order):
        grid[ids] = np.maximum(np.maximum.reduceat(v[order], first, axis=0), F32(0)) + F32(0)      # (+0: a -0 never reaches the grid)
        valid = rows >= 0
        holder[valid] = (v[valid] > 0) & (v[valid] == grid[rows[valid]])
        counts[ids] = np.add.reduceat(holder[order].astype(np.int64), first, axis=0)
    return grid, holder, counts


def scatter_max_grad(rows, v, holder, counts, dout, y, mean, invstd, act, n_seq, count_offset=0):
    """ATen's backward of amax (even split among the holders), then of the activation:
         G = holder ? fp32(dout[row]) / fp32(count[row]) : 0   (numpy float32 division: correctly rounded),
       and for ReLU6 G = 0 where the value is saturated (hardtanh_backward passes 0 < z < 6 only; v < 6 iff z < 6).
    -> (G fp32 [P, C], {"s1": sum G, "s2": sum G * xhat} over the points, float64, each with its bound; xhat = (y - mean) * invstd
    costs the kernel a subtraction, a product and the fused multiply-add: 3 roundings on top of n_seq).
    count_offset: added to every holder count -- only the host test that shows a wrong split being caught sets it."""
    v, dout = _np(v), _np(dout)
    rows = np.asarray(rows, dtype=np.int64)
    G = np.zeros(v.shape, dtype=F32)
    valid = rows >= 0
    r = rows[valid]
    with np.errstate(all="ignore"):
        share = dout[r].astype(F32) / (counts[r] + count_offset).astype(F32)
    g = np.where(holder[valid], share, F32(0))
    if act == RELU6:
        g = np.where(v[valid] < F32(6), g, F32(0))
    G[valid] = g
    assert G.dtype == F32
    Gd = torch.from_numpy(G).double()
    xh = (torch.as_tensor(_np(y)).double() - torch.as_tensor(_np(mean)).double()) * torch.as_tensor(_np(invstd)).double()
    sums = {"s1": (Gd.sum(0), _bound(n_seq, Gd.abs().sum(0))),
            "s2": ((Gd * xh).sum(0), _bound(n_seq + 3, (Gd * xh).abs().sum(0)))}
    return G, sums


# ---- layer 0: Conv1d(4 -> C, k = 1, bias) ------------------------------------------------------------------------------------

def _l0(pts, w, b):
    y = pts @ w.t()
    ya = pts.abs() @ w.abs().t()
    if b is not None:
        y, ya = y + b, ya + b.abs()
    return y, ya


def l0_fwd(pts, w, b, n_part):
    """pts [P, 4], w [C, 4], b [C] or None -> y [P, C] (five terms per element), s1 = sum_p y, s2 = sum_p y^2 per channel
    (n_part: iterations per slot + slots of the partial rows; y^2 carries twice y's relative error plus the product)."""
    y, ya = _l0(pts, w, b)
    return {"y": (y, _bound(5, ya)),
            "s1": (y.sum(0), _bound(5 + n_part, ya.sum(0))),
            "s2": ((y * y).sum(0), _bound(11 + n_part, (ya * ya).sum(0)))}


def l0_bwd(D, Y, w, b, al, be, ga, pts, n_red, drop_last_row=False):
    """g = al*D + be*y + ga per (point, channel); dw [C, 4] = sum_p g * pt, db [C] = sum_p g.  D None: zeros; Y None: y
    recomputed from the point (its five roundings enter g's bound).  n_red: the sequential chain of the row reduction.
    drop_last_row: leaves out the last point -- only the host test that shows a dropped tail row being caught sets it."""
    if Y is None:
        y, ya = _l0(pts, w, b)
        n_g = 3 + 5
    else:
        y, ya, n_g = Y, Y.abs(), 3
    g, gabs = be * y + ga, (be * ya).abs() + ga.abs()
    if D is not None:
        g, gabs = g + al * D, gabs + (al * D).abs()
    if drop_last_row:
        g, gabs, pts = g[:-1], gabs[:-1], pts[:-1]
    return {"dw": (g.t() @ pts, _bound(n_g + 1 + n_red, gabs.t() @ pts.abs())),
            "db": (g.sum(0), _bound(n_g + n_red, gabs.sum(0)))}


# ---- the two GEMM forms of the LiDAR branch, float64 -----------------------------------------------------------------------

def point_mlp_l1(pts, w0, b0, sc0, sh0, W1, bias1):
    """layer 1 over ReLU(bn0(layer 0)) recomputed from the point: [M, N] float64"""
    d = lambda t: None if t is None else t.double()
    a = (_l0(d(pts), d(w0), d(b0))[0] * d(sc0) + d(sh0)).clamp_min(0)
    out = a @ d(W1).t()
    return out if bias1 is None else out + d(bias1)


def l2_scatter(A, sc1, sh1, W2, bias2, sc2, sh2, rows, ncells, m):
    """grid [ncells, N] float64: scatter-max over the first m rows of ReLU(bn2(ReLU(bn1(A)) . W2^T + bias2)); -> (grid, occupied)"""
    d = lambda t: None if t is None else t.double()
    a = (d(A) * d(sc1) + d(sh1)).clamp_min(0)
    y = a @ d(W2).t()
    if bias2 is not None:
        y = y + d(bias2)
    v = (y * d(sc2) + d(sh2)).clamp_min(0)[:m]
    idx = torch.as_tensor(np.asarray(rows)[:m], dtype=torch.int64, device=v.device)
    grid = torch.zeros(ncells, v.shape[1], dtype=torch.float64, device=v.device)
    grid.scatter_reduce_(0, idx[:, None].expand(-1, v.shape[1]), v, "amax", include_self=True)        # v >= 0: the zeros are neutral
    occupied = torch.zeros(ncells, dtype=torch.bool, device=v.device)
    occupied[idx] = True
    return grid, occupied


# ---- the scenes of the scatter tests (shared with the host test, which requires the midpoint count 0 for each) -------------

RNG = (-50.0, 50.0, -50.0, 50.0)
# B, N, H, W, sigma, pad, dup, nan, feature scale: the recipes of tests/test_gpu_lidar_holder_tables.py (dup: exact ties;
# pad, row257, sigma1: cells of more than 256 points; nan: NaN / Inf coordinates), two of them on rectangular grids, and
# `sat`, whose features are scaled so that ReLU6 saturates
SCENES = {
    "dup": (2, 6000, 16, 16, 40.0, 0, 300, 0, 1.0),
    "dup_rect": (2, 6000, 9, 17, 40.0, 0, 300, 0, 1.0),
    "pad": (2, 3000, 16, 16, 40.0, 1500, 100, 0, 1.0),
    "row257": (1, 700, 8, 8, 12.0, 257, 0, 0, 1.0),
    "sigma1": (2, 9000, 32, 32, 1.0, 0, 0, 0, 1.0),
    "nan": (3, 5000, 64, 64, 40.0, 0, 200, 40, 1.0),
    "sat": (2, 4000, 17, 9, 40.0, 0, 150, 0, 6.0),
}
SCENE_WIDTHS = (32, 64, 96, 128, 256)


def scene(name, C):
    """-> B, N, H, W and CPU tensors pts [B*N, 4], y [B*N, C], sc, sh, mean, invstd [C]"""
    B, N, H, W, sigma, pad, dup, nan, scale = SCENES[name]
    g = torch.Generator().manual_seed(1000 * sorted(SCENES).index(name) + C)
    pts = torch.randn(B, N, 4, generator=g) * torch.tensor([sigma, sigma, 2.0, 1.0])
    if pad:
        pts[:, N - pad:] = 0.0
    y = torch.randn(B * N, C, generator=g) * scale
    if dup:
        src = torch.randint(0, N - pad - dup, (dup,), generator=g)
        pts[:, N - pad - dup:N - pad] = pts[:, src]
        yv = y.view(B, N, C)
        yv[:, N - pad - dup:N - pad] = yv[:, src]
    if nan:
        pts[:, :nan, 0] = float("nan")
        pts[:, nan:2 * nan, 1] = float("inf")
    sc = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g) * 0.2
    mean = torch.randn(C, generator=g) * 0.1
    invstd = torch.rand(C, generator=g) + 0.5
    return B, N, H, W, pts.view(B * N, 4).contiguous(), y, sc, sh, mean, invstd


def sparse_dout(counts_per_row, C, seed):
    """dout [ncells, C] that is nonzero only in the first and the last occupied row and in one empty row (where the scene
    leaves one empty: the dense 16 x 16 scenes do not)"""
    ncells = len(counts_per_row)
    occ = np.flatnonzero(counts_per_row > 0)
    empty = np.flatnonzero(counts_per_row == 0)
    assert len(occ) >= 2
    d = torch.zeros(ncells, C)
    sel = [int(occ[0]), int(occ[-1])] + ([int(empty[len(empty) // 2])] if len(empty) else [])
    d[sel] = torch.randn(len(sel), C, generator=torch.Generator().manual_seed(seed))
    return d
