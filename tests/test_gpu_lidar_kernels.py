"""The LiDAR branch kernels of csrc/kd_lidar.hip and the two GEMM forms only that branch uses, called directly through the C ABI
and compared with the independent references of tests/_fp64_lidar_ref.py: the binning, the compaction, the atomic scatter-max
pair (the root every segmented / holder-table test compares with), the shipped sorted training path, layer 0 and its backward
in all pointer modes, layer 1 over the recomputed layer 0 and layer 2 with the scatter-max epilogue.

Only three kinds of comparison appear: bit equality (cells, grid, per-point gradient), the bound C_BOUND * n_seq * 2^-24 * sum|t_i|
(sums, layer 0) and the GEMM family's 2e-5 / 1e-4 rules of test_gpu_gemm_shapes.py.  Every float output starts as NaN with a
sentinel guard tail, every integer output as a sentinel value.

The scatter-max BACKWARD under ReLU6 is refused by the library (a maximum saturated at 6.0 has derivative 0 in ATen, the holder
split of the kernels would hand it dout / holders): those cases assert the refusal; the forward ReLU6 cases compare as usual."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _fp64_lidar_ref as R

pytestmark = pytest.mark.gpu

GUARD, SENT, ISENT = 64, -1.25e30, -77
NAN = float("nan")
TOL, STAT_TOL = 2e-5, 1e-4              # the GEMM rules of test_gpu_gemm_shapes.py
GRIDS = [(16, 16), (33, 17), (17, 33), (1, 40), (40, 1), (128, 128), (192, 192)]
RANGES = [(-50.0, 50.0, -50.0, 50.0), (-20.0, 80.0, -5.0, 3.0)]
CAP = 2048                              # launch cap of the layer-0 kernels (kd_cg_layout's default)


def _lib():
    from kdrt.lib import KDError, lib
    return lib, KDError


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Buf:
    """an output of n elements (float: NaN-filled, integer: ISENT-filled) followed by a guard of sentinels"""

    def __init__(self, *shape, dtype=torch.float32):
        n = math.prod(shape)
        self.n, self.flt = n, dtype.is_floating_point
        fill = NAN if self.flt else (-ISENT if dtype == torch.uint8 else ISENT)
        self.buf = torch.full((n + GUARD,), fill, device="cuda", dtype=dtype)
        self.sent = SENT if self.flt else fill - 1
        self.buf[n:] = self.sent
        self.t = self.buf[:n].view(*shape)

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == self.sent).all()), f"{what}: written past its end"


def _guards(**bufs):
    for n, b in bufs.items():
        b.guard_ok(n)


def _cuda(*ts):
    return [None if t is None else (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).cuda().contiguous() for t in ts]


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).cuda()


# ---- a. binning ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", RANGES, ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("H,W", GRIDS)
def test_bev_index_is_the_reference_cell(H, W, rng):
    lib, _ = _lib()
    pts = R.binning_points(H, W, rng)
    want = R.bev_cells(pts, H, W, *rng)
    # the grid / range of this case makes an exchanged axis visible (the same counts as in test_fp64_lidar_ref_host.py)
    if H != W:
        assert R.swapped_axis_fraction(pts, H, W, rng, "factors") > 0.10
    if rng[:2] != rng[2:]:
        assert R.swapped_axis_fraction(pts, H, W, rng, "ranges") > 0.10
    n = len(pts)
    cell, d_pts = Buf(n, dtype=torch.int32), _cuda(pts)[0]
    lib.call("kd_lidar_bev_index", P(d_pts), P(cell.t), n, H, W, *rng, None)
    torch.cuda.synchronize()
    R.check_exact("cell", cell.t, want.astype(np.int32))
    cell.guard_ok("cell")


# ---- b. compaction ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N", [(1, 1), (1, 63), (2, 512), (1, 1025), (1, 3 * 1024 + 7), (4, 5000)], ids=lambda v: str(v))
def test_compact_keeps_exactly_the_valid_points(B, N):
    lib, _ = _lib()
    H, W, rng = 33, 17, RANGES[1]
    n = B * N
    pts = R.binning_points(H, W, rng, n_random=max(n, 200))
    pts = pts[np.random.RandomState(n).permutation(len(pts))[:n]] if n > 1 else np.array([[3.0, 1.0, 0.5, 0.1]], dtype=np.float32)
    rows = R.grid_rows(pts, B, N, H, W, rng)
    valid = rows >= 0
    nv = int(valid.sum())
    if n >= 63:
        assert 0 < nv < n and not np.isfinite(pts[:, :2]).all()
    d_pts = _cuda(pts)[0]
    out_pts, out_row, counter = Buf(n, 4), Buf(n, dtype=torch.int32), Buf(1, dtype=torch.int32)
    lib.call("kd_lidar_compact", P(d_pts), P(out_pts.t), P(out_row.t), P(counter.t), B, N, H, W, *rng, None)
    torch.cuda.synchronize()
    assert int(counter.t.item()) == nv
    # the (point bits, row) pairs, as sorted multisets
    got = np.concatenate([out_pts.t[:nv].cpu().numpy().view(np.int32), out_row.t[:nv].cpu().numpy()[:, None]], 1)
    want = np.concatenate([pts[valid].view(np.int32), rows[valid].astype(np.int32)[:, None]], 1)
    key = lambda a: a[np.lexsort(a.T[::-1])]
    R.check_exact("compacted (point, row) pairs", key(got), key(want))
    assert bool(torch.isnan(out_pts.t[nv:]).all()) and bool((out_row.t[nv:] == ISENT).all()), "written beyond the count"
    _guards(out_pts=out_pts, out_row=out_row, counter=counter)


# ---- c. the atomic scatter pair --------------------------------------------------------------------------------------------

class _Scene:
    """one scene of R.SCENES at width C with its reference: rows, activated values, grid, holders per activation"""

    def __init__(self, name, C):
        self.B, self.N, self.H, self.W, pts, y, sc, sh, mean, inv = R.scene(name, C)
        self.C, self.Pn, self.ncells = C, self.B * self.N, self.B * self.H * self.W
        self.cpu = (pts, y, sc, sh, mean, inv)
        self.pts, self.y, self.sc, self.sh, self.mean, self.inv = _cuda(pts, y, sc, sh, mean, inv)
        self.rows = R.grid_rows(pts, self.B, self.N, self.H, self.W, R.RNG)
        self.per_row = np.bincount(self.rows[self.rows >= 0], minlength=self.ncells)
        self.ref = {}
        for act in (R.RELU, R.RELU6):
            v, risky = R.activated(y, sc, sh, act)
            assert risky == 0                                    # the exact prediction holds for this seed
            self.ref[act] = (v, *R.scatter_max(self.rows, v, self.ncells))

    def grad(self, act, dout, n_seq):
        v, _, holder, counts = self.ref[act]
        pts, y, sc, sh, mean, inv = self.cpu
        return R.scatter_max_grad(self.rows, v, holder, counts, dout, y, mean, inv, act, n_seq)


@pytest.mark.parametrize("C", R.SCENE_WIDTHS)
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_atomic_scatter_max_pair(name, C):
    lib, KDError = _lib()
    s = _Scene(name, C)
    geo = (s.B, s.N, C, s.H, s.W, *R.RNG)
    _, slots, grid_blocks = R.cg_layout(s.Pn, C, 4096)
    rows_p = lib.kd_lidar_scatter_stat_rows(s.Pn, C)
    nbytes = lib.kd_lidar_scatter_bwd_ws_bytes(s.B, s.H, s.W, C)
    assert rows_p == grid_blocks and nbytes == s.ncells * C * 4
    n_seq = R.cg_iters(s.Pn, C, 4096) + slots + rows_p
    for act in (R.RELU, R.RELU6):
        v, gref, holder, counts = s.ref[act]
        if name == "sat" and act == R.RELU6:
            assert (gref[s.per_row > 0] == 6.0).mean() > 0.20
        grid = Buf(s.ncells, C)
        lib.call("kd_lidar_scatter_max_fwd", P(s.pts), P(s.y), P(s.sc), P(s.sh), act, P(grid.t), *geo, None)
        torch.cuda.synchronize()
        R.check_exact(f"grid (act {act})", grid.t, gref)
        grid.guard_ok("grid")
        douts = [torch.randn(s.ncells, C, generator=torch.Generator().manual_seed(5)), R.sparse_dout(s.per_row, C, 6)]
        for k, dout in enumerate(douts):
            G, part, ws, d_dout = Buf(s.Pn, C), Buf(rows_p, 2, C), Buf(nbytes // 4), dout.cuda()
            args = (P(s.pts), P(s.y), P(s.sc), P(s.sh), act, P(grid.t), P(d_dout), P(s.mean), P(s.inv), P(G.t), P(part.t), *geo,
                    P(ws.t), nbytes, None)
            if act == R.RELU6:
                with pytest.raises(KDError, match="ReLU6 is not supported"):
                    lib.call("kd_lidar_scatter_max_bwd", *args)
                break
            lib.call("kd_lidar_scatter_max_bwd", *args)
            torch.cuda.synchronize()
            Gref, sums = s.grad(act, dout, n_seq)
            R.check_exact(f"G (dout {k})", G.t, Gref)
            assert bool((G.t[torch.from_numpy(s.rows < 0).cuda()] == 0).all()), "rows of invalid points"
            ps = part.t.double().sum(0).cpu()
            R.check_bound(f"sum G (dout {k})", ps[0], sums["s1"])
            R.check_bound(f"sum G*xhat (dout {k})", ps[1], sums["s2"])
            _guards(G=G, partial=part, ws=ws)


@pytest.mark.parametrize("act", [R.RELU, R.RELU6], ids=["relu", "relu6"])
@pytest.mark.parametrize("name,C", [("dup_rect", 96), ("nan", 128), ("sat", 32), ("pad", 256), ("sigma1", 64)])
def test_scatter_max_over_prebinned_rows(name, C, act):
    lib, _ = _lib()
    s = _Scene(name, C)
    pts, y, sc, sh, _, _ = s.cpu
    valid = s.rows >= 0
    yv, rv = y[torch.from_numpy(valid)].contiguous(), s.rows[valid]
    n = len(rv)
    d_y, d_rows = yv.cuda(), _i32(rv)
    v = R.activated(yv, sc, sh, act)[0]
    for p in (None, n - n // 3, 1, 0):
        m = n if p is None else p
        want = R.scatter_max(rv[:m], v[:m], s.ncells)[0]
        p_dev = None if p is None else torch.tensor([p], device="cuda", dtype=torch.int32)
        grid = Buf(s.ncells, C)
        lib.call("kd_lidar_scatter_max_idx_fwd", P(d_y), P(s.sc), P(s.sh), act, P(d_rows), P(grid.t), n, C, s.ncells, P(p_dev), None)
        torch.cuda.synchronize()
        R.check_exact(f"grid (p_dev {p})", grid.t, want)
        grid.guard_ok("grid")
    grid = Buf(s.ncells, C)                                      # P = 0: a zeroed grid, no launch
    lib.call("kd_lidar_scatter_max_idx_fwd", P(d_y), P(s.sc), P(s.sh), act, P(d_rows), P(grid.t), 0, C, s.ncells, None, None)
    torch.cuda.synchronize()
    R.check_exact("grid (P = 0)", grid.t, np.zeros((s.ncells, C), np.float32))
    grid.guard_ok("grid")


# ---- d. the shipped training path --------------------------------------------------------------------------------------------

def _seg_grid(ncells):
    return min(-(-ncells // 4), 4096)


def _seg_long_grid(Pn):
    return min(-(-Pn // 256), 1024)


def _seg_chain(per_row, Pn, long_len):
    """longest sequential fp32 chain of a (sum G, sum G*xhat) entry of the segmented kernels: a wave adds the points of all its
    rows (row r belongs to wave r mod 4*grid) -- or, for rows longer than long_len, of its 64-point chunks -- one after the
    other; then the block's 4 waves are added"""
    ncells = len(per_row)
    nw = _seg_grid(ncells) * 4
    short = per_row if long_len == 0 else np.where(per_row <= long_len, per_row, 0)
    chain = np.bincount(np.arange(ncells) % nw, weights=short).max()
    if long_len and (per_row > long_len).any():
        chunks = -(-int(per_row.sum()) // 64)
        chain = max(chain, -(-chunks // (_seg_long_grid(Pn) * 4)) * 64)
    return int(chain) + 4


@pytest.mark.parametrize("C", (64, 128, 256))
@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_sorted_training_path(name, C):
    """kd_lidar_sort_points -> kd_lidar_seg_hold_fwd -> kd_lidar_seg_hold_bwd (what training runs) and kd_lidar_seg_max_fwd / _bwd
    in the perm form, against the same reference as the atomic pair"""
    lib, KDError = _lib()
    s = _Scene(name, C)
    act = R.RELU
    v, gref, holder, counts = s.ref[act]
    B, N, H, W, Pn, ncells = s.B, s.N, s.H, s.W, s.Pn, s.ncells
    spts, srow, start, perm = Buf(Pn, 4), Buf(Pn, dtype=torch.int32), Buf(ncells + 1, dtype=torch.int32), Buf(Pn, dtype=torch.int32)
    nb = lib.kd_lidar_sort_points_ws_bytes(B, N, H, W)
    ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
    lib.call("kd_lidar_sort_points", P(s.pts), B, N, H, W, *R.RNG, P(spts.t), P(srow.t), P(start.t), P(perm.t), P(ws), nb, None)
    torch.cuda.synchronize()
    key = np.where(s.rows >= 0, s.rows, ncells + np.arange(Pn) // N)
    order = np.argsort(key, kind="stable")
    R.check_exact("perm", perm.t, order.astype(np.int32))
    R.check_exact("row_sorted", srow.t, s.rows[order].astype(np.int32))
    R.check_exact("seg_start", start.t, np.concatenate([[0], np.cumsum(s.per_row)]).astype(np.int32))
    _guards(spts=spts, srow=srow, start=start, perm=perm)
    ys = s.y[perm.t.long()].contiguous()
    dout = torch.randn(ncells, C, generator=torch.Generator().manual_seed(5))
    d_dout = dout.cuda()
    rows_t = lib.kd_lidar_seg_share_stat_rows(ncells, Pn)
    assert rows_t == _seg_grid(ncells) + _seg_long_grid(Pn) and lib.kd_lidar_seg_stat_rows(ncells) == _seg_grid(ncells)

    # holder tables
    grid, rawmax, holders = Buf(ncells, C), Buf(ncells, C), Buf(ncells, C, dtype=torch.uint8)
    lib.call("kd_lidar_seg_hold_fwd", P(ys), P(s.sc), P(s.sh), act, P(start.t), P(srow.t), P(grid.t), P(rawmax.t), P(holders.t), Pn,
             ncells, C, None)
    share, cnt, part = Buf(ncells, C), Buf(ncells, C), Buf(rows_t, 2, C)
    hb = (P(ys), P(s.sc), P(s.sh), act, P(grid.t), P(rawmax.t), P(holders.t), P(d_dout), P(s.mean), P(s.inv), P(start.t), P(srow.t),
          P(share.t), P(cnt.t), P(part.t), Pn, ncells, C, None)
    lib.call("kd_lidar_seg_hold_bwd", *hb)
    torch.cuda.synchronize()
    R.check_exact("grid (holder tables)", grid.t, gref)
    Gref, sums = s.grad(act, dout, _seg_chain(s.per_row, Pn, 256) + rows_t)
    # the rule documented above kd_lidar_l2_dgrad: G[m][c] = (rows[m] >= 0 && v > 0 && v == grid[rows[m]][c]) ? share[rows[m]][c] : 0
    vs, rs = v[torch.from_numpy(order)].cuda(), torch.from_numpy(s.rows[order]).cuda()
    ok = rs >= 0
    G = torch.zeros(Pn, C, device="cuda")
    G[ok] = torch.where((vs[ok] > 0) & (vs[ok] == grid.t[rs[ok]]), share.t[rs[ok]], torch.zeros((), device="cuda"))
    R.check_exact("G rebuilt from (row_sorted, grid, share)", G, Gref[order])
    ps = part.t.double().sum(0).cpu()
    R.check_bound("sum G (holder tables)", ps[0], sums["s1"])
    R.check_bound("sum G*xhat (holder tables)", ps[1], sums["s2"])
    _guards(grid=grid, rawmax=rawmax, holders=holders, share=share, cnt=cnt, partial=part)
    with pytest.raises(KDError, match="ReLU6 is not supported"):
        lib.call("kd_lidar_seg_hold_bwd", *hb[:3], R.RELU6, *hb[4:])

    # perm form on the unsorted features
    rows_s = _seg_grid(ncells)
    grid2, G2, part2 = Buf(ncells, C), Buf(Pn, C), Buf(rows_s, 2, C)
    d_rows = _i32(s.rows)
    lib.call("kd_lidar_seg_max_fwd", P(s.y), P(s.sc), P(s.sh), act, P(start.t), P(perm.t), None, P(grid2.t), Pn, ncells, C, None)
    mb = (P(s.y), P(s.sc), P(s.sh), act, P(grid2.t), P(d_dout), P(s.mean), P(s.inv), P(start.t), P(perm.t), P(d_rows), P(G2.t), P(part2.t),
          Pn, ncells, C, None)
    lib.call("kd_lidar_seg_max_bwd", *mb)
    torch.cuda.synchronize()
    R.check_exact("grid (perm form)", grid2.t, gref)
    R.check_exact("G (perm form)", G2.t, Gref)
    _, sums2 = s.grad(act, dout, _seg_chain(s.per_row, Pn, 0) + rows_s)
    ps = part2.t.double().sum(0).cpu()
    R.check_bound("sum G (perm form)", ps[0], sums2["s1"])
    R.check_bound("sum G*xhat (perm form)", ps[1], sums2["s2"])
    _guards(grid2=grid2, G2=G2, partial2=part2)
    with pytest.raises(KDError, match="ReLU6 is not supported"):
        lib.call("kd_lidar_seg_max_bwd", *mb[:3], R.RELU6, *mb[4:])


# ---- e. layer 0 ------------------------------------------------------------------------------------------------------------

def _l0_rows(C):
    s = R.cg_layout(1, C)[1]
    full = CAP * s
    return {"one": 1, "below_a_slot_row": max(1, s - 1), "cap-1": full - 1, "cap": full, "cap+1": full + 1, "first_4_in_flight": 3 * full + 1,
            "ragged_after_4": 4 * full + 5, "4_then_3_tail": 7 * full + 3}


L0_CASES = [(C, k) for C in (64, 96, 1024) for k in _l0_rows(64)]


def _l0_inputs(Pn, C):
    g = torch.Generator(device="cuda").manual_seed(Pn % 1000 + C)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    pts = r(Pn, 4) * torch.tensor([40.0, 40.0, 2.0, 1.0], device="cuda")
    return g, pts, r(C, 4) * 0.5, r(C)


@pytest.mark.parametrize("C,which", L0_CASES, ids=lambda v: str(v))
def test_l0_fwd(C, which):
    lib, _ = _lib()
    Pn = _l0_rows(C)[which]
    _, pts, w, b = _l0_inputs(Pn, C)
    _, slots, grid = R.cg_layout(Pn, C)
    rows = lib.kd_rowwise_stat_rows(Pn, C)
    assert rows == grid
    n_part = R.cg_iters(Pn, C) + slots
    p_less = max(1, Pn - max(1, Pn // 3))
    for mode in ("both", "stats_only", "y_only", "no_bias", "p_dev"):
        bias = None if mode == "no_bias" else b
        m = p_less if mode == "p_dev" else Pn
        p_dev = torch.tensor([m], device="cuda", dtype=torch.int32) if mode == "p_dev" else None
        y, part = Buf(Pn, C), Buf(rows, 2, C)
        lib.call("kd_lidar_l0_fwd", P(pts), P(w), P(bias), None if mode == "stats_only" else P(y.t), None if mode == "y_only" else P(part.t),
                 Pn, C, P(p_dev), None)
        torch.cuda.synchronize()
        ref = R.l0_fwd(pts[:m].double(), w.double(), None if bias is None else bias.double(), n_part)
        if mode != "stats_only":
            R.check_bound(f"y ({mode})", y.t[:m], ref["y"])
            assert bool(torch.isnan(y.t[m:]).all()), "rows beyond *p_dev written"
        else:
            assert bool(torch.isnan(y.t).all())
        if mode != "y_only":
            ps = part.t.double().sum(0)
            R.check_bound(f"sum y ({mode})", ps[0], ref["s1"])
            R.check_bound(f"sum y^2 ({mode})", ps[1], ref["s2"])
        else:
            assert bool(torch.isnan(part.t).all())
        _guards(y=y, partial=part)


@pytest.mark.parametrize("C,which", L0_CASES, ids=lambda v: str(v))
def test_l0_bwd(C, which):
    lib, _ = _lib()
    Pn = _l0_rows(C)[which]
    g, pts, w, b = _l0_inputs(Pn, C)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    Dg, Y, al, be, ga = r(Pn, C), r(Pn, C), r(C), r(C) * 0.1, r(C) * 0.1
    _, slots, grid = R.cg_layout(Pn, C)
    iters = R.cg_iters(Pn, C)
    nbytes = lib.kd_lidar_l0_bwd_ws_bytes(Pn, C)
    assert nbytes == grid * C * 5 * 4
    n_red = iters + slots + grid + R.SLAB_SPLIT
    tail = torch.arange(Pn, device="cuda") >= (iters - 1) * grid * slots          # the last ragged iteration, row 0, row P-1
    tail[0] = tail[-1] = True
    zero = torch.zeros(C, device="cuda")
    d = lambda t: None if t is None else t.double()
    for mode, Dv, Yv in (("D,Y", Dg, Y), ("D", Dg, None), ("none", None, None)):
        for run in ("all_rows", "tail_rows"):
            if run == "tail_rows":
                if Dv is None:
                    continue
                Dv, bv, gv = Dv * tail[:, None], zero, zero             # g = al * D: only the tail rows carry anything
            else:
                bv, gv = be, ga
            ws, dwb = Buf(nbytes // 4), Buf(C * 5)
            lib.call("kd_lidar_l0_bwd", P(Dv), P(Yv), P(w), P(b), P(al), P(bv), P(gv), P(pts), P(dwb.t), Pn, C, P(ws.t), nbytes, None)
            torch.cuda.synchronize()
            ref = R.l0_bwd(d(Dv), d(Yv), d(w), d(b), d(al), d(bv), d(gv), d(pts), n_red)
            R.check_bound(f"dw ({mode}, {run})", dwb.t[:C * 4], ref["dw"])
            R.check_bound(f"db ({mode}, {run})", dwb.t[C * 4:], ref["db"])
            _guards(ws=ws, dwb=dwb)


# ---- f. the LiDAR GEMM forms -------------------------------------------------------------------------------------------------

def _close(got, want, what):
    err = (got.double() - want).abs().max().item()
    scale = max(want.abs().max().item(), 1e-30)
    assert err <= TOL * scale, (what, err, scale)


@pytest.mark.usefixtures("gemm_arith")
@pytest.mark.parametrize("M", (1, 37, 129, 2100))
def test_l1_fwd_over_the_recomputed_layer0(M):
    lib, _ = _lib()
    K, N = 64, 128
    g = torch.Generator(device="cuda").manual_seed(M)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    pts = r(M, 4) * torch.tensor([40.0, 40.0, 2.0, 1.0], device="cuda")
    w0, b0, sc0, sh0 = r(K, 4) * 0.1, r(K), r(K).abs() * 0.2 + 0.1, r(K) * 0.3
    W1, bias1 = r(N, K) / K ** 0.5, r(N)
    want = R.point_mlp_l1(pts, w0, b0, sc0, sh0, W1, bias1)
    for epi in (0, 1):
        for m in ((None, M - M // 3) if M > 1 else (None,)):
            mm = M if m is None else m
            m_dev = None if m is None else torch.tensor([m], device="cuda", dtype=torch.int32)
            rows = lib.kd_pwconv_stat_rows_for(M, K, N, 3, 1, 0) if epi else 0
            out = Buf(M, N)
            # statistics slab: NaN-filled for the full launch (every row must be written), zeroed under m_dev
            part = None if not epi else torch.full((rows, 2, N), NAN if m is None else 0.0, device="cuda")
            lib.call("kd_lidar_l1_fwd", P(pts), P(w0), P(b0), P(sc0), P(sh0), R.RELU, P(W1), P(bias1), P(out.t), N, epi, P(part), rows,
                     M, K, N, P(m_dev), None)
            torch.cuda.synchronize()
            _close(out.t[:mm], want[:mm], ("l1_fwd", epi, m))
            assert bool(torch.isnan(out.t[mm:]).all()), "rows beyond *m_dev written"
            out.guard_ok("out")
            if epi:
                st, wv = part.double().sum(0), want[:mm]
                assert (st[0] - wv.sum(0)).abs().max().item() <= STAT_TOL * max(1.0, wv.abs().sum(0).max().item())
                assert (st[1] - (wv * wv).sum(0)).abs().max().item() <= STAT_TOL * max(1.0, (wv * wv).sum(0).max().item())


def _l2_rows(M, H, W, seed):
    """grid rows of M in-range points of a concentrated two-frame scene whose last eighth repeats earlier points"""
    rs = np.random.RandomState(seed)
    pts = (rs.randn(4 * M + 64, 4) * np.array([12.0, 12.0, 2.0, 1.0])).astype(np.float32)
    cell = R.bev_cells(pts, H, W, *R.RNG)
    cell = cell[cell >= 0][:M]
    assert len(cell) == M
    rows = (np.arange(M) >= M // 2) * (H * W) + cell
    dup = M // 8
    src = rs.randint(0, M - dup, dup) if dup else np.zeros(0, np.int64)
    rows[M - dup:] = rows[src]
    return rows, src


@pytest.mark.usefixtures("gemm_arith")
@pytest.mark.parametrize("M", (37, 129, 2100))
def test_l2_fwd_with_the_scatter_max_epilogue(M):
    lib, _ = _lib()
    K, N, H, W = 128, 128, 17, 9
    ncells = 2 * H * W
    rows, src = _l2_rows(M, H, W, M)
    g = torch.Generator(device="cuda").manual_seed(M + 1)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    A = r(M, K)
    if len(src):
        A[M - len(src):] = A[torch.from_numpy(src).cuda()]
    sc1, sh1, W2, bias2, sc2, sh2 = r(K).abs() + 0.5, r(K) * 0.2, r(N, K) / K ** 0.5, r(N), r(N).abs() + 0.5, r(N) * 0.2
    d_rows = _i32(rows)
    for m in (None, M - M // 3):
        mm = M if m is None else m
        m_dev = None if m is None else torch.tensor([m], device="cuda", dtype=torch.int32)
        want, occ = R.l2_scatter(A, sc1, sh1, W2, bias2, sc2, sh2, rows, ncells, mm)
        assert 0 < int(occ.sum()) < ncells and np.bincount(rows[:mm]).max() >= (2 if M < 100 else 4)
        grid = Buf(ncells, N)
        lib.call("kd_lidar_l2_fwd_scatter", P(A), K, P(sc1), P(sh1), R.RELU, P(W2), P(bias2), P(sc2), P(sh2), R.RELU, P(d_rows), P(grid.t),
                 ncells, M, K, N, P(m_dev), None)
        torch.cuda.synchronize()
        # max is 1-Lipschitz: the GEMM tolerance on the activations carries over to the grid
        _close(grid.t, want, ("l2_fwd_scatter", m))
        assert bool((grid.t[~occ] == 0).all()), "empty cells"
        grid.guard_ok("grid")


# ---- g. error paths (nothing is launched) ------------------------------------------------------------------------------------

def test_refusals():
    lib, KDError = _lib()
    t = torch.zeros(64 * 64, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    geo = (1, 16, 64, 4, 4, *R.RNG)
    need = lib.kd_lidar_scatter_bwd_ws_bytes(1, 4, 4, 64)
    with pytest.raises(KDError, match="workspace too small"):
        lib.call("kd_lidar_scatter_max_bwd", P(t), P(t), P(t), P(t), R.RELU, P(t), P(t), P(t), P(t), P(t), P(t), *geo, P(t), need - 1, None)
    need = lib.kd_lidar_l0_bwd_ws_bytes(16, 64)
    with pytest.raises(KDError, match="workspace too small"):
        lib.call("kd_lidar_l0_bwd", P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), P(t), 16, 64, P(t), need - 1, None)
    none = "needs a non-negative activation"
    with pytest.raises(KDError, match=none):
        lib.call("kd_lidar_scatter_max_fwd", P(t), P(t), P(t), P(t), 0, P(t), *geo, None)
    with pytest.raises(KDError, match=none):
        lib.call("kd_lidar_scatter_max_idx_fwd", P(t), P(t), P(t), 0, P(i), P(t), 16, 64, 16, None, None)
    with pytest.raises(KDError, match=none):
        lib.call("kd_lidar_seg_max_fwd", P(t), P(t), P(t), 0, P(i), None, None, P(t), 16, 16, 64, None)
    with pytest.raises(KDError, match=none):
        lib.call("kd_lidar_seg_hold_fwd", P(t), P(t), P(t), 0, P(i), P(i), P(t), P(t), P(i), 16, 16, 64, None)
    with pytest.raises(KDError, match=none):
        lib.call("kd_lidar_l2_fwd_scatter", P(t), 64, P(t), P(t), R.RELU, P(t), P(t), P(t), P(t), 0, P(i), P(t), 16, 16, 64, 64, None, None)
    relu6 = "ReLU6 is not supported"
    with pytest.raises(KDError, match=relu6):
        lib.call("kd_lidar_seg_share_bwd", P(t), P(t), P(t), R.RELU6, P(t), P(t), P(t), P(t), P(i), P(i), P(t), P(t), P(t), 16, 16, 64, None)
    with pytest.raises(KDError, match=relu6):
        lib.call("kd_lidar_l2_dgrad", P(t), 64, P(i), P(t), P(t), P(t), P(t), P(t), P(t), P(t), R.RELU6, P(t), P(t), 64, P(t), 64, P(t), P(t),
                 P(t), P(t), R.RELU, P(t), 1, 16, 64, 64, None)
    with pytest.raises(KDError, match=relu6):
        lib.call("kd_lidar_l2_wgrad", P(t), 64, P(i), P(t), P(t), P(t), P(t), P(t), P(t), P(t), R.RELU6, P(t), 64, P(t), P(t), R.RELU, P(t),
                 16, 64, 64, P(t), 4096, None)
