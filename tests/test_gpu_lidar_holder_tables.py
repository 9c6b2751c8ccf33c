"""Scatter-max backward from the holder tables (kd_lidar_seg_hold_fwd / kd_lidar_seg_hold_bwd) against the two-sweep pair
(kd_lidar_seg_max_fwd / kd_lidar_seg_share_bwd), through the C ABI, BIT FOR BIT: the same grid, the same share table and the
same BatchNorm-backward partial sums, every row of them.  Everything here is exact; no tolerance appears.
(The two-sweep pair is itself bit-identical to the atomic pair, test_gpu_lidar_segments.py, which -- like the holder-table
path on the scenes below -- is pinned to an independent reference in test_gpu_lidar_kernels.py.)

The contract covers finite features: a NaN / Inf feature is outside it (the two-sweep pair itself turns one into a NaN sum),
so the scenes put non-finite values into the point COORDINATES only (those points are out of range and never scattered).

The new backward has two routes per cell -- the tables, or the two sweeps for a cell marked 255 -- and a test that only
compared results could let one hide the other.  So the holders table itself is checked: against the holder counts the
two-sweep kernel finds (share of dout = 1 is 1 / holders), and on three constructed inputs
  (a) distinct points, ordinary sc: NO cell is marked, everything went through the tables
      (checked on the CPU beforehand for these seeds: no (cell, channel) of this recipe has two holders at all);
  (b) sc = 2^-30, sh = 1, |raw| < 32: raw * sc is below half an ulp of 1, every point of a cell is a holder of the activated
      maximum 1.0 with its own raw value, so EVERY cell of two or more points is marked (the whole table is predicted);
  (c) duplicated points: holders > 1 and not marked."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu]

RNG = (-50.0, 50.0, -50.0, 50.0)
SWEEP = 255                 # holders entry: "sweep the cell's rows"
LONG = 256                  # rows with more points go to the chunked kernels

# B, N, H, W, sigma, pad, dup, nan  (the scene recipes of test_gpu_lidar_segments.py)
SCENES = {
    "uniform": (2, 6000, 16, 16, 40.0, 0, 0, 0),
    "sigma1": (2, 9000, 32, 32, 1.0, 0, 0, 0),
    "sigma5": (2, 9000, 32, 32, 5.0, 0, 0, 0),
    "dup": (2, 6000, 16, 16, 40.0, 0, 300, 0),
    "nan": (3, 5000, 64, 64, 40.0, 0, 200, 40),
    "pad": (2, 3000, 16, 16, 40.0, 1500, 100, 0),
    "row257": (1, 700, 8, 8, 12.0, 257, 0, 0),
}


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _inputs(B, N, C, seed, pad=0, dup=0, nan=0, sigma=40.0):
    g = torch.Generator().manual_seed(seed)
    pts = torch.randn(B, N, 4, generator=g) * torch.tensor([sigma, sigma, 2.0, 1.0])
    if pad:
        pts[:, N - pad:] = 0.0
    y = torch.randn(B * N, C, generator=g)
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
    return [t.cuda().contiguous() for t in (pts.view(B * N, 4), y, sc, sh, mean, invstd)]


def _sorted_rows(lib, pts, y, B, N, H, W):
    P, ncells = B * N, B * H * W
    spts, srow = torch.empty_like(pts), torch.empty(P, device="cuda", dtype=torch.int32)
    start, perm = torch.empty(ncells + 1, device="cuda", dtype=torch.int32), torch.empty(P, device="cuda", dtype=torch.int32)
    nb = lib.kd_lidar_sort_points_ws_bytes(B, N, H, W)
    ws = torch.empty(nb, device="cuda", dtype=torch.uint8)
    lib.call("kd_lidar_sort_points", _P(pts), B, N, H, W, *RNG, _P(spts), _P(srow), _P(start), _P(perm), _P(ws), nb, None)
    return y[perm.long()].contiguous(), srow, start


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def _both_pairs(lib, ys, srow, start, sc, sh, mean, invstd, dout, P, ncells, C):
    """-> holders [ncells, C] (numpy uint8), counts per cell, holder counts of the two-sweep kernel; asserts the bitwise equalities."""
    def two_sweeps(d):
        grid = torch.full((ncells, C), -1.0, device="cuda")
        lib.call("kd_lidar_seg_max_fwd", _P(ys), _P(sc), _P(sh), 1, _P(start), None, _P(srow), _P(grid), P, ncells, C, None)
        share = torch.full((ncells, C), float("nan"), device="cuda")
        cnt = torch.full((ncells, C), float("nan"), device="cuda")
        part = torch.full((lib.kd_lidar_seg_share_stat_rows(ncells, P), 2, C), float("nan"), device="cuda")
        lib.call("kd_lidar_seg_share_bwd", _P(ys), _P(sc), _P(sh), 1, _P(grid), _P(d), _P(mean), _P(invstd), _P(start), _P(srow),
                 _P(share), _P(cnt), _P(part), P, ncells, C, None)
        return grid, share, part

    grid_o, share_o, part_o = two_sweeps(dout)
    grid_n = torch.full((ncells, C), -1.0, device="cuda")
    rawmax = torch.full((ncells, C), float("nan"), device="cuda")
    holders = torch.full((ncells, C), 77, device="cuda", dtype=torch.uint8)
    lib.call("kd_lidar_seg_hold_fwd", _P(ys), _P(sc), _P(sh), 1, _P(start), _P(srow), _P(grid_n), _P(rawmax), _P(holders), P, ncells,
             C, None)
    share_n = torch.full((ncells, C), float("nan"), device="cuda")
    cnt_n = torch.full((ncells, C), float("nan"), device="cuda")
    part_n = torch.full_like(part_o, float("nan"))
    lib.call("kd_lidar_seg_hold_bwd", _P(ys), _P(sc), _P(sh), 1, _P(grid_n), _P(rawmax), _P(holders), _P(dout), _P(mean), _P(invstd),
             _P(start), _P(srow), _P(share_n), _P(cnt_n), _P(part_n), P, ncells, C, None)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(grid_o), _bits(grid_n))
    assert np.array_equal(_bits(share_o), _bits(share_n))          # rows of empty cells: untouched by both (same NaN fill)
    assert np.array_equal(_bits(part_o), _bits(part_n))
    assert bool(torch.isfinite(part_n).all())
    # holder counts as the two-sweep kernel sees them: share of dout = 1 is 1 / holders (exact for holders <= 256), 0 for none
    _, share_1, _ = two_sweeps(torch.ones_like(dout))
    torch.cuda.synchronize()
    counts = (start[1:] - start[:-1]).cpu().numpy()
    s1 = share_1.cpu().numpy().astype(np.float64)
    short = (counts > 0) & (counts <= LONG)
    with np.errstate(divide="ignore"):
        want = np.where(s1[short] > 0, np.rint(1.0 / s1[short]), 0).astype(np.int64)
    h = holders.cpu().numpy()
    hs = h[short].astype(np.int64)
    assert np.all((hs == SWEEP) | (hs == want))
    assert np.all(hs[want >= SWEEP] == SWEEP)
    assert np.all(h[counts == 0] == 0) and np.all(h[counts > LONG] == SWEEP)
    # rawmax of an unmarked holder is a raw value that activates to the maximum
    rm, g = rawmax.cpu().numpy()[short], grid_n.cpu().numpy()[short]
    sel = (hs != SWEEP) & (hs > 0)
    act = torch.clamp_min(torch.addcmul(sh, rawmax, sc), 0).cpu().numpy()[short]
    assert np.allclose(act[sel], g[sel], rtol=1e-5, atol=1e-6) and np.all(np.isfinite(rm[sel]))
    return h, counts, want, short


@pytest.mark.parametrize("C", (64, 128, 256))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_holder_tables_give_the_two_sweep_results_bitwise(C, scene):
    from kdrt.lib import lib
    B, N, H, W, sigma, pad, dup, nan = SCENES[scene]
    pts, y, sc, sh, mean, invstd = _inputs(B, N, C, 5 + C, pad=pad, dup=dup, nan=nan, sigma=sigma)
    ncells, P = B * H * W, B * N
    ys, srow, start = _sorted_rows(lib, pts, y, B, N, H, W)
    dout = torch.randn(ncells, C, generator=torch.Generator().manual_seed(5)).cuda()
    h, counts, want, short = _both_pairs(lib, ys, srow, start, sc, sh, mean, invstd, dout, P, ncells, C)
    hs = h[short]
    if scene in ("sigma1", "sigma5", "pad", "row257"):
        assert int(counts.max()) > LONG                   # the chunked kernels really ran
    if scene == "uniform":                                # (a): nothing marked -- every short cell went through the tables
        assert int(counts.max()) <= LONG and not np.any(h == SWEEP)
        assert np.all(hs <= 1) and int((hs == 1).sum()) > ncells
    if dup:                                               # (c): ties from duplicated points are counted, not marked
        tied = (hs > 1) & (hs != SWEEP)
        assert int(tied.sum()) > 0 and np.array_equal(hs[tied], want[tied])
        assert not np.any(hs == SWEEP)


@pytest.mark.parametrize("C", (64, 128, 256))
def test_holders_with_different_raw_values_mark_the_cell_for_the_sweep(C):
    """(b) of the module docstring: the whole holders table is predicted on the CPU, and every cell of 2+ points is marked."""
    from kdrt.lib import lib
    B, N, H, W = 2, 4000, 24, 24
    pts, y, _, _, mean, invstd = _inputs(B, N, C, 31 + C)
    assert float(y.abs().max()) < 32.0
    sc = torch.full((C,), 2.0 ** -30, device="cuda")
    sh = torch.ones(C, device="cuda")
    ncells, P = B * H * W, B * N
    ys, srow, start = _sorted_rows(lib, pts, y, B, N, H, W)
    dout = torch.randn(ncells, C, generator=torch.Generator().manual_seed(7)).cuda()
    h, counts, want, short = _both_pairs(lib, ys, srow, start, sc, sh, mean, invstd, dout, P, ncells, C)
    assert int(counts.max()) <= LONG
    assert np.array_equal(want, np.repeat(counts[short][:, None], C, 1))       # every point holds the maximum 1.0
    # prediction: n points, marked iff some raw value differs bitwise from the first point's
    st, yb = start.cpu().numpy(), _bits(ys)
    pred = np.zeros((ncells, C), np.uint8)
    for r in np.nonzero(counts)[0]:
        rows = yb[st[r]:st[r + 1]]
        mixed = np.any(rows != rows[0], axis=0)
        pred[r] = np.where(mixed | (counts[r] >= SWEEP), SWEEP, counts[r])
    assert np.array_equal(h, pred)
    multi = counts >= 2
    assert int(multi.sum()) > 100 and np.all(np.any(h[multi] == SWEEP, axis=1))
    assert np.all(h[counts == 1] == 1)


@pytest.mark.parametrize("same", (254, 256))
def test_holder_count_saturates_into_the_sweep(same):
    """One cell of `same` identical points: 254 holders fit the byte (the table route adds the share 254 times), 256 do not."""
    from kdrt.lib import lib
    B, N, H, W, C = 1, 300, 4, 4, 128
    pts, y, sc, sh, mean, invstd = _inputs(B, N, C, 3)
    pts[:same, :2] = 40.0
    pts[same:, :2] = -40.0 - torch.rand(N - same, 2, device="cuda")
    y[:same] = y[0]
    ncells, P = B * H * W, B * N
    ys, srow, start = _sorted_rows(lib, pts, y, B, N, H, W)
    dout = torch.randn(ncells, C, generator=torch.Generator().manual_seed(9)).cuda()
    h, counts, want, short = _both_pairs(lib, ys, srow, start, sc, sh, mean, invstd, dout, P, ncells, C)
    assert sorted(counts[counts > 0].tolist()) == sorted([same, N - same])
    row = h[int(np.nonzero(counts == same)[0][0])]
    assert set(row.tolist()) == ({0, same} if same < SWEEP else {0, SWEEP})


def test_hold_entry_points_reject_unsupported_width():
    from kdrt.lib import KDError, lib
    t = torch.zeros(64, device="cuda")
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    with pytest.raises(KDError, match="C must be 64, 128 or 256"):
        lib.call("kd_lidar_seg_hold_fwd", _P(t), _P(t), _P(t), 1, _P(i), _P(i), _P(t), _P(t), _P(i), 1, 1, 96, None)
    with pytest.raises(KDError, match="C must be 64, 128 or 256"):
        lib.call("kd_lidar_seg_hold_bwd", _P(t), _P(t), _P(t), 1, _P(t), _P(t), _P(i), _P(t), _P(t), _P(t), _P(i), _P(i), _P(t), _P(t),
                 _P(t), 1, 1, 96, None)


@pytest.mark.parametrize("sigma", (40.0, 2.0))
def test_lidar_encoder_same_gradient_bits_with_and_without_holder_tables(sigma):
    """One training forward + backward of the whole encoder with the module switch old / new: same output and same
    parameter gradients bit for bit (sigma = 2 m: a few cells hold more than a thousand points, the chunked kernels run)."""
    from kdrt import units
    from src.models.lidar_encoder import LiDAREncoder
    torch.manual_seed(3)
    enc = LiDAREncoder(encoder_type="spatial", grid_size=(32, 32)).cuda().train(True)
    pts = _inputs(2, 6000, 64, 21, pad=500, dup=300, sigma=sigma)[0].view(2, 6000, 4)
    res = {}
    saved = units._SCATTER_HOLDERS
    calls = []
    real_call = units.lib.call
    try:
        units.lib.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        for hold in (False, True):
            units._SCATTER_HOLDERS = hold
            units.clear_step_caches()
            enc.zero_grad()
            calls.clear()
            y = enc(pts)
            (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
            torch.cuda.synchronize()
            res[hold] = (y.detach().clone(), {n: p.grad.clone() for n, p in enc.named_parameters()})
            assert ("kd_lidar_seg_hold_fwd" in calls) == hold and ("kd_lidar_seg_hold_bwd" in calls) == hold
            assert ("kd_lidar_seg_share_bwd" in calls) != hold
    finally:
        units._SCATTER_HOLDERS = saved
        del units.lib.__dict__["call"]
    assert np.array_equal(_bits(res[False][0]), _bits(res[True][0]))
    assert len(res[True][1]) > 0
    for n, g in res[False][1].items():
        assert bool(torch.isfinite(g).all()), n
        assert np.array_equal(_bits(g), _bits(res[True][1][n])), n
