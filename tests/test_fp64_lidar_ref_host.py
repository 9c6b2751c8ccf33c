"""The references of tests/_fp64_lidar_ref.py (the truth of tests/test_gpu_lidar_kernels.py) against stock torch on the CPU, the
error bounds they state met by a plain fp32 evaluation, the conditions the GPU tests rely on (no activated value of any scene
sits on an fp32 midpoint; the grids and ranges of the binning test make a swapped axis visible), and -- once, here -- each GPU
comparison shown to fail on a deliberately wrong reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fp64_lidar_ref as R

D = torch.float64
GRIDS = [(16, 16), (33, 17), (17, 33), (1, 40), (40, 1), (128, 128), (192, 192)]
RANGES = [(-50.0, 50.0, -50.0, 50.0), (-20.0, 80.0, -5.0, 3.0)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def test_layout_mirror():
    assert R.cg_layout(1000, 96, 4096) == (24, 10, 100)          # 24 groups, 10 slots, 16 idle threads per block
    assert R.cg_layout(229379, 64) == (16, 16, 2048) and R.cg_iters(229379, 64) == 8
    assert R.cg_layout(5, 1024) == (256, 1, 5) and R.cg_layout(1, 32, 4096) == (8, 32, 1)


# ---- binning ---------------------------------------------------------------------------------------------------------------

def _torch_cells(pts, H, W, x0, x1, y0, y1):
    """lidar_encoder.py:46-55, 69-71 as written, on one frame"""
    p = torch.from_numpy(pts)
    x, y = p[..., 0], p[..., 1]
    xn = (x - x0) / (x1 - x0)
    yn = (y - y0) / (y1 - y0)
    valid = (xn >= 0) & (xn <= 1) & (yn >= 0) & (yn <= 1)
    coords = torch.stack([xn, yn], -1)
    coords = torch.where(valid[:, None], coords, torch.zeros_like(coords))       # (the model indexes with the mask instead)
    gc = (coords * torch.tensor([W - 1, H - 1], dtype=torch.float32)).long()
    ix, iy = gc[..., 0].clamp(0, W - 1), gc[..., 1].clamp(0, H - 1)
    return torch.where(valid, iy * W + ix, torch.full_like(ix, -1)).numpy()


@pytest.mark.parametrize("rng", RANGES, ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("H,W", GRIDS)
def test_bev_cells_is_the_model_expression(H, W, rng):
    pts = R.binning_points(H, W, rng)
    cell = R.bev_cells(pts, H, W, *rng)
    assert np.array_equal(cell, _torch_cells(pts, H, W, *rng))
    edge = R.edge_points(H, W, *rng)
    ce = R.bev_cells(edge, H, W, *rng)
    assert (ce >= 0).sum() > 2 and (ce < 0).sum() >= 10            # the ends are in, their outer neighbours, Inf and NaN are out
    assert len(np.unique(ce[ce >= 0])) >= max(H, W) // 2           # the boundary values reach across the grid


@pytest.mark.parametrize("rng", RANGES, ids=["symmetric", "asymmetric"])
@pytest.mark.parametrize("H,W", GRIDS)
def test_swapped_axes_are_visible(H, W, rng):
    """a W-1 / H-1 exchange shows on every non-square grid, an x / y range exchange on the asymmetric range: more than 10 % of
    the valid points land in another cell -- and, perturbing the reference, the GPU test's comparison fails on them"""
    pts = R.binning_points(H, W, rng)
    cell = R.bev_cells(pts, H, W, *rng)
    assert (cell >= 0).mean() > 0.4
    for swap, visible in (("factors", H != W), ("ranges", rng[:2] != rng[2:])):
        frac = R.swapped_axis_fraction(pts, H, W, rng, swap)
        if visible:
            assert frac > 0.10, (swap, frac)
            with pytest.raises(AssertionError, match="cell"):
                R.check_exact("cell", cell.astype(np.int32), R.bev_cells(pts, H, W, *rng, swap=swap).astype(np.int32))
        elif swap == "factors" or min(H, W) > 1:
            assert frac == 0.0 or swap == "ranges", (swap, frac)


# ---- scatter-max -----------------------------------------------------------------------------------------------------------

def _tie_scene(seed, P=900, C=12, ncells=40):
    g = _g(seed)
    rows = torch.randint(-1, ncells - 5, (P,), generator=g).numpy().astype(np.int64)       # -1: out of range; 5 empty rows
    z = (torch.randint(-8, 30, (P, C), generator=g).float() * 0.25)                         # quarter steps: exact ties, exact 6.0
    return rows, z


@pytest.mark.parametrize("act", [R.RELU, R.RELU6], ids=["relu", "relu6"])
def test_scatter_max_and_its_gradient_are_aten(act):
    """zeros.scatter_reduce_(amax, include_self=False) of the activated features and its autograd, float64, on inputs full of
    exact ties and (ReLU6) saturated maxima: the even split and the z < 6 rule are ATen's own"""
    rows, z = _tie_scene(3)
    ncells, C = 40, z.shape[1]
    one, zero = torch.ones(C), torch.zeros(C)
    v, risky = R.activated(z, one, zero, act)
    assert risky == 0
    grid, holder, counts = R.scatter_max(rows, v, ncells)
    assert int((counts > 1).sum()) > 50
    zt = z.double().requires_grad_()
    a = F.relu(zt) if act == R.RELU else F.hardtanh(zt, 0.0, 6.0)
    valid = torch.from_numpy(rows >= 0)
    idx = torch.from_numpy(rows[rows >= 0])[:, None].expand(-1, C)
    out = torch.zeros(ncells, C, dtype=D).scatter_reduce_(0, idx, a[valid], "amax", include_self=False)
    assert np.array_equal(grid.astype(np.float64), out.detach().numpy())
    _close(torch.from_numpy(v.numpy().astype(np.float64)), a.detach(), 0.0)
    dout = torch.randn(ncells, C, generator=_g(4))
    (out * dout.double()).sum().backward()
    mean, inv = torch.randn(C, generator=_g(5)) * 0.1, torch.rand(C, generator=_g(6)) + 0.5
    G, sums = R.scatter_max_grad(rows, v, holder, counts, dout, z, mean, inv, act, n_seq=1)
    want = zt.grad
    if act == R.RELU6:
        assert int(((grid == 6.0) & (counts > 0)).sum()) > 50 and bool((want[torch.from_numpy(v.numpy() >= 6)] == 0).all())
    # G is the float64 quotient rounded once to fp32
    assert bool(((torch.from_numpy(G).double() - want).abs() <= R.U * want.abs()).all())
    assert bool((torch.from_numpy(G)[~valid] == 0).all())
    xh = (z.double() - mean.double()) * inv.double()
    _close(sums["s1"][0], torch.from_numpy(G).double().sum(0))
    _close(sums["s2"][0], (torch.from_numpy(G).double() * xh).sum(0))
    # the sums as the kernels form them, in fp32, meet the bound stated for their chain length
    Gf = torch.from_numpy(G)
    n_seq = len(rows)
    _, s = R.scatter_max_grad(rows, v, holder, counts, dout, z, mean, inv, act, n_seq=n_seq)
    R.check_bound("s1", Gf.sum(0), s["s1"])
    R.check_bound("s2", (Gf * ((z - mean) * inv)).sum(0), s["s2"])


def test_a_wrong_tie_split_is_caught():
    """count off by one in the split: the bit comparison of G fails (every holder's share changes)"""
    rows, z = _tie_scene(8)
    v, _ = R.activated(z, torch.ones(12), torch.zeros(12), R.RELU)
    grid, holder, counts = R.scatter_max(rows, v, 40)
    dout = torch.randn(40, 12, generator=_g(9))
    a = (rows, v, holder, counts, dout, z, torch.zeros(12), torch.ones(12), R.RELU)
    G, s = R.scatter_max_grad(*a, n_seq=len(rows))
    Gw, sw = R.scatter_max_grad(*a, n_seq=len(rows), count_offset=1)
    with pytest.raises(AssertionError, match="G:"):
        R.check_exact("G", G, Gw)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_bound("sum G", torch.from_numpy(G).sum(0), sw["s1"])


@pytest.mark.parametrize("name", sorted(R.SCENES))
def test_scenes_have_no_midpoint_and_the_cases_they_are_for(name):
    B, N, H, W, sigma, pad, dup, nan, scale = R.SCENES[name]
    for C in R.SCENE_WIDTHS:
        _, _, _, _, pts, y, sc, sh, mean, inv = R.scene(name, C)
        rows = R.grid_rows(pts, B, N, H, W, R.RNG)
        for act in (R.RELU, R.RELU6):
            v, risky = R.activated(y, sc, sh, act)
            assert risky == 0, (name, C, act, risky)
        # (v is the ReLU6 value from here on)
        grid, holder, counts = R.scatter_max(rows, v, B * H * W)
        per_row = np.bincount(rows[rows >= 0], minlength=B * H * W)
        assert (rows >= 0).any() and ((rows < 0).any() or sigma < 20)      # out-of-range points unless the scene is concentrated
        if dup:
            assert int((counts > 1).sum()) > 100                      # exact ties
        if name in ("pad", "row257", "sigma1"):
            assert per_row.max() > 256                                # long cells
        if name == "sat":
            occ = per_row > 0
            assert ((grid[occ] == 6.0).mean()) > 0.20                 # saturated (cell, channel) pairs under ReLU6
        if name in ("dup_rect", "sat"):
            assert H != W


# ---- layer 0 ---------------------------------------------------------------------------------------------------------------

def _l0_inputs(P, C, seed, dtype=D):
    g = _g(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D)
    t = (r(P, 4) * torch.tensor([40.0, 40.0, 2.0, 1.0], dtype=D), r(C, 4) * 0.5, r(C), r(P, C), r(P, C), r(C), r(C) * 0.1, r(C) * 0.1)
    return [x.float().to(dtype) for x in t]                       # fp32-representable values in either dtype


def test_l0_is_conv1d_and_its_autograd():
    P, C = 300, 24
    pts, w, b, Dg, Y, al, be, ga = _l0_inputs(P, C, 1)
    w, b = w.requires_grad_(), b.requires_grad_()
    y = F.conv1d(pts.t()[None], w[:, :, None], b)[0].t()
    r = R.l0_fwd(pts, w.detach(), b.detach(), n_part=1)
    _close(r["y"][0], y.detach())
    _close(r["s1"][0], y.detach().sum(0))
    _close(r["s2"][0], (y.detach() ** 2).sum(0))
    _close(R.l0_fwd(pts, w.detach(), None, 1)["y"][0], F.conv1d(pts.t()[None], w.detach()[:, :, None])[0].t())
    # dL/dy = al*D + be*y + ga is the gradient of  sum (al*D + ga) * y + be * y^2 / 2
    for Dv, Yv in ((Dg, Y), (Dg, None), (None, None)):
        w.grad = b.grad = None
        yy = y if Yv is None else Yv
        d0 = torch.zeros_like(y) if Dv is None else Dv
        gsel = (al * d0 + be * yy + ga).detach()
        (y * gsel).sum().backward(retain_graph=True)
        r = R.l0_bwd(Dv, Yv, w.detach(), b.detach(), al, be, ga, pts, n_red=1)
        _close(r["dw"][0], w.grad)
        _close(r["db"][0], b.grad)


@pytest.mark.parametrize("P,C", [(1, 64), (2049, 96), (40000, 64), (3000, 1024)])
def test_fp32_layer0_meets_the_bounds(P, C):
    a64, a32 = _l0_inputs(P, C, P + C), _l0_inputs(P, C, P + C, torch.float32)
    n = P                                                          # torch's fp32 sums are no longer than one sequential pass
    f64, f32 = R.l0_fwd(*a64[:3], n_part=n), R.l0_fwd(*a32[:3], n_part=n)
    for k in ("y", "s1", "s2"):
        R.check_bound(k, f32[k][0], f64[k])
    for mode in range(3):
        sel = lambda a: (a[3] if mode < 2 else None, a[4] if mode == 0 else None, a[1], a[2], a[5], a[6], a[7], a[0])
        b64, b32 = R.l0_bwd(*sel(a64), n_red=n), R.l0_bwd(*sel(a32), n_red=n)
        for k in ("dw", "db"):
            R.check_bound(k, b32[k][0], b64[k])


def test_a_dropped_tail_row_is_caught():
    """D nonzero only in row 0 and row P-1 (the GPU test's second run): leaving out the last point fails the bound by O(1)"""
    P, C = 5000, 64
    pts, w, b, Dg, Y, al, be, ga = _l0_inputs(P, C, 77)
    be, ga = torch.zeros_like(be), torch.zeros_like(ga)
    Dg[1:-1] = 0
    n_red = R.cg_iters(P, C) + 16 + 313 + R.SLAB_SPLIT
    good = R.l0_bwd(Dg, Y, w, b, al, be, ga, pts, n_red)
    bad = R.l0_bwd(Dg, Y, w, b, al, be, ga, pts, n_red, drop_last_row=True)
    R.check_bound("dw", good["dw"][0].float(), good["dw"])
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_bound("dw", good["dw"][0].float(), bad["dw"])
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_bound("db", good["db"][0].float(), bad["db"])


# ---- the GEMM forms ----------------------------------------------------------------------------------------------------------

def test_point_mlp_l1_and_l2_scatter_are_the_model_layers():
    g = _g(5)
    M, K, N, ncells = 257, 64, 128, 30
    r = lambda *s: torch.randn(*s, generator=g)
    pts, w0, b0, sc0, sh0 = r(M, 4), r(K, 4), r(K), r(K).abs() + 0.5, r(K) * 0.2
    W1, bias1 = r(N, K) / 8, r(N)
    a0 = F.relu(F.conv1d(pts.double().t()[None], w0.double()[:, :, None], b0.double())[0].t() * sc0.double() + sh0.double())
    want = F.conv1d(a0.t()[None], W1.double()[:, :, None], bias1.double())[0].t()
    _close(R.point_mlp_l1(pts, w0, b0, sc0, sh0, W1, bias1), want)
    A, sc1, sh1, W2, bias2, sc2, sh2 = r(M, N), r(N).abs() + 0.5, r(N) * 0.2, r(N, N) / 11, r(N), r(N).abs() + 0.5, r(N) * 0.2
    rows = torch.randint(0, ncells - 4, (M,), generator=g).numpy()
    m = 200
    v = F.relu((F.relu(A.double() * sc1.double() + sh1.double()) @ W2.double().t() + bias2.double()) * sc2.double() + sh2.double())
    idx = torch.from_numpy(rows[:m])[:, None].expand(-1, N)
    want = torch.zeros(ncells, N, dtype=D).scatter_reduce_(0, idx, v[:m], "amax", include_self=False)
    grid, occ = R.l2_scatter(A, sc1, sh1, W2, bias2, sc2, sh2, rows, ncells, m)
    _close(grid, want, 0.0)
    assert bool((grid[~occ] == 0).all()) and int((~occ).sum()) >= 4
