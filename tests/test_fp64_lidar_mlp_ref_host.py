"""Self-check of tests/_fp64_lidar_mlp_ref.py on the host: the references ARE the backward of the point MLP and its scatter-max
(compared with torch.autograd in float64 on a scene with ties, zero-maximum cells and off-grid rows, which ties the table
convention share = dout / holders to ATen's even split among ties), their bounds hold for an honest fp32 evaluation at every shape
of tests/test_gpu_lidar_mlp_bwd.py, eight wrong readings of the contract leave them, and the layout mirrors equal the library's
host-side answers."""
import pytest
import torch
import torch.nn.functional as F

import _fp64_lidar_mlp_ref as L
from test_fp64_gemm_ref_host import EPS, _bn_coeffs, _finalize

GENERAL_M = (1, 33, 129, 4133)
L2_SHAPES = [(64, 128), (128, 128), (256, 128), (36, 40)]           # (N2, K1)
L1_SHAPES = [(128, 64), (128, 128), (40, 36)]                        # (N1, K0)
FUSED_M = (1, 31, 32, 33, 8193, 8225, 16461, 32769, 131071, 131072)
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("RATIO fp32-evaluation", k, f"{WORST[k]:.4f}")


def _l2_layouts(M, N2, K1):
    """(name, statistics layout, n_red of the weight gradient) of every form that serves the shape"""
    wg = L.R.wgrad_tiled_layout(M, N2, K1, True)["n_red"]
    out = [("tiled", L.l2_dgrad_layout(M, N2, K1, "tiled"), wg)]
    if (N2, K1) == (128, 128):
        out.append(("stream", L.l2_dgrad_layout(M, N2, K1, "stream"), wg))
        f = L.fused_layout(M, 2)
        out.append(("fused", f, f["n_red"]))
    return out


def _l2_ref(sc, lay, n_red, dtype, mut=(), slab_row=None):
    M = sc["Y2"].shape[0]
    row = L.slab_row_of(M, lay) if slab_row is None else slab_row
    return L.l2_backward(*L.l2_args(sc, dtype), row, lay["rows"], lay["n_part"], n_red, mut=mut)


def _l1_ref(d, mact, lay, n_m1, n_red, dtype, mut=()):
    M = d["G"].shape[0]
    return L.l1_backward(*L.l1_args(d, mact, dtype), L.slab_row_of(M, lay), lay["rows"], lay["n_part"], n_m1, n_red, mut=mut)


# ---- the references are autograd ---------------------------------------------------------------------------------------------

def test_references_equal_autograd():
    g = torch.Generator().manual_seed(11)
    M, C0, C1, C2, cells = 192, 8, 12, 16, 14
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    pts = r(M, 4) * torch.tensor([20.0, 20.0, 2.0, 0.3], dtype=torch.float64)
    rows = torch.cat([torch.repeat_interleave(torch.arange(10), 17), torch.tensor([-1, -2, L.INT_MIN] * 7 + [-1])]).to(torch.int32)   # cells 10 .. 13 empty
    assert rows.numel() == M
    pts[17:20] = pts[17]                 # cell 1 is a tie of three and a tie of fourteen: one of them holds each maximum
    pts[20:34] = pts[20]
    pts[34:36] = pts[34]                 # a tie of two in cell 2
    pts[170:] = pts[0]                   # off-grid rows with the features of a row of cell 0
    w0, b0, W1, W2 = r(C0, 4) * 0.1, r(C0) * 0.1, r(C1, C0) / C0 ** 0.5, r(C2, C1) / C1 ** 0.5
    g0, be0, g1, be1, g2, be2 = r(C0).abs() + 0.5, r(C0) * 0.3, r(C1).abs() + 0.5, r(C1) * 0.3, r(C2).abs() + 0.5, r(C2) * 0.3
    be2[0:3] = -6.0                      # channels in which every cell's maximum is 0
    dout = r(cells, C2)
    leaves = [w0, b0, W1, W2, g0, be0, g1, be1, g2, be2]
    for t in leaves:
        t.requires_grad_(True)
    bn = lambda y, ga, be: F.batch_norm(y, None, None, ga, be, True, 0.1, EPS)
    conv = lambda a, W: (a[:, None, :] * W[None, :, :]).sum(-1)       # Conv1d(k = 1); row by row, so that equal points give equal bits
    y0 = conv(pts, w0) + b0
    z0 = bn(y0, g0, be0)
    y1 = conv(z0.clamp_min(0), W1)
    z1 = bn(y1, g1, be1)
    a1 = z1.clamp_min(0)
    y2 = conv(a1, W2)
    z2 = bn(y2, g2, be2)
    h = z2.clamp_min(0)
    ok = rows >= 0
    grid = torch.zeros(cells, C2, dtype=torch.float64).index_reduce(0, rows[ok].long(), h[ok], "amax", include_self=True)
    for t in (z0, z1, a1, z2):
        t.retain_grad()
    (grid * dout).sum().backward()
    with torch.no_grad():
        close = lambda got, want, what: torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-10, msg=lambda m: f"{what}: {m}")
        sc0, sh0, mean0, inv0 = _bn_coeffs(y0, g0, be0, True, None, None)
        sc1, sh1, mean1, inv1 = _bn_coeffs(y1, g1, be1, True, None, None)
        sc2, sh2, mean2, inv2 = _bn_coeffs(y2, g2, be2, True, None, None)
        # the tables, from the forward graph alone: grid = per-cell maximum of the features rounded once to fp32 (what the scatter
        # kernels store; rounding is monotonic, so the float64 graph's ties and maxima survive it), holders = the rows of the cell
        # whose feature equals it, share = dout / holders -- ATen's even split among ties
        v = L.z32(y2, sc2, sh2).clamp_min(0)
        tgrid = torch.zeros(cells, C2).index_reduce_(0, rows[ok].long(), v[ok], "amax", include_self=True)
        holders = torch.zeros(cells, C2).index_add_(0, rows[ok].long(), (v[ok] == tgrid[rows[ok].long()]).float())
        assert set(holders[1, 3:].tolist()) >= {3.0, 14.0} and bool((tgrid[:10, 0:3] == 0).all()) and bool((holders[10:] == 0).all())
        share = dout / holders.double()                      # empty cells: 0 holders, inf -- never read into a result
        assert not bool(torch.isfinite(share[10:]).any()) and bool((share[:10, 0:3] != 0).all())
        G = L.table_grad(y2, rows, tgrid.double(), share, sc2, sh2)["G"][0]
        close(G, z2.grad, "table gradient vs d loss / d z2")
        assert bool((G[170:] == 0).all()) and int((G[17:20] != 0).all(0).sum()) > 0 and int((G[20:34] != 0).all(0).sum()) > 0 and bool((G[:, 0:3] == 0).all())
        al2, bb2, ga2 = _finalize(z2.grad, y2, g2, mean2, inv2, True)
        lay = L.l2_dgrad_layout(M, C2, C1, "tiled")
        res = L.l2_backward(y2, rows, tgrid.double(), share, al2, bb2, ga2, sc2, sh2, W2.t().contiguous(), y1, sc1, sh1, mean1, inv1,
                            L.slab_row_of(M, lay), lay["rows"], 0, 0)
        close(res["G1"][0], z1.grad, "G1")
        close(res["s1"][0], be1.grad, "BatchNorm-1 backward s1")
        close(res["s2"][0], g1.grad, "BatchNorm-1 backward s2")
        close(res["dW"][0], W2.grad, "dW2")
        close(res["s1_rows"][0].sum(0), be1.grad, "slab rows of s1")
        # layer 1, mask off (G = d loss / d z1) and on (G = d loss / d a1)
        al1, bb1, ga1 = _finalize(z1.grad, y1, g1, mean1, inv1, True)
        lay1 = L.l1_dgrad_layout(M, C1, C0)
        for Gin, mact, what in ((z1.grad, 0, "mask off"), (a1.grad, 1, "mask on")):
            r1 = L.l1_backward(Gin, y1, al1, bb1, ga1, sc1, sh1, mact, W1.t().contiguous(), pts, w0, b0, sc0, sh0, mean0, inv0,
                               L.slab_row_of(M, lay1), lay1["rows"], 0, 0, 0)
            close(r1["G0"][0], z0.grad, f"G0, {what}")
            close(r1["s1"][0], be0.grad, f"BatchNorm-0 backward s1, {what}")
            close(r1["s2"][0], g0.grad, f"BatchNorm-0 backward s2, {what}")
            close(r1["dW"][0], W1.grad, f"dW1, {what}")
            al0, bb0, ga0 = _finalize(z0.grad, y0, g0, mean0, inv0, True)
            close(al0[:, None] * r1["m1"][0].t() + (bb0 * y0 + ga0).t() @ pts, w0.grad, f"dW0 from the moments, {what}")


# ---- the bounds hold for honest fp32 -------------------------------------------------------------------------------------------

def _within(r32, r64, what, key):
    for k, (val, err) in r64.items():
        d = (r32[k][0].double() - val).abs()
        ratio = (d / err.clamp_min(1e-300))[d > 0].max().item() if bool((d > 0).any()) else 0.0
        WORST[(key, k)] = max(WORST.get((key, k), 0.0), ratio)
        assert ratio < 1.0, f"{what} [{k}]: fp32 evaluation {ratio:.3g}x the bound"


@pytest.mark.parametrize("N2,K1", L2_SHAPES)
@pytest.mark.parametrize("M", GENERAL_M)
def test_layer2_bounds_hold_for_fp32(M, N2, K1):
    for order in ("tail", "head"):
        sc = L.scene(M, N2, K1, order)
        for name, lay, n_red in _l2_layouts(M, N2, K1):
            _within(_l2_ref(sc, lay, n_red, None), _l2_ref(sc, lay, n_red, torch.float64), f"layer 2 {name} {(M, N2, K1)} {order}", "l2 " + name)


@pytest.mark.parametrize("N1,K0", L1_SHAPES)
@pytest.mark.parametrize("M", GENERAL_M)
def test_layer1_bounds_hold_for_fp32(M, N1, K0):
    d = L.l1_inputs(M, N1, K0)
    lay = L.l1_dgrad_layout(M, N1, K0)
    n_red = L.R.wgrad_tiled_layout(M, N1, K0, True)["n_red"]
    for mact in (0, 1):
        _within(_l1_ref(d, mact, lay, lay["n_m1"], n_red, None), _l1_ref(d, mact, lay, lay["n_m1"], n_red, torch.float64),
                f"layer 1 {(M, N1, K0)} mact={mact}", "l1 tiled")


@pytest.mark.parametrize("M", FUSED_M)
def test_fused_bounds_hold_for_fp32(M):
    sc = L.scene(M, 128, 128)
    f2 = L.fused_layout(M, 2)
    _within(_l2_ref(sc, f2, f2["n_red"], None), _l2_ref(sc, f2, f2["n_red"], torch.float64), f"kd_lidar_l2_bwd M={M}", "l2 fused")
    d = L.l1_inputs(M, 128, 64)
    f1 = L.fused_layout(M, 1)
    _within(_l1_ref(d, 0, f1, f1["n_m1"], f1["n_red"], None), _l1_ref(d, 0, f1, f1["n_m1"], f1["n_red"], torch.float64), f"kd_lidar_l1_bwd M={M}",
            "l1 fused")


# ---- the bounds have teeth -----------------------------------------------------------------------------------------------------

def _outside(wrong, ref, keys, what):
    for k in keys:
        val, err = ref[k]
        n = int(((wrong[k][0].double() - val).abs() > err).sum())
        assert n > 0, f"{what}: the wrong reading stays inside the bound of [{k}]"


@pytest.mark.parametrize("form", ["tiled", "stream", "fused"])
def test_teeth_of_the_layer2_bounds(form):
    M = 4133
    sc = L.scene(M, 128, 128)
    assert sc["full"]
    name, lay, n_red = next(l for l in _l2_layouts(M, 128, 128) if l[0] == form)
    ref = _l2_ref(sc, lay, n_red, torch.float64)
    every = ("G1", "s1_rows", "s2_rows", "dW")
    for mut, what in (("offgrid", "the off-grid mask dropped"), ("vpos", "v > 0 dropped"), ("tie", "one holder of a tie dropped"),
                      ("lastrow", "the last row dropped"), ("act1_ge", "the act1 mask taken from >= 0")):
        _outside(_l2_ref(sc, lay, n_red, None, mut={mut}), ref, every[:3] if mut == "act1_ge" else every, f"{form}: {what}")
    # be * Y2 dropped
    _outside(_l2_ref({**sc, "be": torch.zeros_like(sc["be"])}, lay, n_red, None), ref, every + ("s1", "s2"), f"{form}: be*Y dropped")
    # the last chunk (32 rows) attributed to the wrong slab row
    row = L.slab_row_of(M, lay).clone()
    row[-(M % 32 or 32):] = (row[-1] + 1) % lay["rows"]
    _outside(_l2_ref(sc, lay, n_red, None, slab_row=row), ref, ("s1_rows", "s2_rows"), f"{form}: the last chunk in the wrong slab row")


@pytest.mark.parametrize("form", ["tiled", "fused"])
def test_teeth_of_the_layer1_bounds(form):
    M = 4133
    d = L.l1_inputs(M, 128, 64)
    lay = L.l1_dgrad_layout(M, 128, 64) if form == "tiled" else L.fused_layout(M, 1)
    n_red = L.R.wgrad_tiled_layout(M, 128, 64, True)["n_red"] if form == "tiled" else lay["n_red"]
    ref = _l1_ref(d, 0, lay, lay["n_m1"], n_red, torch.float64)
    _outside(_l1_ref(d, 0, lay, lay["n_m1"], n_red, None, mut={"m1_coord"}), ref, ("m1",), f"{form}: one point coordinate dropped from m1")
    _outside(_l1_ref(d, 0, lay, lay["n_m1"], n_red, None, mut={"lastrow"}), ref, ("G0", "s1_rows", "s2_rows", "dW"), f"{form}: the last row dropped")
    _outside(_l1_ref({**d, "be": torch.zeros_like(d["be"])}, 0, lay, lay["n_m1"], n_red, None), ref, ("G0", "s1", "s2", "m1", "dW"), f"{form}: be*Y dropped")


def test_the_scene_holds_what_it_promises():
    for order in ("tail", "head"):
        sc = L.scene(4133, 128, 128, order)
        rows, Y2 = sc["rows"], sc["Y2"]
        inr = rows[rows >= 0]
        assert bool((inr[1:] >= inr[:-1]).all()) and set(rows[sc["off_rows"]].tolist()) == {-1, -2, L.INT_MIN}
        assert bool((rows[sc["off_rows"]] < 0).all()) and int((rows < 0).sum()) == sc["n_off"]
        G = L.table_grad(*(sc[k] for k in ("Y2", "rows", "grid", "share", "sc2", "sh2")))["G"][0]
        Gbad = L.table_grad(*(sc[k] for k in ("Y2", "rows", "grid", "share", "sc2", "sh2")), mut={"offgrid"})["G"][0]
        assert bool((G[sc["off_rows"]] == 0).all()) and int((Gbad[sc["off_rows"]] != 0).sum()) > 32 * sc["n_off"]
        t = sc["tie_rows"]
        assert bool((Y2[t.start + 5:t.stop] == Y2[t.start + 5]).all()) and int((G[t.start + 5:t.stop] != 0).all(0).sum()) > 32
        z = sc["zero_rows"]
        assert bool((sc["grid"][4, 0:4] == 0).all()) and sc["grid"][4, sc["SUB_CH"]] == 0 and bool((G[z, 0:4] == 0).all())
        assert bool((sc["share"][4] != 0).all())
        assert sc["grid"][sc["sub_cell"], sc["SUB_CH"]].item() == L.SUBNORMAL
        assert G[sc["sub_row"], sc["SUB_CH"]] == sc["share"][sc["sub_cell"], sc["SUB_CH"]] and bool((G[sc["sub_row"] + 1:sc["sub_row"] + 4, sc["SUB_CH"]] == 0).all())
        assert bool(torch.isnan(sc["share"][7]).all()) and bool(torch.isnan(sc["share"][-2:]).all()) and not bool(torch.isnan(G).any())
        z1 = L.z32(sc["Y1"], sc["sc1"], sc["sh1"])
        assert 0.3 < (z1 < 0).float().mean().item() < 0.7 and bool((z1[:, sc["OFF_CH"]] < 0).all()) and int((z1[:, sc["ZERO_CH"]] == 0).sum()) >= 4133 // 7


# ---- the layout mirrors equal the library's host-side answers ----------------------------------------------------------------

def test_layout_mirrors_equal_the_library():
    from kdrt.lib import lib
    prev_split, prev_stream = lib.kd_set_gemm_split(1), lib.kd_set_gemm_stream(2)
    try:
        for M in sorted(set(GENERAL_M + FUSED_M + (300000,))):
            for N2, K1 in L2_SHAPES:
                for mode, form in ((0, "tiled"), (2, "stream")):
                    lib.kd_set_gemm_stream(mode)
                    assert lib.kd_lidar_l2_dgrad_stat_rows(M, N2, K1) == L.l2_dgrad_layout(M, N2, K1, form)["rows"], (M, N2, K1, form)
                assert lib.kd_pwconv_wgrad_ws_bytes(M, N2, K1) == L.R.wgrad_ws_bytes(M, N2, K1)
            for N1, K0 in L1_SHAPES:
                lay = L.l1_dgrad_layout(M, N1, K0)
                assert lib.kd_lidar_l1_dgrad_stat_rows(M, N1, K0) == lay["rows"] == L.R.tiled_layout(M, K0, 2)["rows"], (M, N1, K0)
                assert lib.kd_lidar_l1_dgrad_ws_bytes(M, K0) == lay["m1_ws_bytes"], (M, K0)
                assert lay["m1_rows"] * 4 * K0 * 4 <= lay["m1_ws_bytes"]
            f2, f1 = L.fused_layout(M, 2), L.fused_layout(M, 1)
            assert lib.kd_lidar_l2_bwd_stat_rows(M) == f2["rows"] and lib.kd_lidar_l1_bwd_stat_rows(M) == f1["rows"]
            assert lib.kd_lidar_l2_bwd_ws_bytes(M, 128, 128) == f2["ws_bytes"] and lib.kd_lidar_l1_bwd_ws_bytes(M, 128, 64) == f1["ws_bytes"]
            lib.kd_set_gemm_split(0)
            lib.kd_set_gemm_stream(2)
            assert lib.kd_lidar_l2_dgrad_stat_rows(M, 128, 128) == L.l2_dgrad_layout(M, 128, 128, "stream", split=False)["rows"]
            lib.kd_set_gemm_split(1)
        assert (L.fused_layout(8193, 2)["nit"], L.fused_layout(8193, 2)["nit_min"]) == (2, 1), "workgroup 0 two chunks, the rest one"
        assert L.fused_layout(8225, 2)["nchunk"] == 258 and (L.fused_layout(32769, 2)["nit"], L.fused_layout(32769, 2)["nit_min"]) == (5, 4)
        assert 131072 * 128 * 4 == L.R.NT_BYTES and 131071 * 128 * 4 < L.R.NT_BYTES
    finally:
        lib.kd_set_gemm_split(prev_split)
        lib.kd_set_gemm_stream(prev_stream)
