"""The training backward of the LiDAR point MLP called directly through the C ABI -- kd_lidar_l2_dgrad (tiled PRO4 kernel and its
streaming instance), kd_lidar_l2_wgrad (DMODE 3), kd_lidar_l1_dgrad (PRO2 / EPI3, stored, moments-only and both), kd_lidar_l1_wgrad
(AMODE 2) and the one-kernel forms kd_lidar_l2_bwd / kd_lidar_l1_bwd, both arithmetics -- compared with a float64 evaluation of
the same operation on the same fp32 inputs (tests/_fp64_lidar_mlp_ref.py, plain torch on the GPU) within
C_BOUND * n_seq * 2^-24 * sum|t_i| per output: G1 / G0 element-wise, the BatchNorm-backward sums per slab row and in total, the
G0 * point moments, dW.  No element is left out of any comparison.

Every float output, slab, workspace and dW starts as NaN and carries a sentinel guard tail; strided cases take their operands as
column slices of wider NaN buffers and the output keeps its padding columns.  The layer-2 inputs are the adversarial scene of the
reference module at every M >= 128 (off-grid rows that carry a holder's features and rows entries -1, -2, INT_MIN, ties of 2, 3
and 40 rows across a chunk boundary, zero-maximum cells with non-zero shares, a subnormal maximum, NaN shares of empty cells,
exactly-zero pre-activations), in both row orders.  Every case asserts the mirror of the launch layout equal to the library's
answer (kd_lidar_l?_dgrad_stat_rows, kd_lidar_l?_bwd_stat_rows, kd_pwconv_wgrad_ws_bytes, kd_lidar_l?_bwd_ws_bytes,
kd_lidar_l1_dgrad_ws_bytes) and a streaming case that the switch changes the launch.  The one-kernel forms exist in split
arithmetic only: in fp32 arithmetic those cases assert *_supported == 0 and the "no instance" refusal, and skip.

test_table_rebuild_exactly: with W2 = I, al = 1, be = ga = 0 and act1 open the forms reduce to G1 = G up to the split product
x * 1, so holder selection is checked element by element against table_grad.  The subnormal-maximum channel must give `share`:
v = 2^-140 is positive and equals the cell's maximum, the same convention as kd_lidar_seg_share_bwd (holders are the rows with
v > 0 && v == max; fp32 denormals are kept by every kernel of the library).

Measured on an MI355X (see the RATIO / PROBE lines this module prints): this file 4.9 s of wall time
(112 cases, 23 of them the whole-arithmetic skips), next to 5.3 s for tests/test_gpu_gemm_shapes.py in the same session; no case above
0.2 s after the first.

Worst error / bound per kernel over all cases (split | fp32 arithmetic): pw_gemm_kernel<4, 2> G1 0.053 | 0.072, its sums 0.013 | 0.020;
pw_stream_kernel<.., 4, 2> G1 0.029, sums 0.006; pw_wgrad_kernel<.., 3, 1> dW2 0.022 | 0.023; pw_gemm_kernel<2, 3> G0 0.042 | 0.051
(256 x 64 tile), 0.015 | 0.025 (128 x 128), its sums 0.010 | 0.008, moments 0.003 | 0.005; pw_wgrad_kernel<.., 2, 2> dW1 0.018 | 0.019;
lidar_l2_bwd_kernel G1 0.030, sums 0.013, dW2 0.026; lidar_l1_bwd_kernel sums 0.003, moments 0.001, dW1 0.015.  Nothing near 0.5: the
bounds are worst-case chains, random rounding errors use a twentieth of them, a dropped mask, holder, row or term none
(tests/test_fp64_lidar_mlp_ref_host.py).  The table rebuild is exact in every form (worst |G1 - share| = 0, the subnormal maximum
included) and the three forms agree bit for bit.

Single products of the one-kernel forms, worst |got - x*y| / (U |x||y|): G1 2.48 over 1.05 M products, dW2 2.32 and dW1 1.83 over
131 k each -- inside the 3.97 U of include/kd_hip.h, the same figures as the tiled and streaming kernels (2.36 - 2.65)."""
import pytest
import torch

import _fp64_lidar_mlp_ref as L
from test_gpu_gemm_fp64 import SPLIT_PRODUCT_U, Out, _arith, _ld, _lib, _stream_mode, _wide
from test_gpu_tail_kernels import Buf

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]

R = L.R
GENERAL_M = (1, 33, 129, 4133)
L2_SHAPES = [(64, 128), (128, 128), (256, 128), (36, 40)]           # (N2, K1)
L1_SHAPES = [(128, 64), (128, 128), (40, 36)]                        # (N1, K0)
FUSED_M = (1, 31, 32, 33, 8193, 8225, 16461, 32769, 131071, 131072)
RELU, RELU6 = 1, 2
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("RATIO", *k, f"{WORST[k]:.4f}")


def _err():
    from kdrt.lib import KDError
    return KDError


def _check(what, key, got, ref):
    val, err = ref
    got = got.double().reshape(val.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements never written"
    d = (got - val).abs()
    r = (d / err.clamp_min(1e-300))[d > 0].max().item() if bool((d > 0).any()) else 0.0
    print(f"FIGURE {what}: worst error / bound {r:.4f}")
    WORST[key] = max(WORST.get(key, 0.0), r)
    if r > 1.0:
        bad = d > err
        i = int(torch.nonzero(bad.reshape(-1))[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {val.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                    f"got {got.reshape(-1)[i].item():.9g}, float64 {val.reshape(-1)[i].item():.9g}, bound {err.reshape(-1)[i].item():.3g}")


def _check_sums(what, key, part, ref):
    """the slab [rows][2][C]: every row within its bound, and the float64 sum of the rows"""
    part.guard_ok(f"{what} [statistics slab]")
    assert not bool(torch.isnan(part.t).any()), f"{what}: statistics slab rows never written: {torch.nonzero(torch.isnan(part.t).any(2).any(1)).flatten().tolist()}"
    _check(f"{what} [s1 per slab row]", key + ("s1 rows",), part.t[:, 0], ref["s1_rows"])
    _check(f"{what} [s2 per slab row]", key + ("s2 rows",), part.t[:, 1], ref["s2_rows"])
    st = part.t.double().sum(0)
    _check(f"{what} [s1]", key + ("s1",), st[0], ref["s1"])
    _check(f"{what} [s2]", key + ("s2",), st[1], ref["s2"])


def _w(t, strided, left=4, right=4):
    return _wide(t, left, right) if strided else t


# ---- launches ----------------------------------------------------------------------------------------------------------------

def _l2_dgrad(sc, G1, part, rows_n, M, N2, K1, strided=False, act2=RELU, act1=RELU):
    lib, P, stream = _lib()
    Y2, Y1 = _w(sc["Y2"], strided), _w(sc["Y1"], strided, 8, 0)
    lib.call("kd_lidar_l2_dgrad", P(Y2), _ld(Y2), P(sc["rows"]), P(sc["grid"]), P(sc["share"]), P(sc["al"]), P(sc["be"]), P(sc["ga"]), P(sc["sc2"]),
             P(sc["sh2"]), act2, P(sc["Wt"]), P(G1), _ld(G1), P(Y1), _ld(Y1), P(sc["sc1"]), P(sc["sh1"]), P(sc["mean1"]), P(sc["inv1"]), act1, P(part),
             rows_n, M, N2, K1, stream())
    torch.cuda.synchronize()


def _l2_wgrad(sc, M, N2, K1, what, strided=False, act2=RELU):
    lib, P, stream = _lib()
    nb = lib.kd_pwconv_wgrad_ws_bytes(M, N2, K1)
    assert nb == R.wgrad_ws_bytes(M, N2, K1), f"{what}: workspace of {nb} B, the mirror says {R.wgrad_ws_bytes(M, N2, K1)}"
    dW, ws = Buf(N2, K1), Buf(nb // 4)
    Y2, Y1 = _w(sc["Y2"], strided, 8, 4), _w(sc["Y1"], strided, 0, 8)
    lib.call("kd_lidar_l2_wgrad", P(Y2), _ld(Y2), P(sc["rows"]), P(sc["grid"]), P(sc["share"]), P(sc["al"]), P(sc["be"]), P(sc["ga"]), P(sc["sc2"]),
             P(sc["sh2"]), act2, P(Y1), _ld(Y1), P(sc["sc1"]), P(sc["sh1"]), RELU, P(dW.t), M, N2, K1, P(ws.t), nb, stream())
    torch.cuda.synchronize()
    dW.guard_ok(f"{what} [dW]")
    ws.guard_ok(f"{what} [workspace]")
    return dW.t


def _l2_fused_args(sc, G1, part, ldy2=128, ldg1=128, ldy1=128, act2=RELU, act1=RELU, Y2=None):
    P = _lib()[1]
    return (P(sc["Y2"] if Y2 is None else Y2), ldy2, P(sc["rows"]), P(sc["grid"]), P(sc["share"]), P(sc["al"]), P(sc["be"]), P(sc["ga"]), P(sc["sc2"]),
            P(sc["sh2"]), act2, P(sc["Wt"]), P(G1), ldg1, P(sc["Y1"]), ldy1, P(sc["sc1"]), P(sc["sh1"]), P(sc["mean1"]), P(sc["inv1"]), act1, P(part))


def _l2_fused(sc, M, what):
    """one kd_lidar_l2_bwd launch on NaN outputs -> (G1 [M + 4 rows], slab, dW)"""
    lib, P, stream = _lib()
    lay = L.fused_layout(M, 2)
    assert lib.kd_lidar_l2_bwd_stat_rows(M) == lay["rows"] and lib.kd_lidar_l2_bwd_ws_bytes(M, 128, 128) == lay["ws_bytes"], f"{what}: {lay}"
    G1, part, dW, ws = Buf(M + 4, 128), Buf(lay["rows"], 2, 128), Buf(128, 128), Buf(lay["ws_bytes"] // 4)
    lib.call("kd_lidar_l2_bwd", *_l2_fused_args(sc, G1.t, part.t), lay["rows"], P(dW.t), M, 128, 128, P(ws.t), lay["ws_bytes"], stream())
    torch.cuda.synchronize()
    for b, n in ((G1, "G1"), (dW, "dW"), (ws, "workspace")):
        b.guard_ok(f"{what} [{n}]")
    assert bool(torch.isnan(G1.t[M:]).all()), f"{what}: rows M .. M + 3 of G1 written"
    return G1.t[:M], part, dW.t, lay


def _l2_reference(sc, lay, n_red, M):
    return L.l2_backward(*L.l2_args(sc, torch.float64), L.slab_row_of(M, lay, "cuda"), lay["rows"], lay["n_part"], n_red)


# ---- layer 2, the general pair -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N2,K1", L2_SHAPES)
@pytest.mark.parametrize("M", GENERAL_M)
def test_layer2_general_pair(M, N2, K1):
    lib = _lib()[0]
    split = _arith() == "split"
    has_stream = (N2, K1) == (128, 128)
    for order in ("tail", "head"):
        sc = L.scene(M, N2, K1, order, device="cuda")
        for strided in (False, True):
            for form in (("tiled", "stream") if has_stream else ("tiled",)):
                with _stream_mode(2 if form == "stream" else 0):
                    what = f"layer 2 {(M, N2, K1)} rows {order}, {'strided' if strided else 'dense'}, {form}"
                    lay = L.l2_dgrad_layout(M, N2, K1, form, split)
                    rows_n = lib.kd_lidar_l2_dgrad_stat_rows(M, N2, K1)
                    assert rows_n == lay["rows"], f"{what}: the library writes {rows_n} statistics rows, the mirror says {lay}"
                    if form == "stream":
                        with _stream_mode(0):
                            r0 = lib.kd_lidar_l2_dgrad_stat_rows(M, N2, K1)
                        if not split:
                            assert r0 == rows_n, "a streaming instance in fp32 arithmetic?"
                            continue            # (the tiled form of this case has just run)
                        assert lay["form"] == "stream" and (r0 != rows_n or M <= 128), f"{what}: the streaming switch does not change the launch"
                    name = "pw_stream_kernel<pro 4>" if lay["form"] == "stream" else "pw_gemm_kernel<pro 4>"
                    key = (_arith(), name)
                    G1, part = Out(M, K1, 4 if strided else 0), Buf(rows_n, 2, K1)
                    _l2_dgrad(sc, G1.t, part.t, rows_n, M, N2, K1, strided)
                    G1.intact(what)
                    ref = _l2_reference(sc, lay, R.wgrad_tiled_layout(M, N2, K1, split)["n_red"], M)
                    _check(f"[{name} {_arith()}] {what} [G1]", key + ("G1",), G1.t, ref["G1"])
                    _check_sums(f"[{name} {_arith()}] {what}", key, part, ref)
            wl = R.wgrad_tiled_layout(M, N2, K1, split)
            wname = f"pw_wgrad_kernel<{wl['wn']},{wl['wk']},{wl['wm']},dmode 3>"
            what = f"[{wname} {_arith()}] layer 2 {(M, N2, K1)} rows {order}, {'strided' if strided else 'dense'}"
            _check(f"{what} [dW2]", (_arith(), wname, "dW"), _l2_wgrad(sc, M, N2, K1, what, strided), ref["dW"])
    # the holder split is ReLU's: ReLU6 is refused by both
    G1, part = Buf(M, K1), Buf(rows_n, 2, K1)
    with pytest.raises(_err(), match="ReLU6"):
        _l2_dgrad(sc, G1.t, part.t, rows_n, M, N2, K1, act2=RELU6)
    with pytest.raises(_err(), match="ReLU6"):
        _l2_wgrad(sc, M, N2, K1, "ReLU6", act2=RELU6)
    assert bool(torch.isnan(G1.t).all()) and bool(torch.isnan(part.t).all()), "a refused launch wrote its outputs"


# ---- layer 1, the general pair -------------------------------------------------------------------------------------------------

def _l1_dgrad(d, mact, G0, part, rows_n, m1, m1_ws, m1_bytes, M, N1, K0, strided=False):
    lib, P, stream = _lib()
    G, Y1 = _w(d["G"], strided), _w(d["Y1"], strided, 8, 0)
    lib.call("kd_lidar_l1_dgrad", P(G), _ld(G), P(Y1), _ld(Y1), P(d["al"]), P(d["be"]), P(d["ga"]), P(d["msc"]) if mact else None,
             P(d["msh"]) if mact else None, mact, P(d["Wt"]), P(G0), _ld(G0) if G0 is not None else K0, P(d["pts"]), P(d["w0"]), P(d["b0"]),
             P(d["sc0"]), P(d["sh0"]), P(d["mean0"]), P(d["inv0"]), RELU, P(part), rows_n, P(m1), P(m1_ws), m1_bytes, M, N1, K0, stream())
    torch.cuda.synchronize()


def _l1_wgrad(d, mact, M, N1, K0, what, strided=False):
    lib, P, stream = _lib()
    nb = lib.kd_pwconv_wgrad_ws_bytes(M, N1, K0)
    assert nb == R.wgrad_ws_bytes(M, N1, K0), f"{what}: workspace of {nb} B, the mirror says {R.wgrad_ws_bytes(M, N1, K0)}"
    dW, ws = Buf(N1, K0), Buf(nb // 4)
    G, Y1 = _w(d["G"], strided, 8, 4), _w(d["Y1"], strided, 0, 8)
    lib.call("kd_lidar_l1_wgrad", P(G), _ld(G), P(Y1), _ld(Y1), mact, P(d["al"]), P(d["be"]), P(d["ga"]), P(d["msc"]) if mact else None,
             P(d["msh"]) if mact else None, P(d["pts"]), P(d["w0"]), P(d["b0"]), P(d["sc0"]), P(d["sh0"]), RELU, P(dW.t), M, N1, K0, P(ws.t), nb, stream())
    torch.cuda.synchronize()
    dW.guard_ok(f"{what} [dW]")
    ws.guard_ok(f"{what} [workspace]")
    return dW.t


def _l1_reference(d, mact, lay, n_m1, n_red, M):
    return L.l1_backward(*L.l1_args(d, mact, torch.float64), L.slab_row_of(M, lay, "cuda"), lay["rows"], lay["n_part"], n_m1, n_red)


@pytest.mark.parametrize("N1,K0", L1_SHAPES)
@pytest.mark.parametrize("M", GENERAL_M)
def test_layer1_general_pair(M, N1, K0):
    lib = _lib()[0]
    split = _arith() == "split"
    d = L.l1_inputs(M, N1, K0, device="cuda")
    lay = L.l1_dgrad_layout(M, N1, K0)
    for mode in (0, 2):         # no streaming instance for epi 3: the tiled layout in every mode
        with _stream_mode(mode):
            rows_n = lib.kd_lidar_l1_dgrad_stat_rows(M, N1, K0)
            assert rows_n == lay["rows"] == R.tiled_layout(M, K0, 2)["rows"], f"kd_lidar_l1_dgrad_stat_rows({M}, {N1}, {K0}) = {rows_n}, tiled layout {lay}"
    nbm = lib.kd_lidar_l1_dgrad_ws_bytes(M, K0)
    assert nbm == lay["m1_ws_bytes"] and lay["m1_rows"] * 16 * K0 <= nbm, f"moment workspace of {nbm} B, the mirror says {lay}"
    wl = R.wgrad_tiled_layout(M, N1, K0, split)
    name = f"pw_gemm_kernel<pro 2, epi 3, {lay['bm']}x{lay['bn']}>"
    wname = f"pw_wgrad_kernel<{wl['wn']},{wl['wk']},{wl['wm']},amode 2>"
    for mact in (0, RELU):
        ref = _l1_reference(d, mact, lay, lay["n_m1"], wl["n_red"], M)
        for strided in (False, True):
            parts, m1s = {}, {}
            for outputs in ("stored", "moments", "both"):
                what = f"[{name} {_arith()}] layer 1 {(M, N1, K0)} mact={mact}, {'strided' if strided else 'dense'}, {outputs}"
                key = (_arith(), name)
                G0 = Out(M, K0, 4 if strided else 0) if outputs != "moments" else None
                m1, m1_ws = (Buf(4, K0), Buf(nbm // 4)) if outputs != "stored" else (None, None)
                part = Buf(rows_n, 2, K0)
                _l1_dgrad(d, mact, None if G0 is None else G0.t, part.t, rows_n, None if m1 is None else m1.t, None if m1 is None else m1_ws.t,
                          nbm if m1 is not None else 0, M, N1, K0, strided)
                if G0 is not None:
                    G0.intact(what)
                    _check(f"{what} [G0]", key + ("G0",), G0.t, ref["G0"])
                _check_sums(what, key, part, ref)
                parts[outputs] = part.t.clone()
                if m1 is not None:
                    m1.guard_ok(f"{what} [m1]")
                    m1_ws.guard_ok(f"{what} [moment workspace]")
                    _check(f"{what} [m1]", key + ("m1",), m1.t, ref["m1"])
                    m1s[outputs] = m1.t.clone()
            assert torch.equal(parts["stored"], parts["moments"]) and torch.equal(parts["stored"], parts["both"]), f"layer 1 {(M, N1, K0)}: the sums depend on the output form"
            assert torch.equal(m1s["moments"], m1s["both"]), f"layer 1 {(M, N1, K0)}: the moments depend on the output form"
            what = f"[{wname} {_arith()}] layer 1 {(M, N1, K0)} mact={mact}, {'strided' if strided else 'dense'}"
            _check(f"{what} [dW1]", (_arith(), wname, "dW"), _l1_wgrad(d, mact, M, N1, K0, what, strided), ref["dW"])


# ---- the one-kernel forms --------------------------------------------------------------------------------------------------------

def _fused_only(layer):
    """fp32 arithmetic: no instance, said twice -- by *_supported and by the launch -- then the whole-arithmetic skip"""
    lib, P, stream = _lib()
    if _arith() == "split":
        return
    M = 33
    if layer == 2:
        assert lib.kd_lidar_l2_bwd_supported(128, 128) == 0
        sc = L.scene(M, 128, 128, device="cuda")
        G1, part, dW, ws = Buf(M, 128), Buf(2, 2, 128), Buf(128, 128), Buf(1 << 16)
        with pytest.raises(_err(), match="no instance"):
            lib.call("kd_lidar_l2_bwd", *_l2_fused_args(sc, G1.t, part.t), 2, P(dW.t), M, 128, 128, P(ws.t), 4 << 16, stream())
    else:
        assert lib.kd_lidar_l1_bwd_supported(128, 64) == 0
        d = L.l1_inputs(M, 128, 64, device="cuda")
        part, m1, dW, ws = Buf(2, 2, 64), Buf(4, 64), Buf(128, 64), Buf(1 << 16)
        with pytest.raises(_err(), match="no instance"):
            lib.call("kd_lidar_l1_bwd", *_l1_fused_args(d, part.t), 2, P(m1.t), P(dW.t), M, 128, 64, P(ws.t), 4 << 16, stream())
    pytest.skip("the one-kernel backward exists in the split arithmetic only")


@pytest.mark.parametrize("M", FUSED_M)
def test_layer2_one_kernel(M):
    _fused_only(2)
    lib, P, stream = _lib()
    assert lib.kd_lidar_l2_bwd_supported(128, 128) and not lib.kd_lidar_l2_bwd_supported(64, 128)
    sc = L.scene(M, 128, 128, device="cuda")
    what = f"[lidar_l2_bwd_kernel<{'NT' if M * 512 >= R.NT_BYTES else 'plain'}>] M={M}"
    G1, part, dW, lay = _l2_fused(sc, M, what)
    ref = _l2_reference(sc, lay, lay["n_red"], M)
    key = ("split", "lidar_l2_bwd_kernel")
    _check(f"{what} [G1]", key + ("G1",), G1, ref["G1"])
    _check_sums(what, key, part, ref)
    _check(f"{what} [dW2]", key + ("dW",), dW, ref["dW"])
    # the existing claim, kept: G1 has the bits of kd_lidar_l2_dgrad (whichever form the dispatcher takes)
    rows_d = lib.kd_lidar_l2_dgrad_stat_rows(M, 128, 128)
    G1d, part_d = Buf(M, 128), Buf(rows_d, 2, 128)
    _l2_dgrad(sc, G1d.t, part_d.t, rows_d, M, 128, 128)
    assert torch.equal(G1d.t, G1), f"{what}: G1 differs from kd_lidar_l2_dgrad in {int((G1d.t != G1).sum())} elements"
    # refusals: nothing is launched, nothing is written
    G1r, part_r, dWr, ws = Buf(M, 128), Buf(lay["rows"], 2, 128), Buf(128, 128), Buf(lay["ws_bytes"] // 4)
    Y2w = _wide(sc["Y2"])
    for match, args, rows_n, nb in (("dense", _l2_fused_args(sc, G1r.t, part_r.t, ldy2=_ld(Y2w), Y2=Y2w), lay["rows"], lay["ws_bytes"]),
                                    ("dense", _l2_fused_args(sc, G1r.t, part_r.t, ldg1=132), lay["rows"], lay["ws_bytes"]),
                                    ("statistics slab", _l2_fused_args(sc, G1r.t, part_r.t), lay["rows"] + 1, lay["ws_bytes"]),
                                    ("statistics slab", _l2_fused_args(sc, G1r.t, part_r.t), lay["rows"] - 1, lay["ws_bytes"]),
                                    ("workspace too small", _l2_fused_args(sc, G1r.t, part_r.t), lay["rows"], lay["ws_bytes"] - 4),
                                    ("ReLU", _l2_fused_args(sc, G1r.t, part_r.t, act1=0), lay["rows"], lay["ws_bytes"]),
                                    ("ReLU", _l2_fused_args(sc, G1r.t, part_r.t, act2=RELU6), lay["rows"], lay["ws_bytes"])):
        with pytest.raises(_err(), match=match):
            lib.call("kd_lidar_l2_bwd", *args, rows_n, P(dWr.t), M, 128, 128, P(ws.t), nb, stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b.t).all()) for b in (G1r, part_r, dWr, ws)), f"{what}: a refused launch wrote its outputs"


def _l1_fused_args(d, part, ldg=128, ldy=128, act0=RELU, G=None):
    P = _lib()[1]
    return (P(d["G"] if G is None else G), ldg, P(d["Y1"]), ldy, P(d["al"]), P(d["be"]), P(d["ga"]), P(d["Wt"]), P(d["pts"]), P(d["w0"]), P(d["b0"]),
            P(d["sc0"]), P(d["sh0"]), P(d["mean0"]), P(d["inv0"]), act0, P(part))


def _l1_fused(d, M, what):
    lib, P, stream = _lib()
    lay = L.fused_layout(M, 1)
    assert lib.kd_lidar_l1_bwd_stat_rows(M) == lay["rows"] and lib.kd_lidar_l1_bwd_ws_bytes(M, 128, 64) == lay["ws_bytes"], f"{what}: {lay}"
    part, m1, dW, ws = Buf(lay["rows"], 2, 64), Buf(4, 64), Buf(128, 64), Buf(lay["ws_bytes"] // 4)
    lib.call("kd_lidar_l1_bwd", *_l1_fused_args(d, part.t), lay["rows"], P(m1.t), P(dW.t), M, 128, 64, P(ws.t), lay["ws_bytes"], stream())
    torch.cuda.synchronize()
    for b, n in ((m1, "m1"), (dW, "dW"), (ws, "workspace")):
        b.guard_ok(f"{what} [{n}]")
    return part, m1.t, dW.t, lay


@pytest.mark.parametrize("M", FUSED_M)
def test_layer1_one_kernel(M):
    _fused_only(1)
    lib, P, stream = _lib()
    assert lib.kd_lidar_l1_bwd_supported(128, 64) and not lib.kd_lidar_l1_bwd_supported(128, 128)
    d = L.l1_inputs(M, 128, 64, device="cuda")
    what = f"[lidar_l1_bwd_kernel] M={M}"
    part, m1, dW, lay = _l1_fused(d, M, what)
    ref = _l1_reference(d, 0, lay, lay["n_m1"], lay["n_red"], M)
    key = ("split", "lidar_l1_bwd_kernel")
    _check_sums(what, key, part, ref)
    _check(f"{what} [m1]", key + ("m1",), m1, ref["m1"])
    _check(f"{what} [dW1]", key + ("dW",), dW, ref["dW"])
    part_r, m1r, dWr, ws = Buf(lay["rows"], 2, 64), Buf(4, 64), Buf(128, 64), Buf(lay["ws_bytes"] // 4)
    Gw = _wide(d["G"])
    for match, args, rows_n, nb in (("dense", _l1_fused_args(d, part_r.t, ldg=_ld(Gw), G=Gw), lay["rows"], lay["ws_bytes"]),
                                    ("dense", _l1_fused_args(d, part_r.t, ldy=132), lay["rows"], lay["ws_bytes"]),
                                    ("statistics slab", _l1_fused_args(d, part_r.t), lay["rows"] + 1, lay["ws_bytes"]),
                                    ("workspace too small", _l1_fused_args(d, part_r.t), lay["rows"], lay["ws_bytes"] - 4),
                                    ("ReLU", _l1_fused_args(d, part_r.t, act0=0), lay["rows"], lay["ws_bytes"]),
                                    ("ReLU", _l1_fused_args(d, part_r.t, act0=RELU6), lay["rows"], lay["ws_bytes"])):
        with pytest.raises(_err(), match=match):
            lib.call("kd_lidar_l1_bwd", *args, rows_n, P(m1r.t), P(dWr.t), M, 128, 64, P(ws.t), nb, stream())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(b.t).all()) for b in (part_r, m1r, dWr, ws)), f"{what}: a refused launch wrote its outputs"


# ---- the table rebuild, element by element ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["tail", "head"])
@pytest.mark.parametrize("M", [4133, 16461])
def test_table_rebuild_exactly(M, order):
    """W2 = I, al = 1, be = ga = 0, act1 open (sc1 = 0, sh1 = 1): dy = fmaf(1, G, fmaf(0, Y2, 0)) = G and G1 = G . I, one product
    x * 1 per element and exact zeros otherwise.  So G1 must be 0 exactly where table_grad says 0 (every off-grid row, every
    loser of a maximum, every zero-maximum cell) and `share` within the split product's error where it says share (every row of a
    tie; the holder of the subnormal maximum 2^-140), and the forms must agree bit for bit."""
    lib = _lib()[0]
    split = _arith() == "split"
    sc = L.scene(M, 128, 128, order, device="cuda")
    assert sc["full"] and L.fused_layout(16461, 2)["nit"] == 3
    z, o = torch.zeros(128, device="cuda"), torch.ones(128, device="cuda")
    sc = {**sc, "Wt": torch.eye(128, device="cuda"), "al": o, "be": z, "ga": z, "sc1": z, "sh1": o}
    G = L.table_grad(*(sc[k] for k in ("Y2", "rows", "grid", "share", "sc2", "sh2")))["G"][0]
    # what the scene promises, on the reference itself
    SUB, sub = sc["SUB_CH"], sc["sub_row"]
    assert bool((G[sc["off_rows"]] == 0).all()) and not bool(torch.isnan(G).any())
    assert int((G[sc["tie_rows"]] != 0).sum()) > 45 * 32 and bool((G[sc["zero_rows"], 0:4] == 0).all()) and bool((G[sc["zero_rows"], SUB] == 0).all())
    assert G[sub, SUB] == sc["share"][sc["sub_cell"], SUB] != 0 and bool((G[sub + 1:sub + 4, SUB] == 0).all())
    got = {}
    for form in (("tiled", "stream", "fused") if split else ("tiled",)):
        what = f"[{form} {_arith()}] table rebuild M={M} rows {order}"
        if form == "fused":
            got[form] = _l2_fused(sc, M, what)[0]
        else:
            with _stream_mode(2 if form == "stream" else 0):
                lay = L.l2_dgrad_layout(M, 128, 128, form, split)
                assert lay["form"] == form and lib.kd_lidar_l2_dgrad_stat_rows(M, 128, 128) == lay["rows"]
                G1, part = Buf(M, 128), Buf(lay["rows"], 2, 128)
                _l2_dgrad(sc, G1.t, part.t, lay["rows"], M, 128, 128)
                G1.guard_ok(what)
                got[form] = G1.t
        g1 = got[form]
        assert not bool(torch.isnan(g1).any()), f"{what}: elements never written"
        wrong = (g1 != 0) != (G != 0)
        assert not bool(wrong.any()), (f"{what}: holder selection differs from table_grad at {int(wrong.sum())} elements; first (row, channel) "
                                       f"{torch.nonzero(wrong)[0].tolist()}, rows entry {int(sc['rows'][torch.nonzero(wrong)[0][0]])}")
        ratio = ((g1.double() - G.double()).abs() / (R.U * G.double().abs()).clamp_min(1e-300))[G != 0].max().item()
        print(f"PROBE {what}: worst |G1 - share| / (U |share|) = {ratio:.4f}")
        assert ratio <= (SPLIT_PRODUCT_U if split else 0.0), f"{what}: a selected share is off by {ratio:.3g} U"
        assert bool((g1[sc["off_rows"]] == 0).all()), f"{what}: an off-grid row took a share"
        assert g1[sub, SUB] != 0 and abs(g1[sub, SUB].item() - G[sub, SUB].item()) <= SPLIT_PRODUCT_U * R.U * abs(G[sub, SUB].item()), \
            f"{what}: the holder of the subnormal maximum 2^-140 must take its cell's share {G[sub, SUB].item()}, got {g1[sub, SUB].item()}"
    for form in got:
        assert torch.equal(got[form], got["tiled"]), f"table rebuild M={M}: {form} and tiled differ in {int((got[form] != got['tiled']).sum())} elements"


def test_scene_tables_agree_with_the_scatter_kernels():
    """The tables of the scene are the ones the scatter kernels would hand to these GEMMs: kd_lidar_seg_max_fwd gives the scene's
    grid bit for bit (the subnormal maximum 2^-140 and the zero maxima included) and kd_lidar_seg_share_bwd gives dout / holders
    wherever the maximum is positive -- dout itself for the single holder of the subnormal maximum, dout / 40 in the tie cell."""
    lib, P, stream = _lib()
    M, C = 4133, 128
    sc = L.scene(M, C, C, "tail", device="cuda")
    cells, n_in, SUB = sc["cells"], sc["n_in"], sc["SUB_CH"]
    srow = sc["rows"].clamp_min(-1).contiguous()                      # as kd_lidar_sort_points leaves the tail
    start = torch.zeros(cells + 1, dtype=torch.int32, device="cuda")
    start[1:] = torch.bincount(srow[:n_in].long(), minlength=cells).cumsum(0).to(torch.int32)
    assert int(start[-1]) == n_in
    g = torch.Generator(device="cuda").manual_seed(9)
    dout = L.rnd(g, cells, C)
    z = torch.zeros(C, device="cuda")
    grid, share, cnt = Buf(cells, C), Buf(cells, C), Buf(cells, C)
    part = Buf(lib.kd_lidar_seg_share_stat_rows(cells, M), 2, C)
    lib.call("kd_lidar_seg_max_fwd", P(sc["Y2"]), P(sc["sc2"]), P(sc["sh2"]), RELU, P(start), None, P(srow), P(grid.t), M, cells, C, stream())
    torch.cuda.synchronize()
    grid.guard_ok("kd_lidar_seg_max_fwd")
    assert torch.equal(grid.t, sc["grid"]), f"kd_lidar_seg_max_fwd differs from the scene's grid in {int((grid.t != sc['grid']).sum())} elements"
    assert grid.t[sc["sub_cell"], SUB].item() == L.SUBNORMAL
    lib.call("kd_lidar_seg_share_bwd", P(sc["Y2"]), P(sc["sc2"]), P(sc["sh2"]), RELU, P(grid.t), P(dout), P(z), P(z), P(start), P(srow), P(share.t),
             P(cnt.t), P(part.t), M, cells, C, stream())
    torch.cuda.synchronize()
    for b, n in ((share, "share"), (cnt, "count workspace"), (part, "statistics slab")):
        b.guard_ok(f"kd_lidar_seg_share_bwd [{n}]")
    v = L.z32(sc["Y2"], sc["sc2"], sc["sh2"]).clamp_min(0)[:n_in]
    cell = srow[:n_in].long()
    holders = torch.zeros(cells, C, device="cuda").index_add_(0, cell, ((v > 0) & (v == sc["grid"][cell])).float())
    pos = sc["grid"] > 0
    assert bool((holders[pos] >= 1).all()) and holders[sc["sub_cell"], SUB] == 1 and int(holders[3].max()) == 40
    want = dout.double() / holders.double().clamp_min(1)
    d = (share.t.double() - want).abs()[pos]
    assert not bool(torch.isnan(share.t[pos]).any()) and bool((d <= L.C_BOUND * 2 * L.U * want.abs()[pos]).all()), \
        f"kd_lidar_seg_share_bwd: share != dout / holders, worst {(d / (L.U * want.abs()[pos])).max().item():.3g} U"
    assert share.t[sc["sub_cell"], SUB] == dout[sc["sub_cell"], SUB], "the single holder of the subnormal maximum takes the whole dout"


# ---- one product per output element ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("output", ["G1", "dW2", "dW1"])
def test_single_product(output):
    """One non-zero per reduction, full 24-bit random mantissas, exponents -8 .. 8, for the one-kernel forms: every output element
    is one product x * y and every other accumulation an exact add of zero.  G1: dy = Y2 (al = 0, be = 1) one-hot per row.
    dW2: dy = diag(x) over 128 rows, a1 = relu(Y1) with positive Y1.  dW1: dy1 = G = diag(x), a0 = relu(point coordinate)
    (w0 one-hot, b0 = 0, sc0 = 1, sh0 = 0: layer 0 and its affine are exact)."""
    if _arith() != "split":
        _fused_only(2 if output != "dW1" else 1)
    g = torch.Generator(device="cuda").manual_seed(101 + len(output) + ord(output[-1]))
    z, o = torch.zeros(128, device="cuda"), torch.ones(128, device="cuda")
    got, exact = [], []
    if output == "G1":
        M = 8192
        x, W = R.probe_values(g, M), R.probe_values(g, 128, 128)
        col = torch.arange(M, device="cuda") % 128
        Y2 = torch.zeros(M, 128, device="cuda")
        Y2[torch.arange(M, device="cuda"), col] = x
        sc = dict(Y2=Y2, rows=torch.full((M,), -1, dtype=torch.int32, device="cuda"), grid=torch.zeros(1, 128, device="cuda"),
                  share=torch.ones(1, 128, device="cuda"), al=z, be=o, ga=z, sc2=o, sh2=z, Wt=W, Y1=torch.zeros(M, 128, device="cuda"), sc1=z, sh1=o,
                  mean1=z, inv1=o)
        got.append(_l2_fused(sc, M, "single product G1")[0])
        exact.append(x.double()[:, None] * W.double()[:, col].t())
    else:
        M = 128
        for _ in range(8 if output == "dW2" else 16):
            x = R.probe_values(g, M)
            if output == "dW2":
                A = R.probe_values(g, M, 128).abs()
                sc = dict(Y2=torch.diag(x), rows=torch.full((M,), -1, dtype=torch.int32, device="cuda"), grid=torch.zeros(1, 128, device="cuda"),
                          share=torch.ones(1, 128, device="cuda"), al=z, be=o, ga=z, sc2=o, sh2=z, Wt=torch.zeros(128, 128, device="cuda"), Y1=A, sc1=o,
                          sh1=z, mean1=z, inv1=o)
                got.append(_l2_fused(sc, M, "single product dW2")[2].clone())
                exact.append(x.double()[:, None] * A.double())
            else:
                pts = R.probe_values(g, M, 4).abs()
                w0 = torch.zeros(64, 4, device="cuda")
                w0[torch.arange(64, device="cuda"), torch.arange(64, device="cuda") % 4] = 1.0
                d = dict(G=torch.diag(x), Y1=torch.zeros(M, 128, device="cuda"), al=o, be=z, ga=z, Wt=torch.zeros(64, 128, device="cuda"), pts=pts, w0=w0,
                         b0=z[:64], sc0=o[:64], sh0=z[:64], mean0=z[:64], inv0=o[:64])
                got.append(_l1_fused(d, M, "single product dW1")[2].clone())
                exact.append(x.double()[:, None] * pts.double()[:, torch.arange(64, device="cuda") % 4])
    got, exact = torch.cat(got).double(), torch.cat(exact)
    assert not bool(torch.isnan(got).any()), f"[{output}] elements never written"
    ratio = ((got - exact).abs() / (R.U * exact.abs())).max().item()
    print(f"\nPROBE split one-kernel {output} worst |got - x*y| / (U |x||y|) = {ratio:.4f} over {exact.numel()} products")
    assert ratio <= SPLIT_PRODUCT_U, f"[{output}] per-product error {ratio:.4f} U |x||y| exceeds {SPLIT_PRODUCT_U} U |x||y|"
