"""The 1x1-convolution GEMM family called directly through the C ABI -- pw_gemm_kernel (128 x 128 and 256 x 64 tiles),
pw_stream_kernel, pw_wgrad_kernel, pw_wgrad_rs_kernel, both arithmetics -- compared element-wise with a float64 evaluation of the
same operation on the same fp32 inputs (tests/_fp64_gemm_ref.py, plain torch on the GPU) within C_BOUND * n_seq * 2^-24 * sum|t_i|
per output, plus kd_transpose_batch and kd_copy_segments bit for bit.  No element is left out of any comparison.

Outputs, statistics slabs, dW and workspaces start as NaN and carry a sentinel guard tail; strided outputs keep their padding
columns; operands are column slices of wider NaN buffers.  The kernel form is chosen with the process-wide switches
(kd_set_gemm_stream, kd_set_wgrad_rs; restored afterwards) and every case asserts that the library selects the form it names:
the mirror of the launch layout equals kd_pwconv_stat_rows_for / kd_pwconv_wgrad_ws_bytes, and a streaming case's row count
differs from the tiled one.  The streaming and role-specialised forms exist in split arithmetic only: in fp32 arithmetic those
cases assert that the dispatcher has no such instance and skip.

Kernel -> tests: test_forward (every prologue / epilogue, both tile shapes on NaN slabs, every (K / 32, N tile / 32) streaming
instance), test_forward_m_dev, test_data_gradient, test_weight_gradient, test_looping_and_non_temporal (waves that own several
slabs, three column tiles, C on both sides of the non-temporal threshold; streaming and tiled C bit for bit),
test_single_product (one non-zero per reduction: |got - x*y| <= SPLIT_PRODUCT_U * U |x||y| in split arithmetic, U |x||y| in fp32),
test_transpose_batch, test_copy_segments.

Measured on an MI355X: this file 6.9 s of wall time (250 cases, 40 of them the whole-arithmetic skips), next to 5.5 s for
tests/test_gpu_gemm_shapes.py in the same session; no case above 0.2 s after the first.

Single products, worst |got - x*y| / (U |x||y|) over 1.05-1.18 M products per kernel form: split arithmetic pw_gemm_kernel<128x128>
2.52, pw_gemm_kernel<256x64> 2.44, pw_stream_kernel 2.65, pw_wgrad_kernel 2.36, pw_wgrad_rs_kernel 2.37; fp32 arithmetic 0.998 /
0.999 / 0.999 (the two tile shapes, pw_wgrad_kernel).  The six products, smallest first, therefore do NOT meet the 2 U the header
used to promise (a sequentially nearest-rounded emulation gives 1.55-1.67 U: the instruction's own accumulation rounds less
tightly); the documented figure and SPLIT_PRODUCT_U are now 1.5 x the worst measured, 3.97 U.

Worst error / bound per kernel form over all cases (split | fp32 arithmetic): C 0.10 | 0.08 (pw_gemm_kernel<256x64>, epi 5), 0.06 |
0.07 (pw_gemm_kernel<128x128>), 0.06 (pw_stream_kernel); forward statistics 0.03 | 0.03; data-gradient sums 0.009 | 0.011; dW 0.017 |
0.021 (pw_wgrad_kernel), 0.019 (pw_wgrad_rs_kernel); the looping cases 0.06 (C) and 0.002 (sums).  The bounds are worst-case chains:
random rounding errors use a tenth of them, a dropped term, row or mask none (tests/test_fp64_gemm_ref_host.py)."""
from contextlib import contextmanager

import pytest
import torch

import _fp64_gemm_ref as R
from test_gpu_tail_kernels import NAN, Buf

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]

PADV = 7.0                  # padding columns of a strided output
SPLIT_PRODUCT_U = 3.97      # include/kd_hip.h: error <= 3.97 * 2^-24 |x||y| per product in split arithmetic (1.5 x the worst measured)
WORST = {}                  # (arithmetic, kernel form, output) -> worst error / bound seen in this session


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("RATIO", *k, f"{WORST[k]:.4f}")


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _arith():
    from kdrt import ops
    return ops.get_gemm_arithmetic()


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _d(t):
    if isinstance(t, (tuple, list)):
        return tuple(_d(v) for v in t)
    if isinstance(t, dict):
        return {k: _d(v) for k, v in t.items()}
    return t.double() if torch.is_tensor(t) else t


def _wide(t, left=4, right=4):
    """t [M, n] as a column slice of a wider NaN buffer (row stride != width)"""
    if t is None:
        return None
    M, n = t.shape
    buf = torch.full((M, left + n + right), NAN, device=t.device)
    buf[:, left:left + n] = t
    return buf[:, left:left + n]


def _ld(t):
    return 0 if t is None else t.stride(0)


class Out:
    """a NaN [M, N] output inside a [M, N + pad] buffer whose padding columns must stay as they are, with a guard tail"""

    def __init__(self, M, N, pad=4):
        self.b, self.N = Buf(M, N + pad), N
        self.b.t[:, N:] = PADV
        self.t = self.b.t[:, :N]

    def intact(self, what):
        self.b.guard_ok(what)
        assert bool((self.b.t[:, self.N:] == PADV).all()), f"{what}: padding columns of the output written"


def _check(what, key, got, ref):
    val, err = ref
    got = got.double().reshape(val.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements never written"
    d = (got - val).abs()
    r = (d / err.clamp_min(1e-300)).max().item() if d.numel() else 0.0
    WORST[key] = max(WORST.get(key, 0.0), r)
    if r > 1.0:
        bad = d > err
        i = int(torch.nonzero(bad.reshape(-1))[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {val.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                    f"got {got.reshape(-1)[i].item():.9g}, float64 {val.reshape(-1)[i].item():.9g}, bound {err.reshape(-1)[i].item():.3g}")


def _shares(x, sc, sh, what):
    if x.numel() >= 4096:
        lo, mid, hi = R.relu6_shares(x, sc, sh)
        assert min(lo, mid, hi) >= 0.01, f"ReLU6 inputs must exercise both clamps {what}: {lo:.3f} / {mid:.3f} / {hi:.3f}"


@contextmanager
def _stream_mode(mode):
    lib = _lib()[0]
    prev = lib.kd_set_gemm_stream(mode)
    try:
        yield
    finally:
        lib.kd_set_gemm_stream(prev)


@contextmanager
def _rs_mode(mode):
    lib = _lib()[0]
    prev = lib.kd_set_wgrad_rs(mode)
    try:
        yield
    finally:
        lib.kd_set_wgrad_rs(prev)


def _rows_both(M, K, N, pro, epi, add):
    """kd_pwconv_stat_rows_for with the tiled kernels only / with every streaming instance"""
    lib = _lib()[0]
    with _stream_mode(0):
        r0 = lib.kd_pwconv_stat_rows_for(M, K, N, pro, epi, int(add))
    with _stream_mode(2):
        r2 = lib.kd_pwconv_stat_rows_for(M, K, N, pro, epi, int(add))
    return r0, r2


def _no_stream_in_fp32(cases, what):
    """fp32 arithmetic: the dispatcher reports the tiled row count whatever the streaming switch says -> whole-arithmetic skip"""
    for M, K, N, pro, epi, add in cases:
        r0, r2 = _rows_both(M, K, N, pro, epi, add)
        assert r0 == r2 == R.tiled_layout(M, N)["rows"], f"{what}: a streaming instance in fp32 arithmetic? {(M, K, N, pro, epi, add)}"
    pytest.skip("streaming kernels exist in the split arithmetic only")


def _layout(M, K, N, pro, epi, add, form, what):
    """the mirrored layout of the launch about to be made (the switch is already set), asserted against the library"""
    lib = _lib()[0]
    lay = R.gemm_layout(M, K, N, pro, epi, add, form if _arith() == "split" else "tiled")
    rows = lib.kd_pwconv_stat_rows_for(M, K, N, pro, epi, int(add))
    assert rows == lay["rows"], f"{what}: the library writes {rows} statistics rows, the mirror says {lay}"
    return lay


def _gemm(A, A2, pro, pro_act, p, W, bias, C, addend, epi, X, e, epi_act, part, rows, M, K, N, m_dev=None):
    lib, P, stream = _lib()
    p = tuple(p) + (None,) * (5 - len(p))
    e = tuple(e) + (None,) * (4 - len(e))
    lib.call("kd_pwconv_gemm", P(A), _ld(A), P(A2), _ld(A2), pro, pro_act, *(P(v) for v in p), P(W), P(bias), P(C), _ld(C), P(addend),
             _ld(addend), epi, P(X), _ld(X), *(P(v) for v in e), epi_act, P(part), rows, M, K, N, P(m_dev), stream())


def _stat_check(what, key, part, ref):
    st = part.t.double().sum(0)
    assert not bool(torch.isnan(st).any()), f"{what}: statistics slab rows never written: {torch.nonzero(torch.isnan(part.t).any(2).any(1)).flatten().tolist()}"
    _check(f"{what} [s1]", key + ("s1",), st[0], ref["s1"])
    _check(f"{what} [s2]", key + ("s2",), st[1], ref["s2"])
    part.guard_ok(f"{what} [statistics slab]")


# ---- forward -----------------------------------------------------------------------------------------------------------

FWD_PLAIN = [(1, 4, 4), (37, 36, 20), (300, 100, 132)]
FWD_STREAM = [(333, K, N) for K in (32, 64, 128) for N in (32, 64, 128)] + [(333, 32, 192), (640, 64, 192)]
FWD_TALL = [(M, 32, N) for N in (32, 64, 192) for M in (128, 129, 256, 257, 385)]
FWD = [(*s, "tiled") for s in FWD_PLAIN + FWD_STREAM + FWD_TALL] + [(*s, "stream") for s in FWD_STREAM]


def _fwd_form_name(lay):
    return "pw_stream_kernel" if lay["form"] == "stream" else f"pw_gemm_kernel<{lay['bm']}x{lay['bn']}>"


def _run_fwd(inp, ref_in, M, K, N, kw, form, what, m_dev=None, count=None):
    pro, epi, add = kw["pro"], kw["epi"], kw["addend"] is not None
    lay = _layout(M, K, N, pro, epi, add, form, what)
    if form == "stream":
        assert lay["form"] == "stream", f"{what}: no streaming instance"
        r0, r2 = _rows_both(M, K, N, pro, epi, add)
        assert r0 != r2, f"{what}: the streaming switch does not change the launch"
    name = _fwd_form_name(lay)
    what = f"[{name} {_arith()}] {what}"
    C, part = Out(M, N), (Buf(lay["rows"], 2, N) if epi == 1 else None)
    _gemm(_wide(inp["A"]), None, pro, kw["pro_act"], (kw["sc"], kw["sh"]), inp["W"], kw["bias"], C.t, _wide(kw["addend"], 8, 4), epi, None,
          (kw["esc"], kw["esh"]), kw["epi_act"], None if part is None else part.t, lay["rows"], M, K, N, m_dev)
    torch.cuda.synchronize()
    dk = {k: ref_in["kw"][k] for k in kw}
    ref = R.gemm_fwd(ref_in["A"], ref_in["W"], n_part=lay["n_part"], **dk)
    key = (_arith(), name)
    C.intact(what)
    if count is None:
        _check(f"{what} [c]", key + (f"c epi{epi}",), C.t, ref["c"])
    else:
        n = min(count, M)
        assert bool(torch.isnan(C.t[n:]).all()), f"{what}: rows at or beyond the device row count {count} written"
        _check(f"{what} [c, rows below {n}]", key + (f"c epi{epi}",), C.t[:n], tuple(v[:n] for v in ref["c"]))
    if epi == 1:
        _stat_check(what, key, part, ref)


@pytest.mark.parametrize("M,K,N,form", FWD)
def test_forward(M, K, N, form):
    if form == "stream" and _arith() != "split":
        _no_stream_in_fp32([(M, K, N, pro, epi, add) for pro in (0, 1) for epi in (0, 1, 5) for add in (0, 1)], "forward")
    inp = R.fwd_inputs(_gen(M, K, N), M, K, N)
    _shares(inp["A"], *inp["pro"][2], f"[forward operand {(M, K, N)}]")
    dinp = _d(inp)
    with _stream_mode(2 if form == "stream" else 0):
        for (what, kw), (_, dkw) in zip(R.fwd_cases(inp), R.fwd_cases(dinp)):
            _run_fwd(inp, dict(A=dinp["A"], W=dinp["W"], kw=dkw), M, K, N, kw, form, f"forward {(M, K, N)} {what}")


@pytest.mark.parametrize("M,K,N", [(300, 64, 128), (300, 32, 64)])
@pytest.mark.parametrize("form", ["tiled", "stream"])
def test_forward_m_dev(M, K, N, form):
    """a device-side row count: inside a tile / slab, on a tile boundary, equal to M and larger than M"""
    if form == "stream" and _arith() != "split":
        _no_stream_in_fp32([(M, K, N, pro, epi, 1) for pro in (0, 1) for epi in (0, 5)], "m_dev")
    inp = R.fwd_inputs(_gen(M, K, N, 9), M, K, N)
    dinp = _d(inp)
    with _stream_mode(2 if form == "stream" else 0):
        for (what, kw), (_, dkw) in zip(R.fwd_cases(inp), R.fwd_cases(dinp)):
            if kw["epi"] == 1 or kw["epi_act"] == 0 and kw["epi"] == 5 or kw["pro_act"] == 1 or kw["bias"] is None:
                continue            # epi 0 and epi 5 (ReLU, ReLU6), pro 0 and pro 1 / ReLU6, with and without the residual
            for count in (77, 256, M, M + 50):
                m_dev = torch.tensor([count], dtype=torch.int32, device="cuda")
                _run_fwd(inp, dict(A=dinp["A"], W=dinp["W"], kw=dkw), M, K, N, kw, form, f"m_dev={count} {(M, K, N)} {what}", m_dev, count)


# ---- data gradient -----------------------------------------------------------------------------------------------------

DG_STREAM = [(333, Kr, No) for Kr in (32, 64, 128) for No in (32, 64, 128)] + [(333, 32, 192), (257, 64, 192), (129, 128, 768)]
DG = [(*s, "tiled") for s in [(37, 20, 36)] + DG_STREAM] + [(*s, "stream") for s in DG_STREAM]


def _run_dgrad(inp, dinp, M, Kred, Nout, kw, dkw, form, what):
    epi, add = kw["epi"], kw["addend"] is not None
    lay = _layout(M, Kred, Nout, 2, epi, add, form, what)
    if form == "stream":
        r0, r2 = _rows_both(M, Kred, Nout, 2, epi, add)
        assert r0 != r2, f"{what}: the streaming switch does not change the launch"
    name = _fwd_form_name(lay)
    what = f"[{name} {_arith()}] {what}"
    C, part = Out(M, Nout), (Buf(lay["rows"], 2, Nout) if epi == 2 else None)
    _gemm(_wide(inp["G"]), _wide(inp["Y"], 8, 0), 2, kw["pro_act"], (kw["al"], kw["be"], kw["ga"], kw["msc"], kw["msh"]), inp["Wt"], None, C.t,
          _wide(kw["addend"], 8, 4), epi, _wide(inp["X"], 0, 8) if epi == 2 else None, (kw["esc"], kw["esh"], kw["mean"], kw["invstd"]),
          kw["epi_act"], None if part is None else part.t, lay["rows"], M, Kred, Nout)
    torch.cuda.synchronize()
    ref = R.gemm_dgrad(dinp["G"], dinp["Y"], dinp["Wt"], n_part=lay["n_part"], **dkw)
    key = (_arith(), name)
    C.intact(what)
    _check(f"{what} [c]", key + (f"c pro2 epi{epi}",), C.t, ref["c"])
    if epi == 2:
        _stat_check(what, key + ("epi2",), part, ref)
    return C.t


@pytest.mark.parametrize("M,Kred,Nout,form", DG)
def test_data_gradient(M, Kred, Nout, form):
    cases = [(pa, add, epi) for pa in (1, 2, 0) for add in (0, 1) for epi in (0, 2)]
    if form == "stream" and _arith() != "split":
        _no_stream_in_fp32([(M, Kred, Nout, 2, epi, add) for _, add, epi in cases], "data gradient")
    inp = R.dgrad_inputs(_gen(M, Kred, Nout, 1), M, Kred, Nout)
    _shares(inp["Y"], *inp["pro"][2], f"[data gradient operand {(M, Kred, Nout)}]")
    _shares(inp["X"], *inp["epi"][2][:2], f"[data gradient epilogue {(M, Kred, Nout)}]")
    dinp = _d(inp)
    ran = 0
    with _stream_mode(2 if form == "stream" else 0):
        for (what, kw), (_, dkw) in zip(R.dgrad_cases(inp), R.dgrad_cases(dinp)):
            if form == "stream" and R.stream_layout(M, Kred, Nout, 2, kw["epi"], kw["addend"] is not None) is None:
                continue            # (stream_cfg keeps this instance out: the tiled form of the case runs under "tiled")
            _run_dgrad(inp, dinp, M, Kred, Nout, kw, dkw, form, f"data gradient {(M, Kred, Nout)} {what}")
            ran += 1
    assert ran >= (6 if form == "stream" else 24), f"data gradient {(M, Kred, Nout)} {form}: only {ran} cases have an instance"


# ---- weight gradient ---------------------------------------------------------------------------------------------------

WG_RS = [(17, 384, 64), (777, 192, 32), (301, 768, 128), (777, 64, 192), (777, 64, 384), (301, 128, 384), (301, 128, 768), (777, 128, 128),
         (777, 128, 64), (777, 64, 128), (777, 128, 256), (301, 256, 256), (777, 64, 256)]
WG_PLAIN = [(129, 768, 768), (37, 20, 36), (100, 32, 32), (333, 100, 132), (333, 36, 200), (1000, 16, 256)]
WG = [(*s, "tiled") for s in WG_RS + WG_PLAIN] + [(*s, "rs") for s in WG_RS]


def _wgrad(inp, args, M, N, K, what):
    """one kd_pwconv_wgrad launch on column slices, a NaN dW and a NaN workspace"""
    lib, P, stream = _lib()
    al, be, ga, msc, msh, dm, da, A, asc, ash, am, aa = args
    nb = lib.kd_pwconv_wgrad_ws_bytes(M, N, K)
    assert nb == R.wgrad_ws_bytes(M, N, K), f"{what}: workspace of {nb} B, the mirror says {R.wgrad_ws_bytes(M, N, K)}"
    dW, ws = Buf(N, K), Buf(nb // 4)
    D, X, Aw = _wide(inp["D"]), _wide(inp["X"], 8, 0), _wide(A, 0, 8)
    lib.call("kd_pwconv_wgrad", P(D), _ld(D), P(X), _ld(X), dm, da, P(al), P(be), P(ga), P(msc), P(msh), P(Aw), _ld(Aw), am, aa, P(asc), P(ash),
             P(dW.t), M, N, K, P(ws.t), nb, stream())
    torch.cuda.synchronize()
    dW.guard_ok(f"{what} [dW]")
    ws.guard_ok(f"{what} [workspace]")
    return dW.t


@pytest.mark.parametrize("M,N,K,form", WG)
def test_weight_gradient(M, N, K, form):
    split = _arith() == "split"
    inp = R.wgrad_inputs(_gen(M, N, K, 2), M, N, K)
    if form == "rs":
        assert R.wgrad_rs_layout(M, N, K) is not None, f"no role-specialised instance for N={N} K={K}"
        if not split:                   # no such instance in fp32 arithmetic: the switch changes nothing, bit for bit
            args = next(a for w, a in R.wgrad_cases(inp) if w == "d_mode=2 d_act=2 a_mode=1 a_act=2")
            with _rs_mode(0):
                t0 = _wgrad(inp, args, M, N, K, "fp32, tiled")
            with _rs_mode(2):
                t2 = _wgrad(inp, args, M, N, K, "fp32, every instance")
            assert torch.equal(t0, t2), "a role-specialised instance in fp32 arithmetic?"
            pytest.skip("the role-specialised weight gradient exists in the split arithmetic only")
    _shares(inp["X"], *inp["d"][2], f"[weight gradient D {(M, N, K)}]")
    _shares(inp["A"], *inp["a"][2], f"[weight gradient A {(M, N, K)}]")
    dinp = _d(inp)
    lay = R.wgrad_layout(M, N, K, form, split)
    name = "pw_wgrad_rs_kernel" if lay["form"] == "rs" else f"pw_wgrad_kernel<{lay['wn']},{lay['wk']},{lay['wm']}>"
    with _rs_mode(2 if form == "rs" else 0):
        for (what, args), (_, dargs) in zip(R.wgrad_cases(inp), R.wgrad_cases(dinp)):
            what = f"[{name} {_arith()}] weight gradient {(M, N, K)} {what}"
            got = _wgrad(inp, args, M, N, K, what)
            _check(what, (_arith(), name, "dw"), got, R.gemm_wgrad(dinp["D"], dinp["X"], *dargs, lay["n_red"])["dw"])


# ---- waves that own several slabs; the non-temporal store ---------------------------------------------------------------

LOOP = [(131173, 128, 128, 1, True), (131000, 128, 128, 1, False), (43557, 32, 192, 3, False)]


@pytest.mark.parametrize("kind", ["forward", "data gradient"])
@pytest.mark.parametrize("M,K,N,ntiles,nt", LOOP)
def test_looping_and_non_temporal(M, K, N, ntiles, nt, kind):
    """forward epi 1 with pro 1 / ReLU6 and the data gradient epi 2 at row counts where a streaming wave owns two or three slabs
    (the last one ragged), at one and at three column tiles, with C just above and just below the non-temporal threshold"""
    split = _arith() == "split"
    fwd = kind == "forward"
    pro, epi = (1, 1) if fwd else (2, 2)
    add = False if fwd else next(a for a in (False, True) if R.stream_cfg(K, N, 2, 2, a) is not None)
    lay = R.stream_layout(M, K, N, pro, epi, add)
    # the derivation of the shapes, from stream_grid and kd_nt_store as they are in the tree: a retune must fail here
    assert lay is not None and lay["ntiles"] == ntiles and lay["grid"] == 256 // ntiles, lay
    assert M > 32 * R.SW * lay["grid"], "no wave owns a second slab"
    assert (M * N * 4 >= R.NT_BYTES) == nt
    if nt or ntiles == 3:
        assert M > 2 * 32 * R.SW * lay["grid"] and lay["slabs_per_wave"] == 3 and M % 32 != 0, "two full rounds of slabs and a ragged tail"
    if nt:
        assert (M - 200) * N * 4 < R.NT_BYTES, "just above the threshold"
    inp = R.fwd_inputs(_gen(M, K, N, 3), M, K, N) if fwd else R.dgrad_inputs(_gen(M, K, N, 4), M, K, N)
    outs = {}
    for form in (("tiled", "stream") if split else ("tiled",)):
        with _stream_mode(2 if form == "stream" else 0):
            flay = _layout(M, K, N, pro, epi, add, form, kind)
            assert flay["form"] == form
            name = _fwd_form_name(flay)
            what = f"[{name} {_arith()}] {kind} {(M, K, N)} {'non-temporal' if nt else 'plain'} store"
            key = (_arith(), name + " looping")
            C, part = Buf(M, N), Buf(flay["rows"], 2, N)
            if fwd:
                sc, sh = inp["pro"][2]
                _shares(inp["A"], sc, sh, what)
                _gemm(inp["A"], None, 1, 2, (sc, sh), inp["W"], inp["bias"], C.t, None, 1, None, (), 0, part.t, flay["rows"], M, K, N)
                torch.cuda.synchronize()
                ref = R.gemm_fwd(inp["A"].double(), inp["W"].double(), pro=1, pro_act=2, sc=sc.double(), sh=sh.double(), bias=inp["bias"].double(),
                                 epi=1, n_part=flay["n_part"])
            else:
                msc, msh = inp["pro"][2]
                esc, esh, mean, inv = inp["epi"][2]
                addend = inp["addend"] if add else None
                _gemm(inp["G"], inp["Y"], 2, 2, (*inp["fold"], msc, msh), inp["Wt"], None, C.t, addend, 2, inp["X"], (esc, esh, mean, inv), 2, part.t,
                      flay["rows"], M, K, N)
                torch.cuda.synchronize()
                al, be, ga = _d(inp["fold"])
                ref = R.gemm_dgrad(inp["G"].double(), inp["Y"].double(), inp["Wt"].double(), al, be, ga, msc.double(), msh.double(), 2,
                                   addend=None if addend is None else addend.double(), epi=2, X=inp["X"].double(), esc=esc.double(), esh=esh.double(),
                                   mean=mean.double(), invstd=inv.double(), epi_act=2, n_part=flay["n_part"])
            C.guard_ok(what)
            _check(f"{what} [c]", key + ("c",), C.t, ref["c"])
            _stat_check(what, key, part, ref)
            outs[form] = C.t
    if split:
        assert torch.equal(outs["tiled"], outs["stream"]), f"{kind} {(M, K, N)}: streaming and tiled C differ"


# ---- one product per output element ------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["pw_gemm_kernel<128x128>", "pw_gemm_kernel<256x64>", "pw_stream_kernel", "pw_wgrad_kernel", "pw_wgrad_rs_kernel"])
def test_single_product(form):
    """Operands with one non-zero per reduction, full 24-bit random mantissas, exponents -8 .. 8: every output element is one product
    x*y and every other accumulation an exact add of zero, so |got - x*y| is the arithmetic's per-product error."""
    lib, P, stream = _lib()
    split = _arith() == "split"
    limit = SPLIT_PRODUCT_U if split else 1.0
    g = _gen(len(form), 77)
    if "wgrad" not in form:
        K, N = 64, (64 if "256x64" in form else 128)
        M = (1 << 20) // N
        if form == "pw_stream_kernel" and not split:
            _no_stream_in_fp32([(M, K, N, 0, 0, 0)], "single product")
        x, W = R.probe_values(g, M), R.probe_values(g, N, K)
        col = torch.arange(M, device="cuda") % K
        A = torch.zeros(M, K, device="cuda")
        A[torch.arange(M, device="cuda"), col] = x
        exact = x.double()[:, None] * W.double()[:, col].t()
        with _stream_mode(2 if form == "pw_stream_kernel" else 0):
            lay = _layout(M, K, N, 0, 0, False, "stream" if form == "pw_stream_kernel" else "tiled", form)
            assert _fwd_form_name(lay) == form, lay
            C = Buf(M, N)
            _gemm(A, None, 0, 0, (), W, None, C.t, None, 0, None, (), 0, None, 0, M, K, N)
            torch.cuda.synchronize()
            C.guard_ok(form)
    else:
        rs = form == "pw_wgrad_rs_kernel"
        M = N = 768
        K = 128 if rs else 768
        assert (R.wgrad_rs_layout(M, N, K) is not None) == rs
        nb = lib.kd_pwconv_wgrad_ws_bytes(M, N, K)
        C, ws = Buf(N, K), Buf(nb // 4)
        got, exact = [], []

        def run():
            x, A = R.probe_values(g, M), R.probe_values(g, M, K)
            D = torch.diag(x)
            C.t.fill_(NAN)
            lib.call("kd_pwconv_wgrad", P(D), N, None, 0, 0, 0, None, None, None, None, None, P(A), K, 0, 0, None, None, P(C.t), M, N, K, P(ws.t),
                     nb, stream())
            torch.cuda.synchronize()
            got.append(C.t.clone())
            exact.append(x.double()[:, None] * A.double())
        if rs and not split:
            g0 = g.get_state()
            with _rs_mode(0):
                run()
            g.set_state(g0)
            with _rs_mode(2):
                run()
            assert torch.equal(got[0], got[1]), "a role-specialised instance in fp32 arithmetic?"
            pytest.skip("the role-specialised weight gradient exists in the split arithmetic only")
        with _rs_mode(2 if rs else 0):
            for _ in range(-(-(1 << 20) // (N * K))):
                run()
        ws.guard_ok(form)
        C.guard_ok(form)
        C, exact = torch.cat(got), torch.cat(exact)
    got = (C.t if isinstance(C, Buf) else C).double()
    assert not bool(torch.isnan(got).any()), f"[{form}] elements never written"
    ratio = ((got - exact).abs() / (R.U * exact.abs())).max().item()
    print(f"\nPROBE {_arith()} {form} worst |got - x*y| / (U |x||y|) = {ratio:.4f} over {exact.numel()} products")
    assert ratio <= limit, f"[{form} {_arith()}] per-product error {ratio:.4f} U |x||y| exceeds {limit} U |x||y|"


# ---- small utilities: bit for bit ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sizes", [[(4, 4)], [(768, 256)], [(5, 12)], [(4, 4), (16, 16), (7, 12), (768, 256), (33, 20)],
                                   [(64, 4), (3, 3), (128, 128), (1, 1000), (257, 1)]], ids=lambda s: "-".join(f"{r}x{c}" for r, c in s))
def test_transpose_batch(sizes):
    """n in {1, 5} matrices, R*C a multiple of 256 and not, first-block offsets ascending from 0 as include/kd_hip.h describes"""
    lib, P, stream = _lib()
    g = _gen(len(sizes), *sizes[0])
    ins = [torch.randn(r, c, generator=g, device="cuda") for r, c in sizes]
    outs = [Buf(c, r) for r, c in sizes]
    first, rows = 0, []
    for (r, c), i, o in zip(sizes, ins, outs):
        rows.append([i.data_ptr(), o.t.data_ptr(), r, c, first])
        first += -(-r * c // 256)
    table = torch.tensor(rows, dtype=torch.int64, device="cuda")
    lib.call("kd_transpose_batch", P(table), len(sizes), first, stream())
    torch.cuda.synchronize()
    for (r, c), i, o in zip(sizes, ins, outs):
        assert torch.equal(o.t, i.t().contiguous()), f"kd_transpose_batch: matrix {r}x{c} of {sizes}"
        o.guard_ok(f"kd_transpose_batch {r}x{c} of {sizes}")


@pytest.mark.parametrize("lens", [(1,), (0, 1), (255, 256, 257), (100003, 0, 1, 256), (0, 0, 0, 5), (257,), (256, 100000), (1, 1, 1, 1)],
                         ids=lambda s: "-".join(map(str, s)))
def test_copy_segments(lens):
    lib, P, stream = _lib()
    g = _gen(len(lens), *lens)
    src = [torch.randn(max(n, 1), generator=g, device="cuda")[:n] for n in lens]
    dst = [Buf(n) for n in lens]
    args = []
    for k in range(4):
        args += [P(src[k]), P(dst[k].t), lens[k]] if k < len(lens) else [None, None, 0]
    lib.call("kd_copy_segments", *args, stream())
    torch.cuda.synchronize()
    for n, s, d in zip(lens, src, dst):
        assert torch.equal(d.t, s), f"kd_copy_segments: segment of {n} of {lens}"
        d.guard_ok(f"kd_copy_segments {n} of {lens}")
