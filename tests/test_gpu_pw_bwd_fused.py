"""kd_pwconv_bwd (csrc/kd_wgrad_rs.hip): the data gradient and the weight gradient of the 192 x 32 1x1 layer in one launch -- the
role-specialised weight-gradient kernel with the data gradient on a matrix wave that plan leaves idle.  Called through the C
ABI on seeded inputs (tests/_fp64_gemm_ref.py) and compared BIT FOR BIT with the two launches it replaces:

    dW == kd_pwconv_wgrad (default role-specialised mode)          dX == kd_pwconv_gemm(pro = d_mode, epi 0) with W = Wt

(d_mode 0 hands the raw gradient to both GEMMs, so its data gradient is the pro 0 launch of the tiled kernel; d_mode 2 is
what unit_backward passes: pro 2, with the ReLU6 mask coefficients or without a mask.)  dW, the workspace and dX start as NaN; dX
is followed by 64 sentinel rows.  Row counts: one row, around one 32-row chunk (33: a one-row tail chunk), one slice of nine
chunks (odd count: the padding step runs), three slices with a short ragged last one, 256 slices with a ragged tail.  At
M = 773 both results also meet the float64 bounds tests/test_gpu_gemm_fp64.py applies to the existing kernels.

The library has no instance with an addend (kd_pwconv_bwd refuses it, the caller keeps two launches): refusals below.
Unit level: an InvertedResidual(32, 64, stride 2) backward with units._PW_BWD_FUSED on and off, same gradient bits."""
import pytest
import torch

import _fp64_gemm_ref as R
from test_gpu_tail_kernels import NAN, SENT

pytestmark = pytest.mark.gpu

N, K = 192, 32
ROWS = [1, 31, 32, 33, 257, 773, 65553]
GUARD_ROWS = 64
ACT_NONE, ACT_RELU6 = 0, 2


def _lib():
    from kdrt.lib import lib, KDError
    from kdrt.ops import P, stream
    return lib, P, stream, KDError


@pytest.fixture(autouse=True)
def _split_arithmetic():
    from kdrt import ops
    prev = ops.set_gemm_arithmetic("split")
    yield
    ops.set_gemm_arithmetic(prev)


_INPUTS = {}


def _inputs(M):
    """seeded operands of one row count, shared by its cases (never written)"""
    if M not in _INPUTS:
        g = torch.Generator(device="cuda").manual_seed(4100 + M)
        w = R.wgrad_inputs(g, M, N, K)                     # D, X [M, N], A [M, K], fold, mask coefficients
        d = R.dgrad_inputs(g, 1, N, K)                     # Wt [K, N] (one row of everything else)
        _INPUTS[M] = dict(D=w["D"], X=w["X"], A=w["A"], fold=w["fold"], mask=w["d"], Wt=d["Wt"].contiguous())
    return _INPUTS[M]


def _case(inp, mode):
    """(d_mode, d_act, al, be, ga, msc, msh) as unit_backward passes them"""
    al, be, ga = inp["fold"]
    if mode == "d_mode0":
        return 0, ACT_NONE, None, None, None, None, None
    if mode == "d_mode2":
        return 2, ACT_NONE, al, be, ga, None, None
    msc, msh = inp["mask"][ACT_RELU6]
    return 2, ACT_RELU6, al, be, ga, msc, msh


def _two_kernels(inp, M, case):
    lib, P, stream, _ = _lib()
    dm, da, al, be, ga, msc, msh = case
    nb = lib.kd_pwconv_wgrad_ws_bytes(M, N, K)
    dW = torch.full((N, K), NAN, device="cuda")
    ws = torch.full((nb // 4,), NAN, device="cuda")
    lib.call("kd_pwconv_wgrad", P(inp["D"]), N, P(inp["X"]), N, dm, da, P(al), P(be), P(ga), P(msc), P(msh), P(inp["A"]), K, 0, 0, None,
             None, P(dW), M, N, K, P(ws), nb, stream())
    dX = torch.full((M, K), NAN, device="cuda")
    lib.call("kd_pwconv_gemm", P(inp["D"]), N, P(inp["X"]) if dm == 2 else None, N if dm == 2 else 0, dm, da, P(al), P(be), P(ga), P(msc),
             P(msh), P(inp["Wt"]), None, P(dX), K, None, 0, 0, None, 0, None, None, None, None, 0, None, 0, M, N, K, None, stream())
    torch.cuda.synchronize()
    return dW, dX


def _fused(inp, M, case):
    lib, P, stream, _ = _lib()
    dm, da, al, be, ga, msc, msh = case
    assert lib.kd_pwconv_bwd_supported(N, K, dm, 0, 0) == 1
    nb = lib.kd_pwconv_bwd_ws_bytes(M, N, K)
    assert nb >= R.wgrad_rs_layout(M, N, K)["ws_bytes"]
    dW = torch.full((N, K), NAN, device="cuda")
    ws = torch.full((nb // 4 + GUARD_ROWS,), NAN, device="cuda")
    ws[nb // 4:] = SENT
    buf = torch.full((M + GUARD_ROWS, K), NAN, device="cuda")
    buf[M:] = SENT
    lib.call("kd_pwconv_bwd", P(inp["D"]), N, P(inp["X"]), N, dm, da, P(al), P(be), P(ga), P(msc), P(msh), P(inp["A"]), K, 0, 0, None,
             None, P(inp["Wt"]), P(buf), K, None, 0, 0, P(dW), M, N, K, P(ws), nb, stream())
    torch.cuda.synchronize()
    assert bool((buf[M:] == SENT).all()), "rows at or beyond M written"
    assert bool((ws[nb // 4:] == SENT).all()), "written past the workspace"
    return dW, buf[:M]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("mode", ["d_mode0", "d_mode2", "d_mode2_relu6"])
@pytest.mark.parametrize("M", ROWS)
def test_bits_of_the_two_kernels(M, mode):
    inp = _inputs(M)
    case = _case(inp, mode)
    dW0, dX0 = _two_kernels(inp, M, case)
    dW1, dX1 = _fused(inp, M, case)
    assert not bool(torch.isnan(dW1).any()), f"{int(torch.isnan(dW1).sum())} elements of dW never written"
    assert not bool(torch.isnan(dX1).any()), f"{int(torch.isnan(dX1).any(1).sum())} rows of dX never written"
    nw = int((_bits(dW0) != _bits(dW1)).sum())
    assert nw == 0, f"dW differs from kd_pwconv_wgrad in {nw} of {N * K} elements (max {float((dW0 - dW1).abs().max()):.3g})"
    nx = int((_bits(dX0) != _bits(dX1)).sum())
    assert nx == 0, f"dX differs from kd_pwconv_gemm in {nx} of {M * K} elements (max {float((dX0 - dX1).abs().max()):.3g})"
    if M == 773:            # the float64 bounds of tests/test_gpu_gemm_fp64.py: same bound functions, same arithmetic
        dm, da, al, be, ga, msc, msh = case
        d64 = lambda t: None if t is None else t.double()
        lay = R.wgrad_rs_layout(M, N, K)
        ref_w = R.gemm_wgrad(d64(inp["D"]), d64(inp["X"]), d64(al), d64(be), d64(ga), d64(msc), d64(msh), dm, da, d64(inp["A"]), None, None, 0, 0,
                             lay["n_red"])["dw"]
        if dm == 2:
            ref_x = R.gemm_dgrad(d64(inp["D"]), d64(inp["X"]), d64(inp["Wt"]), d64(al), d64(be), d64(ga), d64(msc), d64(msh), da)["c"]
        else:
            ref_x = R.gemm_fwd(d64(inp["D"]), d64(inp["Wt"]))["c"]
        for what, got, (val, err) in (("dW", dW1, ref_w), ("dX", dX1, ref_x)):
            r = ((got.double() - val).abs() / err.clamp_min(1e-300)).max().item()
            print(f"RATIO kd_pwconv_bwd {mode} {what} {r:.4f}")
            assert r <= 1.0, f"{what}: worst error {r:.3g} x the float64 bound"


def test_refusals():
    lib, P, stream, KDError = _lib()
    assert lib.kd_pwconv_bwd_supported(192, 32, 2, 0, 0) == 1 and lib.kd_pwconv_bwd_supported(192, 32, 0, 0, 0) == 1
    for n, k, dm, am, epi in ((128, 128, 2, 0, 0), (32, 32, 2, 0, 0), (192, 32, 2, 1, 0), (192, 32, 2, 0, 2), (192, 32, 1, 0, 0), (32, 192, 2, 0, 0)):
        assert lib.kd_pwconv_bwd_supported(n, k, dm, am, epi) == 0, (n, k, dm, am, epi)
    prev = lib.kd_set_gemm_split(0)
    try:
        assert lib.kd_pwconv_bwd_supported(192, 32, 2, 0, 0) == 0, "an instance in the exact-fp32 arithmetic?"
    finally:
        lib.kd_set_gemm_split(prev)
    assert lib.kd_pwconv_bwd_supported(192, 32, 2, 0, 0) == 1
    M = 64
    inp = _inputs(257)
    al, be, ga = inp["fold"]
    nb = lib.kd_pwconv_bwd_ws_bytes(M, N, K)
    ws = torch.full((nb // 4,), NAN, device="cuda")
    dW, dX = torch.full((128, 128), NAN, device="cuda"), torch.full((M, 128), NAN, device="cuda")
    add = torch.zeros(M, K, device="cuda")

    def call(n=N, k=K, am=0, epi=0, addend=None, ldd=None, nbytes=nb):
        lib.call("kd_pwconv_bwd", P(inp["D"]), n if ldd is None else ldd, P(inp["X"]), n, 2, 0, P(al), P(be), P(ga), None, None, P(inp["A"]),
                 k, am, 0, P(al) if am else None, P(al) if am else None, P(inp["Wt"]), P(dX), k, P(addend), K if addend is not None else 0,
                 epi, P(dW), M, n, k, P(ws), nbytes, stream())

    for kw, msg in ((dict(n=128, k=128), "no instance"), (dict(n=32, k=32), "no instance"), (dict(am=1), "no instance"),
                    (dict(epi=2), "no instance"), (dict(addend=add), "addend"), (dict(ldd=N + 8), "dense"), (dict(nbytes=nb - 4), "workspace")):
        with pytest.raises(KDError, match=msg):
            call(**kw)
    prev = lib.kd_set_gemm_split(0)
    try:
        with pytest.raises(KDError, match="exact-fp32"):
            call()
    finally:
        lib.kd_set_gemm_split(prev)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dW).all()) and bool(torch.isnan(dX).all()) and bool(torch.isnan(ws).all()), "a refused call launched"


def test_unit_backward_dispatch():
    from kdrt import units
    from src.models.camera_encoder import InvertedResidual
    torch.manual_seed(3)
    m = InvertedResidual(32, 64, stride=2).cuda().train()
    x0 = torch.randn(2, 32, 16, 16, generator=torch.Generator().manual_seed(17)).cuda()
    res = {}
    saved = units._PW_BWD_FUSED
    calls = []
    real_call = units.lib.call
    try:
        units.lib.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        for on in (False, True):
            units._PW_BWD_FUSED = on
            m.zero_grad()
            x = x0.clone().requires_grad_(True)
            y = m(x)
            calls.clear()
            (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
            torch.cuda.synchronize()
            assert ("kd_pwconv_bwd" in calls) == on, calls
            res[on] = {"input": x.grad.clone(), **{n: p.grad.clone() for n, p in m.named_parameters()}}
    finally:
        del units.lib.__dict__["call"]                     # (the instance attribute: the class's method is back)
        units._PW_BWD_FUSED = saved
    for name in res[True]:
        assert not bool(torch.isnan(res[True][name]).any()), name
        assert torch.equal(_bits(res[False][name]), _bits(res[True][name])), f"gradient of {name} differs between the two forms"
