"""The bf16-storage inference kernels (csrc/kd_bf16.hip, and csrc/kd_lidar_infer.hip's one-kernel LiDAR encoder), each called
directly through the C ABI and compared element-wise with a float64 evaluation of the same operation on the same bf16-rounded
operands (tests/_bf16_ref.py).  A bf16 output must lie in [rne_bf16(act(value - err)), rne_bf16(act(value + err))] with
err = C_BOUND * n_seq * 2^-24 * sum|t_i|; an fp32 output within err.  Every case family runs on random inputs (the interval; the
share of intervals that hold more than one bf16 value is printed and capped at 25 %) and on exactly summable inputs (small
integers times powers of two: the output must equal rne_bf16(exact) bit for bit, fp32 outputs exactly).

Row / item counts come from each kernel's own launch layout (the mirrors in _bf16_ref.py, asserted per case by on_ladder): a few
rows, a partial unit or block, full-1, full, full+1 (one unit into a second grid turn) and a ragged third turn.  Outputs start as
NaN (an unwritten element fails), carry sentinel columns / a sentinel tail (an element written outside fails), and the A operand's
columns from K on are NaN (they must never be loaded).

Kernel -> tests:
  pw_gemm_bf16_v2_kernel<NB, KU, RES> (KU = 2 ... 48, NB 4 / 2 / 1, both RES): test_gemm_second_form_ladder (also the same bits as
      the first form; NB = 4 with RES at K = 128 and 384), test_gemm_small_shapes
  pw_gemm_bf16_kernel<4 / 2 / 1, 0, 0>: test_gemm_first_form_ladder (device-side row count, also one smaller than M)
  pw_gemm_bf16_kernel<1, 0 / 1, 0, TAIL>: test_gemm_tail_shapes;  <., 1, 0>: test_gemm_fp32_input
  pw_gemm_bf16_kernel<4, 3, 0> and <4, 0, 4>: test_lidar_two_launches (each alone and chained)
  lidar_mlp_scatter_infer_kernel<1> / <3>: test_lidar_one_kernel, test_lidar_one_kernel_split_arithmetic
  dw_bf16_s1_pipe_kernel<16> / <8>, dw_bf16_kernel<1> / <2>: test_dw_ladder, test_dw_segments_and_edges
  stem_bf16_v2_kernel<3, COUT>, stem_bf16_kernel<COUT>: test_stem_ladder, test_stem_widths_and_edges
  bilinear_sum_bf16_kernel: test_bilinear_ratios, test_bilinear_ladder
  cls_bf16_kernel: test_cls_ladder, test_cls_shapes;  weighted_tail_bf16_kernel: test_weighted_tail
  argument checks of all seven entry points: test_refusals

Measured on an MI355X: 353 cases in 3.6 s of test time (6.0 s with collection), peak allocated memory 2981 MiB (the float64
references of the three-turn GEMM and depthwise cases); test_zz_report_peak_memory prints both figures."""
import time

import numpy as np
import pytest
import torch

import _bf16_ref as R
from test_gpu_tail_kernels import GUARD, NAN, RESIZE, SENT, Buf, _check, _ladder

pytestmark = pytest.mark.gpu

PAD = 32                      # sentinel columns on both sides of a GEMM output (C is a column slice of a wider buffer)
MARK = 7.0
_T0 = time.time()


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


class BBuf:
    """a NaN-filled bf16 output of n elements followed by a guard of sentinels"""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + GUARD,), NAN, device="cuda", dtype=torch.bfloat16)
        self.buf[n:] = SENT
        self.sent = self.buf[n].clone()
        self.t = self.buf[:n].view(*shape)

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == self.sent).all()), f"{what}: written past its end"


def _fail(what, bad, got, lo, hi):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(bad.shape)))
    pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} outside the rule; first at {idx}: got {got.reshape(-1)[i].item():.9g}, "
                f"admitted [{lo.reshape(-1)[i].item():.9g}, {hi.reshape(-1)[i].item():.9g}]")


def _check_bf16(what, got, ref, act_id=R.NONE, res=None, exact=False):
    z, e = ref
    g = got.double().reshape(z.shape)
    assert not bool(torch.isnan(g).any()), f"{what}: {int(torch.isnan(g).sum())} elements never written"
    lo, hi = R.interval(z, torch.zeros_like(e) if exact else e, act_id, res)
    share = R.loose_share(lo, hi)
    if exact:
        assert share == 0
    else:
        print(f"{what}: {share:.2%} of the intervals hold more than one bf16 value")
        assert share <= R.LOOSE_CAP, f"{what}: input set too loose ({share:.1%})"
    bad = (g < lo) | (g > hi)
    if bool(bad.any()):
        _fail(what, bad, g, lo, hi)


# ---- kd_bf16_pwconv, epi 0 ----------------------------------------------------------------------------------------------

def _gemm_inputs(M, K, N, res, exact, a_kind, act_id, seed):
    g = _gen(seed)
    lda = K + (8 if a_kind == 0 else 4)
    if exact:
        A, W, b, sc, sh = R.exact_gemm_inputs(g, M, K, N, "cuda", lda=lda, fp32_a=a_kind == 1, relu6=act_id == R.RELU6)
        Rs = R.exact_acts(g, (M, N + 8), 8, device="cuda") if res else None
    else:
        A, W, b, sc, sh = R.random_gemm_inputs(g, M, K, N, "cuda", lda=lda, fp32_a=a_kind == 1)
        Rs = torch.randn(M, N + 8, generator=g, device="cuda").bfloat16() if res else None
    return A, W, b, sc, sh, Rs


def _gemm_run(inputs, M, K, N, a_kind, act_id, first_form, m_eff=None):
    """-> the [M, N] output view; C is the middle column slice of a NaN buffer between sentinel columns, A has lda > K (NaN there),
    the residual ldres > N.  first_form: a device-side row count (m_eff, default M) selects pw_gemm_bf16_kernel."""
    lib, P, stream = _lib()
    A, W, b, sc, sh, Rs = inputs
    wide = torch.full((M, N + 2 * PAD), NAN, device="cuda", dtype=torch.bfloat16)
    wide[:, :PAD] = MARK
    wide[:, PAD + N:] = MARK
    out = wide[:, PAD:PAD + N]
    mdev = torch.tensor([M if m_eff is None else m_eff], device="cuda", dtype=torch.int32) if first_form else None
    lib.call("kd_bf16_pwconv", P(A), A.stride(0), a_kind, P(W), P(b), P(sc), P(sh), act_id, P(out), out.stride(0), P(Rs),
             Rs.stride(0) if Rs is not None else 0, 0, M, K, N, P(mdev), None, None, None, None, 0, None, None, 0, stream())
    torch.cuda.synchronize()
    assert bool((wide[:, :PAD] == MARK).all()) and bool((wide[:, PAD + N:] == MARK).all()), "columns next to C were written"
    return out


def _gemm_check(what, out, inputs, K, N, act_id, exact, m_eff=None):
    A, W, b, sc, sh, Rs = inputs
    m = out.shape[0] if m_eff is None else m_eff
    res = None if Rs is None else Rs[:m, :N]
    _check_bf16(what, out[:m], R.pwconv(A[:m, :K], W, b, sc, sh, res), act_id, res, exact)
    if m < out.shape[0]:
        assert bool(torch.isnan(out[m:]).all()), f"{what}: rows from the device-side count on were written"


def _v2_params():
    out = []
    for K, N, res in R.V2_CASES:
        cap = R.gemm_v2_layout(10 ** 7, K, N, res)["grid"]
        unit = R.gemm_v2_layout(10 ** 7, K, N, res)["unit"]
        out += [pytest.param(K, N, res, name, M, id=f"K{K}-N{N}-{'res' if res else 'nores'}-{name}") for name, M in R.gemm_ladder(unit, cap).items()]
    return out


@pytest.mark.parametrize("K,N,res,name,M", _v2_params())
def test_gemm_second_form_ladder(K, N, res, name, M):
    """every K instance of the second form through a three-turn walk over its units (32 * SL rows): the prefetch of the next
    unit's A fragments across a turn, the partial last unit, the clamped rows after M; and bit for bit the first form's output."""
    wk = R.gemm_v2_layout(M, K, N, res)
    R.on_ladder(name, wk)
    act_id = R.RELU6 if (K // 32) % 2 else R.RELU
    for exact in (False, True):
        inputs = _gemm_inputs(M, K, N, res, exact, 0, act_id, M + K + N + exact)
        what = f"{wk['kernel']} {name} M={M} {'exact' if exact else 'random'}"
        out = _gemm_run(inputs, M, K, N, 0, act_id, first_form=False)
        _gemm_check(what, out, inputs, K, N, act_id, exact)
        first = _gemm_run(inputs, M, K, N, 0, act_id, first_form=True)
        assert torch.equal(out.view(torch.int16), first.view(torch.int16)), f"{what}: the two forms differ"


@pytest.mark.parametrize("M,K,N,res", R.SMALL_CASES, ids=lambda v: str(v))
def test_gemm_small_shapes(M, K, N, res):
    """single-turn launches of the second form: M = 1, one row more than a unit, small N; with a residual NB = 1 (K = 32), NB = 2
    (N = 64, and K = 512 on the LDS budget) and NB = 4 (K = 256, N = 128)"""
    assert R.gemm_v2_layout(M, K, N, res) is not None
    for exact in (False, True):
        inputs = _gemm_inputs(M, K, N, res, exact, 0, R.RELU, M + K + exact)
        out = _gemm_run(inputs, M, K, N, 0, R.RELU, first_form=False)
        _gemm_check(f"second form M={M} K={K} N={N}", out, inputs, K, N, R.RELU, exact)


def _v1_params():
    out = []
    for K, N, res in R.V1_CASES:
        cap = R.gemm_v1_layout(10 ** 7, K, N)["grid"]
        out += [pytest.param(K, N, res, name, M, id=f"K{K}-N{N}-{'res' if res else 'nores'}-{name}") for name, M in R.gemm_ladder(32, cap).items()]
    return out


@pytest.mark.parametrize("K,N,res,name,M", _v1_params())
def test_gemm_first_form_ladder(K, N, res, name, M):
    """the first form at its NB = 4, 2 and 1 selections (and K = 96, which the second form has no instance for), selected by a
    device-side row count: equal to M, and -- from `partial` on -- 37 rows short of it (rows from there on stay NaN)."""
    wk = R.gemm_v1_layout(M, K, N)
    R.on_ladder(name, wk)
    assert wk["NB"] == {768: 4, 704: 2, 736: 1}[N]
    act_id = R.RELU6 if res else R.RELU
    for exact in (False, True):
        inputs = _gemm_inputs(M, K, N, res, exact, 0, act_id, M + K + N + exact)
        for m_eff in (M, M - 37) if M > 40 and exact else (M,):
            out = _gemm_run(inputs, M, K, N, 0, act_id, first_form=True, m_eff=m_eff)
            _gemm_check(f"{wk['kernel']} {name} M={M} m_dev={m_eff} {'exact' if exact else 'random'}", out, inputs, K, N, act_id, exact, m_eff)


@pytest.mark.parametrize("a_kind", [0, 1])
@pytest.mark.parametrize("res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("K,N", R.TAIL_KN, ids=lambda v: str(v))
def test_gemm_tail_shapes(K, N, res, a_kind):
    """TAIL instances: K past a multiple of 32 by 8 / 16 / 24 (fragments past K are zeros, never loaded: A is NaN from column K
    on), a last column tile of 8 / 16 / 24 columns (neither read nor stored past N)."""
    cap = R.gemm_v1_layout(10 ** 7, K, N)["grid"]
    lad = R.gemm_ladder(32, cap)
    for name in ("few", "partial", "full+1") + (("ragged",) if (K, N) in ((104, 72), (8, 8)) else ()):
        M = lad[name]
        wk = R.gemm_v1_layout(M, K, N)
        assert wk["tail"] and wk["NB"] == 1
        R.on_ladder(name, wk)
        for exact in (True,) if name != "partial" else (False, True):
            inputs = _gemm_inputs(M, K, N, res, exact, a_kind, R.RELU, M + K + N + a_kind)
            out = _gemm_run(inputs, M, K, N, a_kind, R.RELU, first_form=False)
            _gemm_check(f"{wk['kernel']} a_kind={a_kind} {name} M={M} K={K} N={N}", out, inputs, K, N, R.RELU, exact)


@pytest.mark.parametrize("name", ["partial", "full+1", "ragged"])
@pytest.mark.parametrize("K,N", R.A1_CASES, ids=lambda v: str(v))
def test_gemm_fp32_input(K, N, name):
    """a_kind 1: fp32 A rounded to bf16 on load (the LiDAR map into the fusion)"""
    M = R.gemm_ladder(32, R.gemm_v1_layout(10 ** 7, K, N)["grid"])[name]
    wk = R.gemm_v1_layout(M, K, N)
    R.on_ladder(name, wk)
    for exact in (False, True):
        inputs = _gemm_inputs(M, K, N, name == "ragged", exact, 1, R.RELU6, M + K + exact)
        if not exact:
            assert bool((inputs[0][:, :K] != inputs[0][:, :K].bfloat16().float()).any())        # the rounding on load is a real one
        out = _gemm_run(inputs, M, K, N, 1, R.RELU6, first_form=False)
        _gemm_check(f"{wk['kernel']} a_kind=1 {name} M={M}", out, inputs, K, N, R.RELU6, exact)


# ---- the LiDAR encoder: a_kind 3, epi 4, and the one-kernel form -----------------------------------------------------------

LIDAR_P = {"one": 1, "31": 31, "32": 32, "33": 33, "full-1": 65535, "full": 65536, "full+1": 65537, "ragged": 2 * 65536 + 21845 + 5}


def _lidar_case(P, exact, seed):
    g = _gen(seed)
    ncells = P // 8 + 64
    n_skip = 0 if P < 31 else 7
    cell = R.cell_pattern(P, ncells, n_skip, "cuda")
    l0, l1, l2, pts = R.lidar_params(g, P, exact, "cuda")
    return pts.contiguous(), cell, ncells, l0, l1, l2


def _grid_check(what, grid, ref, cell, ncells, exact):
    assert not exact or float(ref[1].max()) == 0                         # exact inputs: the bound is 0, the map must match exactly
    _check(what, grid.t, ref)
    empty = torch.ones(ncells, dtype=torch.bool, device="cuda")
    empty[cell[cell >= 0].long()] = False
    assert bool(empty.any()) and bool((grid.t[empty] == 0).all()), f"{what}: a cell without a point is not exactly 0"
    assert bool((grid.t > 0).any())
    grid.guard_ok(what)


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("name", ["33", "full+1", "ragged", "cut"])
def test_lidar_two_launches(name, exact):
    """kd_bf16_pwconv a_kind 3 (layer 0 recomputed from the point, K = 64) and epi 4 (scatter-max by cell, ReLU and ReLU6), each
    alone against its reference and chained as kdrt/bf16.py chains them.  Cells sorted, runs of equal cells across quad, half-wave
    and slab boundaries, single-point cells, a cell < 0 tail, `cut`: a device-side count that cuts a slab."""
    lib, Pp, stream = _lib()
    P = 5000 if name == "cut" else LIDAR_P[name]
    m_eff = 4987 if name == "cut" else P
    pts, cell, ncells, l0, l1, l2 = _lidar_case(P, exact, P + exact)
    wk = R.gemm_v1_layout(m_eff, 64, 128)
    assert wk["NB"] == 4 and R.gemm_v1_layout(10 ** 7, 64, 128)["per_turn"] * 32 == 65536
    if name in ("full+1", "ragged"):
        R.on_ladder(name, wk)
    mdev = torch.tensor([m_eff], device="cuda", dtype=torch.int32)
    y1 = BBuf(P, 128)
    lib.call("kd_bf16_pwconv", Pp(pts), 4, 3, Pp(l1[0]), Pp(l1[1]), Pp(l1[2]), Pp(l1[3]), R.RELU, Pp(y1.t), 128, None, 0, 0, P, 64, 128,
             Pp(mdev), Pp(l0[0]), Pp(l0[1]), Pp(l0[2]), Pp(l0[3]), R.RELU, None, None, 0, stream())
    torch.cuda.synchronize()
    a0 = R.layer0(pts[:m_eff], *l0, R.RELU)
    _check_bf16(f"a_kind 3 {name}", y1.t[:m_eff], R.pwconv(a0, *l1), R.RELU, None, exact)
    assert bool(torch.isnan(y1.t[m_eff:]).all())
    y1.guard_ok("y1")
    y1v = y1.t[:m_eff]                                              # the chained input: what the first launch wrote
    for act_id in (R.RELU, R.RELU6):
        grid = Buf(ncells, 128)
        grid.t.zero_()
        lib.call("kd_bf16_pwconv", Pp(y1.t), 128, 0, Pp(l2[0]), Pp(l2[1]), Pp(l2[2]), Pp(l2[3]), act_id, None, 0, None, 0, 4, P, 128, 128,
                 Pp(mdev), None, None, None, None, 0, Pp(cell), Pp(grid.t), 128, stream())
        torch.cuda.synchronize()
        z, e = R.pwconv(y1v, *l2)
        ref = R.scatter_max(R.act(z, act_id), torch.zeros_like(e) if exact else e, cell[:m_eff], ncells)
        _grid_check(f"epi 4 act={act_id} {name}", grid, ref, cell[:m_eff], ncells, exact)


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("name", list(LIDAR_P) + ["cut"])
def test_lidar_one_kernel(name, exact):
    """kd_bf16_lidar_mlp_scatter (NP = 1): the bound carries the layer-1 rounding uncertainty; on exact inputs the map equals the
    chained two-launch reference bit for bit."""
    lib, Pp, stream = _lib()
    P = 5000 if name == "cut" else LIDAR_P[name]
    m_eff = 4987 if name == "cut" else P
    pts, cell, ncells, l0, l1, l2 = _lidar_case(P, exact, P + exact)
    wk = R.lidar_layout(m_eff)
    if name in ("full", "full+1", "ragged"):
        R.on_ladder(name, wk)
    assert wk["iters"] == {"full+1": 2, "ragged": 3}.get(name, 1)
    pdev = torch.tensor([m_eff], device="cuda", dtype=torch.int32) if name == "cut" else None
    grid = Buf(ncells, 128)
    lib.call("kd_bf16_lidar_mlp_scatter", Pp(pts), Pp(cell), Pp(pdev), *[Pp(t) for t in l0], *[Pp(t) for t in l1], *[Pp(t) for t in l2],
             Pp(grid.t), ncells, P, 64, 128, 128, stream())
    torch.cuda.synchronize()
    ref = R.lidar_encoder(pts[:m_eff], cell[:m_eff], ncells, l0, l1, l2, exact)
    _grid_check(f"{wk['kernel']} {name}", grid, ref, cell[:m_eff], ncells, exact)


@pytest.mark.parametrize("name", list(LIDAR_P))
def test_lidar_one_kernel_split_arithmetic(name):
    """the NP = 3 instance of the same kernel (kd_lidar_mlp_scatter_infer) at the same point counts against the float64 evaluation
    of the fp32 operands: 2e-5 of the map's largest magnitude (tests/test_gpu_gemm_shapes.py's TOL), exact zeros in empty cells."""
    lib, Pp, stream = _lib()
    assert lib.kd_lidar_mlp_scatter_infer_supported(64, 128, 128)
    P = LIDAR_P[name]
    pts, cell, ncells, l0, l1, l2 = _lidar_case(P, False, P + 3)
    g = _gen(P)
    pts = torch.randn(P, 4, generator=g, device="cuda")
    grid = Buf(ncells, 128)
    lib.call("kd_lidar_mlp_scatter_infer", Pp(pts), Pp(cell), None, *[Pp(t) for t in l0], *[Pp(t) for t in l1], *[Pp(t) for t in l2],
             Pp(grid.t), ncells, P, 64, 128, 128, stream())
    torch.cuda.synchronize()
    val = R.lidar_encoder_fp32(pts, cell, ncells, l0, l1, l2)
    tol = 2e-5 * float(val.abs().max())
    _grid_check(f"NP=3 {name}", grid, (val, torch.full_like(val, tol)), cell, ncells, False)


# ---- kd_bf16_dwconv3x3 -----------------------------------------------------------------------------------------------------

def _dw_inputs(B, H, W, C, exact, seed):
    g = _gen(seed)
    if exact:
        x = R.exact_acts(g, (B, H, W, C), 100, device="cuda")
        w = R.exact_weights(g, C, 9, emin=-2, device="cuda").reshape(C, 1, 3, 3)
        sc, sh = R.exact_affine(g, C, -4, -1, device="cuda")
        return x, w, sc, sh, R.RELU
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    return rnd(B, H, W, C).bfloat16(), rnd(C, 1, 3, 3) * 0.3, rnd(C).abs() + 0.5, rnd(C) * 0.2, R.RELU6


def _dw_case(B, H, W, C, stride, exact, name=None, kernel=None):
    lib, P, stream = _lib()
    wk = R.dw_layout(B, H, W, C, stride)
    what = f"{wk['kernel']} B={B} H={H} W={W} C={C} {'exact' if exact else 'random'}"
    if kernel:
        assert wk["kernel"] == kernel, what
    if name:
        R.on_ladder(name, wk, what)
    x, w, sc, sh, act_id = _dw_inputs(B, H, W, C, exact, B * 1000 + H * 10 + W + C)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = BBuf(B, Ho, Wo, C)
    lib.call("kd_bf16_dwconv3x3", P(x), P(w), P(sc), P(sh), act_id, P(y.t), B, H, W, C, stride, stream())
    torch.cuda.synchronize()
    step = max(1, (1 << 23) // (H * W * C))
    for b0 in range(0, B, step):                                         # the reference frame by frame: float64 maps stay small
        _check_bf16(what + f" frames {b0}..", y.t[b0:b0 + step], R.dwconv(x[b0:b0 + step], w, sc, sh, stride), act_id, None, exact)
    y.guard_ok(what)


DW_LAUNCH = {"pipe16": ("dw_bf16_s1_pipe_kernel<16>", 1, 16), "pipe8": ("dw_bf16_s1_pipe_kernel<8>", 1, 8), "seg1": ("dw_bf16_kernel<1>", 1, 7),
             "seg1b": ("dw_bf16_kernel<1>", 1, 9), "seg2": ("dw_bf16_kernel<2>", 2, 5)}


def _split_items(n):
    """n work items of a one-segment map = B frames x Wo columns, Wo the largest divisor up to 20"""
    wo = max(d for d in range(1, 21) if n % d == 0)
    return n // wo, wo


def _dw_ladder_params():
    out = []
    for lname, (kernel, stride, H) in DW_LAUNCH.items():
        for C in (1024, 768, 8):
            _, slots, _ = R.cg8_layout(10 ** 7, C)
            lad = _ladder(slots, 2048)
            for name in lad if C != 8 else ("few", "partial_block", "full+1"):
                if lname == "seg1b" and name not in ("full+1", "few"):
                    continue
                out.append(pytest.param(kernel, stride, H, C, name, lad[name], id=f"{lname}-C{C}-{name}"))
    return out


@pytest.mark.parametrize("kernel,stride,H,C,name,items", _dw_ladder_params())
def test_dw_ladder(kernel, stride, H, C, name, items):
    """each of the four launches through a three-turn walk over work items on one-segment maps (Ho = 16, 8, 7 / 9, and 3 for stride
    2): C = 1024 (two items per block), 768 (idle threads in the block), 8 (256 items per block).  Exact inputs; random inputs at
    the `full+1` entry of C = 768."""
    B, Wo = _split_items(items)
    W = Wo if stride == 1 else 2 * Wo - 1
    _dw_case(B, H, W, C, stride, True, name, kernel)
    if C == 768 and name == "full+1":
        _dw_case(B, H, W, C, stride, False, name, kernel)


@pytest.mark.parametrize("B,H,W,C,stride", [(3, 32, 5, 1024, 1), (2, 48, 9, 768, 1), (3, 24, 7, 1024, 1), (2, 32, 1100, 1024, 1), (2, 24, 700, 1024, 1),
                                            (5, 48, 300, 768, 1), (2, 1, 1, 8, 1), (2, 2, 3, 16, 1), (1, 3, 2, 8, 1), (2, 1, 17, 24, 2), (3, 2, 1, 8, 2),
                                            (1, 3, 3, 40, 2), (2, 16, 15, 32, 1), (2, 16, 16, 32, 1), (2, 8, 17, 32, 1), (1, 17, 16, 64, 2), (2, 33, 15, 8, 2),
                                            (2, 40, 17, 64, 1), (1, 64, 3, 8, 1)], ids=lambda v: str(v))
def test_dw_segments_and_edges(B, H, W, C, stride):
    """two- and three-segment maps of the pipe kernels (Ho = 32, 48, 24): a thread's carry-over from one segment to its next -- rows
    0 and 1 of the next segment are fetched during the last two arrivals -- within a frame, across frames and, in the wide maps,
    across grid turns; H or W of 1, 2 and 3; W of 15, 16 and 17."""
    wk = R.dw_layout(B, H, W, C, stride)
    if W >= 300:
        assert wk["iters"] >= 2 and wk["nseg"] >= 2, wk
    _dw_case(B, H, W, C, stride, True)
    if W >= 300 or (H, W) == (16, 16):
        _dw_case(B, H, W, C, stride, False)


# ---- kd_bf16_stem ----------------------------------------------------------------------------------------------------------

def _stem_case(B, Cin, H, W, Cout, exact, name=None):
    lib, P, stream = _lib()
    wk = R.stem_layout(B, Cin, H, W, Cout)
    what = f"{wk['kernel']} B={B} Cin={Cin} H={H} W={W} {'exact' if exact else 'random'}"
    if name:
        R.on_ladder(name, wk, what)
    g = _gen(B + H * 7 + W + Cout + Cin)
    if exact:
        x = R._ints(g, (B, Cin, H, W), -1000, 1000, "cuda").float()
        w = (R._ints(g, (Cout, Cin, 3, 3), -8, 8, "cuda") / 8).float()
        sc, sh = R.exact_affine(g, Cout, -9, -6, device="cuda")
        act_id = R.RELU
    else:
        x, w = torch.randn(B, Cin, H, W, generator=g, device="cuda"), torch.randn(Cout, Cin, 3, 3, generator=g, device="cuda") * 0.3
        sc, sh, act_id = torch.randn(Cout, generator=g, device="cuda").abs() + 0.5, torch.randn(Cout, generator=g, device="cuda") * 0.2, R.RELU6
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = BBuf(B, Ho, Wo, Cout)
    lib.call("kd_bf16_stem", P(x), P(w), P(sc), P(sh), act_id, P(y.t), B, Cin, H, W, Cout, stream())
    torch.cuda.synchronize()
    _check_bf16(what, y.t, R.stem(x, w, sc, sh), act_id, None, exact)
    y.guard_ok(what)


STEM_PIX = {"one": 1, "63": 63, "64": 64, "65": 65, "255": 255, "256": 256, "257": 257, "full+1": 4096 * 256 + 1, "ragged": 2 * 4096 * 256 + 349525 + 5}


@pytest.mark.parametrize("Cin", [3, 4])
@pytest.mark.parametrize("name", list(STEM_PIX))
def test_stem_ladder(name, Cin):
    """pixels at Cout = 8 around the wave (64) and block (256) sizes and through three turns of the 4096-block cap; Cin = 3 takes
    stem_bf16_v2_kernel (stores through a wave-private LDS tile), Cin = 4 stem_bf16_kernel"""
    B, Ho, Wo = R.bhw(STEM_PIX[name])
    H, W = 2 * Ho - (Ho % 2), 2 * Wo - 1                                 # even and odd input sizes with that output size
    _stem_case(B, Cin, H, W, 8, True, name if name in ("full+1", "ragged") else None)
    if name == "257":
        _stem_case(B, Cin, H, W, 8, False)


@pytest.mark.parametrize("Cin", [1, 3, 4])
@pytest.mark.parametrize("Cout", [8, 16, 24, 32, 40])
def test_stem_widths_and_edges(Cout, Cin):
    for B, H, W in ((2, 9, 13), (1, 1, 1), (3, 2, 1), (2, 1, 2), (1, 2, 37), (2, 31, 2)):
        _stem_case(B, Cin, H, W, Cout, True)
    _stem_case(2, Cin, 9, 13, Cout, False)


# ---- kd_bf16_bilinear_sum --------------------------------------------------------------------------------------------------

def _bilinear_case(B, sizes, Ho, Wo, C, exact, name=None):
    lib, P, stream = _lib()
    wk = R.bilinear_layout(B, Ho, Wo, C)
    what = f"{wk['kernel']} B={B} {sizes} -> {Ho}x{Wo} C={C} {'exact' if exact else 'random'}"
    if name:
        R.on_ladder(name, wk, what)
    g = _gen(B + Ho * 3 + Wo + C)
    ins = [R.exact_acts(g, (B, h, w, C), 100, device="cuda") if exact else torch.randn(B, h, w, C, generator=g, device="cuda").bfloat16() for h, w in sizes]
    a = []
    for i in range(3):
        a += [P(ins[i]), sizes[i][0], sizes[i][1]] if i < len(ins) else [None, 0, 0]
    out = BBuf(B, Ho, Wo, C)
    lib.call("kd_bf16_bilinear_sum", *a, P(out.t), B, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    _check_bf16(what, out.t, R.bilinear_sum(ins, Ho, Wo), R.NONE, None, exact)
    out.guard_ok(what)


@pytest.mark.parametrize("C", [8, 64, 256, 2048])
@pytest.mark.parametrize("nin", [1, 2, 3])
def test_bilinear_ratios(nin, C):
    """identity, 2x and 4x (dyadic interpolation weights: exact inputs, bit for bit; the inputs of one call mix the three ratios)
    and the non-dyadic ratios of tests/test_gpu_tail_kernels.py's RESIZE list (bound)"""
    for ho, wo in ((8, 12), (16, 4)):
        sizes = [(ho, wo), (ho // 2, wo // 2), (ho // 4, wo // 4)]
        for rot in range(3):
            _bilinear_case(2, (sizes[rot:] + sizes[:rot])[:nin], ho, wo, C, True)
    for hi, ho in RESIZE:
        if (hi, ho) in ((16, 64), (64, 16)):                              # dyadic: covered above
            continue
        wi, wo = hi + 3, (ho - 1 if ho > 1 else 5)                        # (a 1 x 1 map would hold 16 outputs, most of them exact ties)
        _bilinear_case(2, [(hi, wi), (max(1, hi // 2), max(1, wi // 2)), (hi, wi)][:nin], ho, wo, C, False)


@pytest.mark.parametrize("name", list(_ladder(1, 2048)))
def test_bilinear_ladder(name):
    """C = 2048: one pixel per block, `full` is 2048 pixels"""
    B, Ho, Wo = R.bhw(_ladder(1, 2048)[name])
    _bilinear_case(B, [(Ho, Wo), (max(1, Ho // 2), max(1, Wo // 2))], Ho, Wo, 2048, False, name)
    half = Ho % 2 == 0 and Wo % 2 == 0                                   # a 2x input where the map allows it, else two identity inputs
    _bilinear_case(B, [(Ho, Wo), (Ho // 2, Wo // 2) if half else (Ho, Wo)], Ho, Wo, 2048, True, name)


# ---- kd_bf16_cls_conv ------------------------------------------------------------------------------------------------------

def _cls_case(M, Cin, NC, exact, name=None):
    lib, P, stream = _lib()
    wk = R.pixel_layout("cls_bf16_kernel", M)
    what = f"cls_bf16_kernel M={M} Cin={Cin} NC={NC} {'exact' if exact else 'random'}"
    if name:
        R.on_ladder(name, wk, what)
    g = _gen(M + Cin + NC)
    B, _, _ = R.bhw(M)
    if exact:
        x, w, b = R.exact_acts(g, (M, Cin), 100, device="cuda"), R.exact_weights(g, NC, Cin, device="cuda"), R.exact_bias(g, NC, device="cuda")
    else:
        x = torch.randn(M, Cin, generator=g, device="cuda").bfloat16()
        w, b = torch.randn(NC, Cin, generator=g, device="cuda"), torch.randn(NC, generator=g, device="cuda")
    logits = Buf(B, NC, M // B)
    lib.call("kd_bf16_cls_conv", P(x), P(w), P(b), P(logits.t), M, M // B, Cin, NC, stream())
    torch.cuda.synchronize()
    z, e = R.cls_conv(x, w, b, B)
    _check(what, logits.t, (z, torch.zeros_like(e) if exact else e))
    logits.guard_ok(what)


@pytest.mark.parametrize("name", list(_ladder(256, 4096)))
def test_cls_ladder(name):
    M = _ladder(256, 4096)[name]
    for exact in (False, True):
        _cls_case(M, 8, 2, exact, name)


@pytest.mark.parametrize("NC", [1, 2, 3, 4])
@pytest.mark.parametrize("Cin", [8, 32, 64])
def test_cls_shapes(Cin, NC):
    """M = 3 * 3011 and 7 * 143: HW does not divide the block, the NCHW index split crosses frames inside a block"""
    for M in (9033, 1001, 1):
        for exact in (False, True):
            _cls_case(M, Cin, NC, exact)


# ---- kd_bf16_weighted_tail -------------------------------------------------------------------------------------------------

def _wt_params():
    lad = _ladder(4, 4096)
    return [(512, n, m) for n, m in lad.items()] + [(c, None, m) for c in (64, 128, 256, 512) for m in (1, 3 * (256 // (c // 8)) + 1, 1000 + c // 64)]


@pytest.mark.parametrize("C,name,M", _wt_params(), ids=lambda v: str(v))
def test_weighted_tail(C, name, M):
    """the softmax tail of the weighted fusion (expf: the bound only).  M ladder at C = 512 (4 rows per block, `full` is 16 384
    rows); M = 1 and M no multiple of the rows per block: the clamped lanes take part in the shuffles."""
    lib, P, stream = _lib()
    wk = R.weighted_tail_layout(M, C)
    what = f"weighted_tail_bf16_kernel M={M} C={C}"
    if name:
        R.on_ladder(name, wk, what)
    g = _gen(M + C)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    h, cat = rnd(M, C).relu().bfloat16(), rnd(M, 2 * C).relu().bfloat16()
    w2, b2 = rnd(2, C) * (2.0 / C ** 0.5), rnd(2) * 0.1
    out = BBuf(M, C)
    lib.call("kd_bf16_weighted_tail", P(h), P(cat), P(w2), P(b2), P(out.t), M, C, stream())
    torch.cuda.synchronize()
    _check_bf16(what, out.t, R.weighted_tail(h, cat, w2, b2))
    out.guard_ok(what)


# ---- argument checks: a negative status and a message that names the function; no kernel is launched ---------------------------

def test_refusals():
    lib, P, stream = _lib()
    ARG, ALIGN, SHAPE = -1, -2, -4
    f = torch.zeros(4096, device="cuda")
    h = torch.zeros(8192, device="cuda", dtype=torch.bfloat16)
    i = torch.zeros(64, device="cuda", dtype=torch.int32)
    pf, ph, pi, s = P(f), P(h), P(i), stream()

    def refused(fn, want, *args):
        rc = getattr(lib, fn)(*args)
        msg = lib.kd_last_error_string().decode()
        assert rc == want and fn in msg, (fn, rc, want, msg)

    dw = lambda **k: (k.get("x", ph), pf, pf, pf, 1, k.get("y", ph), k.get("B", 1), k.get("H", 4), k.get("W", 4), k.get("C", 8), 1, s)
    for bad in (dict(C=0), dict(H=0), dict(W=0), dict(H=-1), dict(C=12), dict(C=1032)):
        refused("kd_bf16_dwconv3x3", ARG, *dw(**bad))
    refused("kd_bf16_dwconv3x3", ALIGN, *dw(x=ph + 2))
    bl = lambda **k: (k.get("in0", ph), k.get("H0", 4), k.get("W0", 4), k.get("in1", None), k.get("H1", 0), k.get("W1", 0), None, 0, 0,
                      k.get("out", ph), 1, k.get("Ho", 4), k.get("Wo", 4), k.get("C", 8), s)
    for bad in (dict(C=0), dict(Ho=0), dict(Wo=0), dict(H0=0), dict(W0=-2), dict(in1=ph, H1=0, W1=4)):
        refused("kd_bf16_bilinear_sum", ARG, *bl(**bad))
    for bad in (dict(in0=ph + 2), dict(out=ph + 8), dict(in1=ph + 4, H1=4, W1=4)):
        refused("kd_bf16_bilinear_sum", ALIGN, *bl(**bad))
    refused("kd_bf16_stem", ALIGN, pf, pf, pf, pf, 1, ph + 2, 1, 3, 4, 4, 8, s)
    refused("kd_bf16_stem", ARG, pf, pf, pf, pf, 1, ph, 1, 3, 0, 4, 8, s)
    refused("kd_bf16_stem", SHAPE, pf, pf, pf, pf, 1, ph, 1, 3, 4, 4, 12, s)
    refused("kd_bf16_cls_conv", ALIGN, ph + 2, pf, pf, pf, 4, 4, 8, 2, s)
    refused("kd_bf16_cls_conv", ARG, ph, pf, pf, pf, 4, 0, 8, 2, s)
    refused("kd_bf16_cls_conv", ARG, ph, pf, pf, pf, 4, 4, 0, 2, s)

    def pw(**k):
        return (k.get("A", ph), k.get("lda", 32), k.get("a_kind", 0), pf, pf, pf, pf, 1, k.get("C", ph), k.get("ldc", 32), k.get("res", None),
                k.get("ldres", 0), k.get("epi", 0), 4, 32, 32, None, k.get("l0", None), k.get("l0", None), k.get("l0", None), k.get("l0", None), 1,
                k.get("cell", None), k.get("grid", None), k.get("ldgrid", 0), s)
    refused("kd_bf16_pwconv", ALIGN, *pw(A=pf + 4, lda=4, a_kind=3, l0=pf))          # the points are read with 16-byte loads
    refused("kd_bf16_pwconv", ARG, *pw(epi=4, cell=pi, grid=pf, ldgrid=16))
    refused("kd_bf16_pwconv", ARG, *pw(lda=24))
    refused("kd_bf16_pwconv", ARG, *pw(a_kind=1, A=pf, lda=28))
    refused("kd_bf16_pwconv", ARG, *pw(ldc=30))
    refused("kd_bf16_pwconv", ARG, *pw(res=ph, ldres=16))
    refused("kd_bf16_pwconv", ALIGN, *pw(C=ph + 2))
    refused("kd_bf16_pwconv", ALIGN, *pw(res=ph + 2, ldres=32))
    refused("kd_bf16_pwconv", ALIGN, *pw(A=ph + 2))
    torch.cuda.synchronize()
    assert bool((f == 0).all()) and bool((h == 0).all())


def test_zz_report_peak_memory():
    """the figures for this file's docstring (runs last in the file)"""
    print(f"test_gpu_bf16_kernels.py: {time.time() - _T0:.1f} s wall, peak allocated {torch.cuda.max_memory_allocated() / 2 ** 20:.0f} MiB")
