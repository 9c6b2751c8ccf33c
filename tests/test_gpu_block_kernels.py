"""The fused inference block kernels of csrc/kd_block.hip called directly through the C ABI -- kd_dw_pw_infer (dw_pw_infer_kernel:
stride 1 with 32 and 64 output channels, stride 2 with 64) and kd_block_infer (block_infer_kernel: 64 -> Ch -> 64 at stride 1,
32 -> Ch -> 64 at stride 2) -- against a float64 evaluation of the same operation on the same fp32 inputs (tests/_fp64_block_ref.py,
plain torch on the GPU) within C_BOUND * n_seq * 2^-24 * sum|t_i| per output, bit for bit on inputs whose every intermediate is
exact, and one product at a time through each matrix phase.  No element is left out of any comparison.

Every output starts as NaN and carries a sentinel guard tail; strided outputs keep their padding columns; x is the middle B images
of a B + 2 image buffer whose first and last images are NaN; every weight and coefficient vector sits at a 16-byte-aligned offset
inside a NaN buffer; the residual is a column slice of a wider NaN buffer; about a third of all BatchNorm scales are negative.  The
kernels use the split arithmetic whatever the process-wide switch says, so nothing here runs once per arithmetic.

The case table (R.CASES, 7 per instance) lets every map -- 1 x 1, 1 x 23, 23 x 1, smaller than a tile, exactly one tile, one pixel
over, 3 x 3 tiles with partial last ones; at stride 2 a last halo row outside and inside the image -- every hidden width (one chunk,
one prefetch, an odd chunk count, the teacher's 192 / 384), B = 1 and 3 and every argument variant meet every instance
(tests/test_fp64_block_ref_host.py::test_case_table_covers_every_value).

Kernel -> tests: test_float64, test_exact (no tolerance: a dropped tap, a misplaced halo pixel, a swapped chunk, a wrong pixel-to-row
map or column cannot hide), test_single_product (|got - x*y| <= SPLIT_PRODUCT_U * U |x||y|), test_goes_red (the
comparisons of test_float64 and test_exact FAIL on the real kernel output against three wrong references), test_refusals,
test_dispatch_at_the_default_modes (the shape rules production runs).

Measured on an MI355X: this file 3.7 s of wall time (86 cases; 4.2 s in a second session), next to 6.5 s for tests/test_gpu_gemm_fp64.py in the same session;
after the first case (0.8 s) none above 0.3 s (the 278 k-product probes), the table's cases 0.01 s each.

Worst error / bound per instance over the table: kd_dw_pw_infer stride 1 / Cout 32 0.008, stride 1 / Cout 64 0.019, stride 2 / Cout 64
0.019; kd_block_infer 64 -> Ch -> 64 at stride 1 0.006, 32 -> Ch -> 64 at stride 2 0.007 (the teacher's widths on the largest maps
0.001 - 0.004).  The bounds are worst-case chains: the three wrong references of test_goes_red miss them by factors of 4.6e3 and more.
test_exact is bit-equal on all 35 cases: v_mfma_f32_32x32x16_bf16 returns the exact sum when every product and partial sum is
representable.  Single products, worst |got - x*y| / (U |x||y|): project phase 2.29 / 2.32 / 2.48 (the three kd_dw_pw_infer instances,
139 k - 278 k products each), expand phase 2.18 (Cin 64, 123 k products) and 2.00 (Cin 32, 39 k) -- inside the 2.36 - 2.65 of the GEMM
family and the documented 3.97.  No test here has found a fault in the kernels."""
import functools

import pytest
import torch

import _fp64_block_ref as R
from test_gpu_gemm_fp64 import SPLIT_PRODUCT_U, Out, _ld, _shares, _wide
from test_gpu_tail_kernels import NAN, Buf

pytestmark = pytest.mark.gpu

KD_ERR_ARG, KD_ERR_ALIGN, KD_ERR_SHAPE = -1, -2, -4
VECTORS = ("isc", "ish", "we", "ebias", "esc", "esh", "wd", "dsc", "dsh", "wp", "pbias", "psc", "psh")
WORST = {}                  # instance -> worst error / bound seen in this session
PROBE = {}                  # (matrix phase, instance) -> worst |got - x*y| / (U |x||y|)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _run.cache_clear()
    print()
    for k in sorted(WORST):
        print("RATIO", k, f"{WORST[k]:.4f}")
    for k in sorted(PROBE):
        print("PROBE", *k, f"{PROBE[k]:.4f}")


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import stream
    return lib, stream


def _nanpad(t):
    """t at a 16-byte-aligned offset inside a NaN buffer, NaN on both sides"""
    if t is None:
        return None
    buf = torch.full((t.numel() + 8,), NAN, device=t.device)
    v = buf[4:4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 0
    return v


def _poisoned(c, d):
    """the tensors of case c as the kernel gets them: x between two NaN images, the vectors inside NaN buffers, the residual a column
    slice of a wider NaN buffer"""
    t = dict(d)
    xb = torch.full((c.B + 2, *d["x"].shape[1:]), NAN, device="cuda")
    xb[1:-1] = d["x"]
    t["x"] = xb[1:-1]
    for k in VECTORS:
        t[k] = _nanpad(d.get(k))
    t["res"] = _wide(d["res"], 8, 4)
    return t


def _call_args(c, t, out, ldo, ldres=None, off=()):
    """the entry point's name followed by its arguments; off: the operands whose pointer is moved by one float"""
    _, stream = _lib()
    fn, s, Cin, Cout = R.INST[c.inst]
    p = lambda k: None if t.get(k) is None else t[k].data_ptr() + (4 if k in off else 0)
    tail = (p("wd"), p("dsc"), p("dsh"), t["dact"], p("wp"), p("pbias"), p("psc"), p("psh"), t["pact"], p("res"),
            _ld(t["res"]) if ldres is None else ldres, out.data_ptr(), ldo, c.B, c.H, c.W)
    if fn == "kd_dw_pw_infer":
        return fn, p("x"), p("isc"), p("ish"), t["iact"], *tail, c.Ch, s, Cout, stream()
    return fn, p("x"), p("we"), p("ebias"), p("esc"), p("esh"), t["eact"], *tail, Cin, c.Ch, s, Cout, stream()


def _launch(c, d, what):
    """one launch on poisoned operands -> the [Mo, Cout] output, its guard tail and padding columns checked"""
    lib, _ = _lib()
    _, s, _, Cout = R.INST[c.inst]
    Mo = c.B * R._out_size(c.H, s) * R._out_size(c.W, s)
    t = _poisoned(c, d)
    o = Out(Mo, Cout, c.pad) if c.pad else Buf(Mo, Cout)
    lib.call(*_call_args(c, t, o.t, Cout + c.pad))
    torch.cuda.synchronize()
    o.intact(what) if c.pad else o.guard_ok(what)
    return o.t.clone()


@functools.lru_cache(maxsize=None)
def _run(c, exact):
    """(fp32 inputs, kernel output) of case c: launched once, shared by the tests that look at it"""
    d = R.inputs(torch.Generator(device="cuda").manual_seed(R.seed_of(c, exact)), c, exact)
    return d, _launch(c, d, f"{R.case_id(c)}{' exact' if exact else ''}")


def _ratio(got, ref):
    val, err = ref
    return ((got.double() - val).abs() / err.clamp_min(1e-300)).max().item()


def _check(what, key, got, ref):
    val, err = ref
    got = got.double().reshape(val.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements never written"
    d = (got - val).abs()
    r = (d / err.clamp_min(1e-300)).max().item()
    print(f"\nCASE {what} worst error / bound {r:.4f}")
    WORST[key] = max(WORST.get(key, 0.0), r)
    if r > 1.0:
        bad = d > err
        i = int(torch.nonzero(bad.reshape(-1))[0])
        pytest.fail(f"{what}: {int(bad.sum())} of {val.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                    f"got {got.reshape(-1)[i].item():.9g}, float64 {val.reshape(-1)[i].item():.9g}, bound {err.reshape(-1)[i].item():.3g}")


# ---- float64, exact integers ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_float64(c):
    d, got = _run(c, False)
    pre = {}
    ref = R.reference(c, R.to_double(d), pre=pre)
    for what, raw, sc, sh in R.relu6_operands(c, d, pre):
        _shares(raw, sc, sh, f"[{what} of {R.case_id(c)}]")
    _check(R.case_id(c), c.inst, got, ref)


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_exact(c):
    """inputs on which every intermediate is exact in fp32 and in the three-piece split: the float64 value bit for bit"""
    d, got = _run(c, True)
    pre = {}
    val = R.reference(c, R.to_double(d), pre=pre)[0]
    assert R.exact_headroom(pre) < 2 ** 24, "the recipe's project sums are not exact in fp32"
    for what, raw, sc, sh in R.relu6_operands(c, d, pre):
        _shares(raw, sc, sh, f"[{what} of {R.case_id(c)}, exact recipe]")
    got = got.double()
    assert not bool(torch.isnan(got).any()), f"{int(torch.isnan(got).sum())} elements never written"
    if not torch.equal(got, val):
        bad = got != val
        i = int(torch.nonzero(bad.reshape(-1))[0])
        pytest.fail(f"{int(bad.sum())} of {val.numel()} elements differ from float64 (largest deviation {(got - val).abs().max().item():.6g}); "
                    f"first at flat index {i}: got {got.reshape(-1)[i].item():.12g}, float64 {val.reshape(-1)[i].item():.12g}")


# ---- one product per output element ------------------------------------------------------------------------------------------

def _unit_tail(Ch, Cout):
    wd = torch.zeros(Ch, 9, device="cuda")
    wd[:, 4] = 1.0
    one, zero = (lambda n: torch.ones(n, device="cuda")), (lambda n: torch.zeros(n, device="cuda"))
    return dict(wd=wd, dsc=one(Ch), dsh=zero(Ch), dact=0, pbias=None, psc=one(Cout), psh=zero(Cout), pact=0, res=None)


def _probe(phase, inst, c, d, exact):
    got = _launch(c, d, f"single product, {phase} of {inst}").double()
    assert not bool(torch.isnan(got).any()), f"[{inst}] elements never written"
    ratio = ((got - exact).abs() / (R.U * exact.abs())).max().item()
    PROBE[(phase, inst)] = ratio
    print(f"\nPROBE {phase} {inst} worst |got - x*y| / (U |x||y|) = {ratio:.4f} over {exact.numel()} products")
    assert ratio <= SPLIT_PRODUCT_U, f"[{inst}] per-product error {ratio:.4f} U |x||y| exceeds {SPLIT_PRODUCT_U} U |x||y|"


def _single_product_project(inst, Ch):
    """Centre tap 1, unit affines, no activation, bias or residual; x non-zero in channel m mod Ch of the input pixel of output pixel
    m, full 24-bit mantissas: out[m, n] = x[m] * wp[n, m mod Ch] is one product of the project GEMM and every other accumulation
    an exact add of zero.  Every channel occurs in every 32-row block of the pixel tile."""
    _, s, _, Cout = R.INST[inst]
    B, Ho, Wo = 2, 41, 53
    H, W = s * (Ho - 1) + 1, s * (Wo - 1) + 1
    g = torch.Generator(device="cuda").manual_seed(Ch + s)
    Mo = B * Ho * Wo
    m = torch.arange(Mo, device="cuda")
    ch, ox, oy, b = m % Ch, m % Wo, (m // Wo) % Ho, m // (Ho * Wo)
    TW = 16 if s == 1 else 8
    rb = ((oy % 8) * TW + ox % TW) // 32
    for i in range(8 * TW // 32):
        assert ch[rb == i].unique().numel() == Ch, f"row block {i} of the tile does not meet every channel"
    xv, wp = R.probe_values(g, Mo), R.probe_values(g, Cout, Ch)
    x = torch.zeros(B, H, W, Ch, device="cuda")
    x[b, s * oy, s * ox, ch] = xv
    c = R.Case(inst, B, H, W, Ch, "asis", 0, 0, False, False, 0, None, None)
    d = dict(x=x, isc=None, ish=None, iact=0, wp=wp, stride=s, **_unit_tail(Ch, Cout))
    _probe("project", inst, c, d, xv.double()[:, None] * wp.double()[:, ch].t())


def _single_product_expand(inst, Ch):
    """Ch = 64, wp the identity, centre tap 1, unit affines; x non-zero in input channel m mod Cin of pixel m:
    out[m, n] = fl(x[m] * we[n, m mod Cin]) is one product of the expand GEMM, the project by the identity is exact."""
    _, s, Cin, Cout = R.INST[inst]
    B, H, W = (2, 24, 40) if s == 1 else (2, 33, 35)
    g = torch.Generator(device="cuda").manual_seed(Cin + s)
    M = B * H * W
    m = torch.arange(M, device="cuda")
    ch = m % Cin
    xv, we = R.probe_values(g, M), R.probe_values(g, Ch, Cin)
    x = torch.zeros(M, Cin, device="cuda")
    x[m, ch] = xv
    c = R.Case(inst, B, H, W, Ch, None, 0, 0, False, False, 0, 0, False)
    d = dict(x=x.view(B, H, W, Cin), we=we, ebias=None, esc=torch.ones(Ch, device="cuda"), esh=torch.zeros(Ch, device="cuda"), eact=0,
             wp=torch.eye(Cout, Ch, device="cuda"), stride=s, **_unit_tail(Ch, Cout))
    exact = (xv.double()[:, None] * we.double()[:, ch].t()).view(B, H, W, Ch)[:, ::s, ::s].reshape(-1, Ch)
    _probe("expand", inst, c, d, exact)


@pytest.mark.parametrize("inst,Ch", [("dwpw_s1_32", 96), ("dwpw_s1_64", 384), ("dwpw_s2_64", 192), ("block_s1", 64), ("block_s2", 64)])
def test_single_product(inst, Ch):
    """the probe of tests/test_gpu_gemm_fp64.py carried through the fused kernels: the project phase through kd_dw_pw_infer, the
    expand phase through kd_block_infer"""
    (_single_product_project if R.INST[inst][0] == "kd_dw_pw_infer" else _single_product_expand)(inst, Ch)


# ---- negative controls on the real kernel output -----------------------------------------------------------------------------

@pytest.mark.parametrize("inst", list(R.INST))
def test_goes_red(inst):
    """the comparisons of test_float64 and test_exact fail against a reference with the residual omitted, one tap dropped, the
    border padded with act(sh) -- on the outputs those tests looked at (launched once: _run)"""
    c = R.red_case(inst)
    d, got = _run(c, False)
    dx, gotx = _run(c, True)
    d, dx = R.to_double(d), R.to_double(dx)
    assert _ratio(got, R.reference(c, d)) <= 1.0 and torch.equal(gotx.double(), R.reference(c, dx)[0])
    for w in ("no_res", "tap", "border"):
        r = _ratio(got, R.reference(c, d, wrong=w))
        print(f"\nWRONG {R.case_id(c)} {w}: {r:.3g}x the bound")
        assert r > 1.0, f"the float64 comparison passes with {R.WRONGS[w]} ({r:.3g}x the bound)"
        assert not torch.equal(gotx.double(), R.reference(c, dx, wrong=w)[0]), f"the exact comparison passes with {R.WRONGS[w]}"


# ---- refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", list(R.INST))
def test_refusals(inst):
    """each call returns its error code and launches nothing: the output is still all NaN afterwards"""
    lib, _ = _lib()
    c = R.red_case(inst)
    fn, s, _, Cout = R.INST[inst]
    d = R.inputs(torch.Generator(device="cuda").manual_seed(5), c)
    t = _poisoned(c, d)
    out = Buf(c.B * R._out_size(c.H, s) * R._out_size(c.W, s), Cout)
    rc = lambda **kw: getattr(lib, fn)(*_call_args(c, t, out.t, kw.pop("ldo", Cout), **kw)[1:])
    for k in ("x", "wd", "wp", "dsc") + (("we",) if fn == "kd_block_infer" else ()):
        assert rc(off=(k,)) == KD_ERR_ALIGN, f"{fn}: {k} offset by one float"
    assert rc(ldo=Cout - 1) == KD_ERR_SHAPE, f"{fn}: ldo < Cout"
    assert rc(ldres=Cout - 1) == KD_ERR_SHAPE, f"{fn}: ldres < Cout with a residual"
    t["ish" if fn == "kd_dw_pw_infer" else "esh"] = None
    assert rc() == KD_ERR_ARG, f"{fn}: a scale without its shift"
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all()), f"{fn}: a refused call launched"
    out.guard_ok(fn)


# ---- dispatch at the default modes -------------------------------------------------------------------------------------------

def test_dispatch_at_the_default_modes():
    """DW_PW_FUSED = [1], BLOCK_INFER = [1], split arithmetic, eval under no_grad: which entry point each module reaches"""
    from kdrt import ops, units
    from src.models.camera_encoder import InvertedResidual
    from src.models.fusion_module import DWSeparableConv
    assert units.DW_PW_FUSED == [1] and units.BLOCK_INFER == [1]
    torch.manual_seed(11)
    table = [(InvertedResidual(32, 64, stride=2), 32, {"kd_block_infer"}),
             (InvertedResidual(64, 64, stride=1), 64, {"kd_block_infer"}),
             (InvertedResidual(64, 128, stride=2), 64, set()),
             (DWSeparableConv(128, 128), 128, set()),
             (InvertedResidual(64, 64, stride=2), 64, {"kd_dw_pw_infer"}),       # Ch 384 -> 64 at stride 2: not a whole supported block
             (DWSeparableConv(192, 64), 192, {"kd_dw_pw_infer"})]
    calls = []
    real_call = units.lib.call
    prev = ops.set_gemm_arithmetic("split")
    try:
        units.lib.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
        for m, cin, want in table:
            m = m.cuda().eval()
            x = torch.randn(2, cin, 9, 17, generator=torch.Generator().manual_seed(cin)).cuda()
            calls.clear()
            with torch.no_grad():
                y = m(x)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all())
            assert {n for n in calls if n in ("kd_block_infer", "kd_dw_pw_infer")} == want, (type(m).__name__, cin, calls)
    finally:
        del units.lib.__dict__["call"]                     # (the instance attribute: the class's method is back)
        ops.set_gemm_arithmetic(prev)
