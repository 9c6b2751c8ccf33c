"""Self-check of tests/_fp64_gemm_ref.py on the host: the references ARE the 1x1 convolution's forward and backward (compared
with torch.autograd in float64), their bounds hold for an honest fp32 evaluation and reject six wrong readings of the contract,
the launch-layout mirrors equal the library's host-side answers, and the emulated split product separates the shipped six
piece products from the leading three."""
import pytest
import torch
import torch.nn.functional as F

import _fp64_gemm_ref as R

EPS = 1e-5
FWD = [(333, 64, 128), (257, 32, 192), (37, 36, 20)]               # (M, K, N) of the GPU suite's recipes
DGRAD = [(333, 128, 64), (257, 64, 192), (37, 20, 36)]             # (M, Kred, Nout)
WGRAD = [(777, 128, 64), (333, 64, 192), (37, 20, 36)]             # (M, N, K)


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _d(t):
    if isinstance(t, (tuple, list)):
        return tuple(_d(v) for v in t)
    if isinstance(t, dict):
        return {k: _d(v) for k, v in t.items()}
    return t.double() if torch.is_tensor(t) else t


def _missed(wrong, ref):
    """share of the elements at which `wrong` lies outside the bound of the reference"""
    val, err = ref
    return ((wrong - val).abs() > err).double().mean().item()


def _shares(x, sc, sh, what):
    lo, mid, hi = R.relu6_shares(x, sc, sh)
    assert min(lo, mid, hi) >= 0.01, f"ReLU6 inputs must exercise both clamps {what}: {lo:.3f} / {mid:.3f} / {hi:.3f}"


# ---- the references are autograd ---------------------------------------------------------------------------------------------

def _bn_coeffs(y, gamma, beta, training, rm, rv):
    mean, var = (y.mean(0), y.var(0, unbiased=False)) if training else (rm, rv)
    inv = 1.0 / torch.sqrt(var + EPS)
    sc = gamma * inv
    return sc, beta - mean * sc, mean, inv


def _finalize(Gm, y, gamma, mean, inv, training):
    """al, be, ga as bwd_finalize_tail of csrc/kd_bn.hip defines them from s1 = sum Gm, s2 = sum Gm * xhat"""
    a = gamma * inv
    if not training:
        return a, torch.zeros_like(a), torch.zeros_like(a)
    c1, c2 = Gm.sum(0) / y.shape[0], (Gm * (y - mean) * inv).sum(0) / y.shape[0]
    return a, -a * c2 * inv, a * (c2 * inv * mean - c1)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("act_id,training", [(2, True), (1, True), (2, False), (1, False)])
def test_references_equal_autograd(act_id, training, residual):
    g = _gen(act_id, training, residual, 5)
    M, C0, C1, C2 = 192, 8, 12, 16
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W1, W2 = r(M, C0), r(C1, C0) / C0 ** 0.5, r(C2, C1) / C1 ** 0.5
    g1, b1, g2, b2 = r(C1).abs() + 2.0, r(C1) + 3.0, r(C2).abs() + 2.0, r(C2) + 3.0
    rm1, rv1, rm2, rv2 = r(C1) * 0.1, r(C1).abs() + 0.5, r(C2) * 0.1, r(C2).abs() + 0.5
    Rh, Ra = r(M, C2), (r(M, C1) if residual else None)
    leaves = [x, W1, W2, g1, b1, g2, b2]
    for t in leaves:
        t.requires_grad_(True)
    fact = (lambda z: z.clamp(0, 6)) if act_id == 2 else (lambda z: z.clamp_min(0))
    y1 = x @ W1.t()
    z1 = F.batch_norm(y1, rm1.clone(), rv1.clone(), g1, b1, training, 0.1, EPS)
    a1 = fact(z1)
    y2 = a1 @ W2.t()
    z2 = F.batch_norm(y2, rm2.clone(), rv2.clone(), g2, b2, training, 0.1, EPS)
    h = fact(z2)
    for t in (y1, z1, a1, y2, z2):
        t.retain_grad()
    loss = (h * Rh).sum() + ((a1 * Ra).sum() if residual else 0.0)
    loss.backward()
    with torch.no_grad():
        sc1, sh1, mean1, inv1 = _bn_coeffs(y1, g1, b1, training, rm1, rv1)
        sc2, sh2, mean2, inv2 = _bn_coeffs(y2, g2, b2, training, rm2, rv2)
        _shares(y1, sc1, sh1, "layer 1") if act_id == 2 else None
        close = lambda got, want, what: torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-10, msg=lambda m: f"{what}: {m}")
        # forward: deferred BatchNorm + activation on load; the inference epilogue of epi 5
        f = R.gemm_fwd(y1, W2, pro=1, pro_act=act_id, sc=sc1, sh=sh1, epi=1)
        close(f["c"][0], y2, "forward")
        close(f["s1"][0], y2.sum(0), "forward s1")
        close(f["s2"][0], (y2 * y2).sum(0), "forward s2")
        close(R.gemm_fwd(y1, W2, pro=1, pro_act=act_id, sc=sc1, sh=sh1, epi=5, esc=sc2, esh=sh2, epi_act=act_id,
                         addend=Rh if residual else None)["c"][0], h + (Rh if residual else 0.0), "epi 5")
        # data gradient of conv 2 with BatchNorm 2's backward folded into the load, mask on (G = dL/dh) and off (G = dL/dz2)
        Gm = z2.grad
        al, be, ga = _finalize(Gm, y2, g2, mean2, inv2, training)
        for G, msc, msh, pa, what in ((Rh, sc2, sh2, act_id, "mask on"), (Gm, None, None, 0, "mask off")):
            d0 = R.gemm_dgrad(G, y2, W2.t(), al, be, ga, msc, msh, pa, addend=Ra, epi=0)
            close(d0["c"][0], a1.grad, f"data gradient, epi 0, {what}")
            d2 = R.gemm_dgrad(G, y2, W2.t(), al, be, ga, msc, msh, pa, addend=Ra, epi=2, X=y1, esc=sc1, esh=sh1, mean=mean1,
                              invstd=inv1, epi_act=act_id)
            close(d2["c"][0], z1.grad, f"data gradient, epi 2, {what}")
            close(d2["s1"][0], b1.grad, f"BatchNorm-backward s1, {what}")
            close(d2["s2"][0], g1.grad, f"BatchNorm-backward s2, {what}")
            w = R.gemm_wgrad(G, y2, al, be, ga, msc, msh, 2, pa, y1, sc1, sh1, 1, act_id, 0)
            close(w["dw"][0], W2.grad, f"weight gradient, {what}")
        # conv 1: BatchNorm 1's backward folded in, plain operand
        al1, be1, ga1 = _finalize(z1.grad, y1, g1, mean1, inv1, training)
        close(R.gemm_wgrad(a1.grad, y1, al1, be1, ga1, sc1, sh1, 2, act_id, x, None, None, 0, 0, 0)["dw"][0], W1.grad, "weight gradient 1")
        close(R.gemm_dgrad(a1.grad, y1, W1.t(), al1, be1, ga1, sc1, sh1, act_id)["c"][0], x.grad, "data gradient 1")
        close(R.gemm_wgrad(y1.grad, None, None, None, None, None, None, 0, 0, x, None, None, 0, 0, 0)["dw"][0], W1.grad, "plain weight gradient")


# ---- the bounds hold for honest fp32 -----------------------------------------------------------------------------------------

def _within(r32, r64, what):
    for k, (val, err) in r64.items():
        d = (r32[k][0].double() - val).abs()
        assert bool((d <= err).all()), f"{what} [{k}]: fp32 evaluation {(d / err.clamp_min(1e-300)).max().item():.3g}x the bound"


@pytest.mark.parametrize("M,K,N", FWD)
def test_forward_bounds_hold_for_fp32(M, K, N):
    inp = R.fwd_inputs(_gen(M, K, N), M, K, N)
    if M * K >= 4096:
        _shares(inp["A"], *inp["pro"][2], f"[forward {M}x{K}]")
    for form in ("tiled", "stream"):
        for what, kw in R.fwd_cases(inp):
            n_part = R.gemm_layout(M, K, N, kw["pro"], kw["epi"], kw["addend"] is not None, form)["n_part"]
            _within(R.gemm_fwd(inp["A"], inp["W"], n_part=n_part, **kw), R.gemm_fwd(_d(inp["A"]), _d(inp["W"]), n_part=n_part, **_d(kw)),
                    f"forward {form} {(M, K, N)} {what}")


@pytest.mark.parametrize("M,Kred,Nout", DGRAD)
def test_data_gradient_bounds_hold_for_fp32(M, Kred, Nout):
    inp = R.dgrad_inputs(_gen(M, Kred, Nout, 1), M, Kred, Nout)
    if M * Kred >= 4096:
        _shares(inp["Y"], *inp["pro"][2], f"[data gradient operand {M}x{Kred}]")
        _shares(inp["X"], *inp["epi"][2][:2], f"[data gradient epilogue {M}x{Nout}]")
    for form in ("tiled", "stream"):
        for what, kw in R.dgrad_cases(inp):
            n_part = R.gemm_layout(M, Kred, Nout, 2, kw["epi"], kw["addend"] is not None, form)["n_part"]
            _within(R.gemm_dgrad(inp["G"], inp["Y"], inp["Wt"], n_part=n_part, **kw),
                    R.gemm_dgrad(_d(inp["G"]), _d(inp["Y"]), _d(inp["Wt"]), n_part=n_part, **_d(kw)), f"data gradient {form} {(M, Kred, Nout)} {what}")


@pytest.mark.parametrize("M,N,K", WGRAD)
def test_weight_gradient_bounds_hold_for_fp32(M, N, K):
    inp = R.wgrad_inputs(_gen(M, N, K, 2), M, N, K)
    if M * N >= 4096:
        _shares(inp["X"], *inp["d"][2], f"[weight gradient D {M}x{N}]")
        _shares(inp["A"], *inp["a"][2], f"[weight gradient A {M}x{K}]")
    for form in ("tiled", "rs"):
        n_red = R.wgrad_layout(M, N, K, form)["n_red"]
        for what, args in R.wgrad_cases(inp):
            _within(R.gemm_wgrad(inp["D"], inp["X"], *args, n_red), R.gemm_wgrad(_d(inp["D"]), _d(inp["X"]), *_d(args), n_red),
                    f"weight gradient {form} {(M, N, K)} {what}")


# ---- the bounds have teeth ---------------------------------------------------------------------------------------------------

def _bites(wrong, ref, keys, what):
    for k in keys:
        share = _missed(wrong[k], ref[k])
        assert share >= 0.01, f"{what}: the wrong reference misses the bound of [{k}] on only {share:.4f} of its elements"


@pytest.mark.parametrize("M,Kred,Nout", DGRAD)
def test_teeth_of_the_data_gradient_bounds(M, Kred, Nout):
    inp = _d(R.dgrad_inputs(_gen(M, Kred, Nout, 1), M, Kred, Nout))
    G, Y, Wt, X, add = (inp[k] for k in ("G", "Y", "Wt", "X", "addend"))
    al, be, ga = inp["fold"]
    msc, msh = inp["pro"][2]
    esc, esh, mean, inv = inp["epi"][2]
    val = lambda r: {k: v[0] for k, v in r.items()}
    for form in ("tiled", "stream"):
        lay = R.gemm_layout(M, Kred, Nout, 2, 2, True, form)
        kw = dict(addend=add, epi=2, X=X, esc=esc, esh=esh, mean=mean, invstd=inv, n_part=lay["n_part"])
        ref = R.gemm_dgrad(G, Y, Wt, al, be, ga, msc, msh, 2, epi_act=2, **kw)
        # ReLU6 masks without the z < 6 test: the operand's, then the epilogue's
        _bites(val(R.gemm_dgrad(G, Y, Wt, al, be, ga, msc, msh, 1, epi_act=2, **kw)), ref, ("c", "s1", "s2"), f"{form}: operand mask without z < 6")
        _bites(val(R.gemm_dgrad(G, Y, Wt, al, be, ga, msc, msh, 2, epi_act=1, **kw)), ref, ("c", "s1", "s2"), f"{form}: epilogue mask without z < 6")
        # the addend applied after the epi 2 mask
        c = R.gemm_dgrad(G, Y, Wt, al, be, ga, msc, msh, 2, epi_act=2, **{**kw, "addend": None})["c"][0] + add
        _bites({"c": c, "s1": c.sum(0), "s2": (c * (X - mean) * inv).sum(0)}, ref, ("c", "s1", "s2"), f"{form}: addend after the mask")
        # be * Y dropped from the operand
        _bites(val(R.gemm_dgrad(G, Y, Wt, al, torch.zeros_like(be), ga, msc, msh, 2, epi_act=2, **kw)), ref, ("c", "s1", "s2"), f"{form}: be*Y dropped")
        # one statistics-slab row left out
        row = R.slab_row_of(M, lay)
        for j in {0, int(row.max())}:
            _bites(val(R.gemm_dgrad(G, Y, Wt, al, be, ga, msc, msh, 2, epi_act=2, rowsel=row != j, **kw)), ref, ("s1", "s2"), f"{form}: slab row {j} left out")


@pytest.mark.parametrize("M,K,N", FWD)
def test_teeth_of_the_forward_bounds(M, K, N):
    inp = _d(R.fwd_inputs(_gen(M, K, N), M, K, N))
    A, W, bias, add = (inp[k] for k in ("A", "W", "bias", "addend"))
    sc, sh = inp["pro"][2]
    val = lambda r: {k: v[0] for k, v in r.items()}
    for form in ("tiled", "stream"):
        lay = R.gemm_layout(M, K, N, 1, 1, False, form)
        kw = dict(pro=1, pro_act=2, sc=sc, sh=sh, n_part=lay["n_part"])
        ref = R.gemm_fwd(A, W, bias=bias, epi=1, **kw)
        _bites(val(R.gemm_fwd(A, W, bias=None, epi=1, **kw)), ref, ("c", "s1", "s2"), f"{form}: bias dropped")
        row = R.slab_row_of(M, lay)
        for j in {0, int(row.max())}:
            _bites(val(R.gemm_fwd(A, W, bias=bias, epi=1, rowsel=row != j, **kw)), ref, ("s1", "s2"), f"{form}: slab row {j} left out")
    for ea in (1, 2):
        esc, esh = inp["epi"][ea]
        kw = dict(pro=1, pro_act=2, sc=sc, sh=sh, bias=bias, epi=5, esc=esc, esh=esh)
        ref = R.gemm_fwd(A, W, addend=add, epi_act=ea, **kw)
        z = R.gemm_fwd(A, W, addend=None, epi_act=0, **kw)["c"][0]
        _bites({"c": R.act(z + add, ea)}, ref, ("c",), f"epi 5, act {ea}: residual before the activation")
        _bites(val(R.gemm_fwd(A, W, addend=add, epi_act=ea, **{**kw, "bias": None})), ref, ("c",), f"epi 5, act {ea}: bias dropped")


@pytest.mark.parametrize("M,N,K", WGRAD)
def test_teeth_of_the_weight_gradient_bounds(M, N, K):
    inp = _d(R.wgrad_inputs(_gen(M, N, K, 2), M, N, K))
    D, X, A = inp["D"], inp["X"], inp["A"]
    al, be, ga = inp["fold"]
    msc, msh = inp["d"][2]
    asc, ash = inp["a"][2]
    for form in ("tiled", "rs"):
        n_red = R.wgrad_layout(M, N, K, form)["n_red"]
        ref = R.gemm_wgrad(D, X, al, be, ga, msc, msh, 2, 2, A, asc, ash, 1, 2, n_red)
        _bites({"dw": R.gemm_wgrad(D, X, al, be, ga, msc, msh, 2, 1, A, asc, ash, 1, 2, n_red)["dw"][0]}, ref, ("dw",), f"{form}: mask without z < 6")
        _bites({"dw": R.gemm_wgrad(D, X, al, torch.zeros_like(be), ga, msc, msh, 2, 2, A, asc, ash, 1, 2, n_red)["dw"][0]}, ref, ("dw",),
               f"{form}: be*X dropped")


# ---- the single-product probe has teeth --------------------------------------------------------------------------------------

def test_split_product_emulation():
    g = _gen(24)
    n = 1 << 20
    x, y = R.probe_values(g, n), R.probe_values(g, n)
    assert bool((x.abs().frexp().exponent.unique().numel() > 8)), "mixed exponents"
    hi, mid, lo = R.split3(x)
    assert bool(((hi.double() + mid.double() + lo.double() - x.double()).abs() <= 2.0 ** -26 * x.abs().double()).all())
    exact = x.double() * y.double()                                   # 48 significant bits: exact in float64
    ratio = lambda got: (got.double() - exact).abs() / (R.U * exact.abs())
    six, rev, three = (ratio(R.six_products(x, y, o)) for o in (R.SMALLEST_FIRST, R.LARGEST_FIRST, R.LEADING_THREE))
    plain = ratio(x * y)
    print(f"max per-product error in U: six smallest first {six.max().item():.3f}, largest first {rev.max().item():.3f}, "
          f"leading three {three.max().item():.1f} ({(three > 2).double().mean().item():.3f} of the pairs above 2 U), plain fp32 {plain.max().item():.3f}")
    assert six.max().item() <= 2.0
    assert plain.max().item() <= 1.0
    assert (three > 2).double().mean().item() > 0.9


# ---- the layout mirrors equal the library's host-side answers ------------------------------------------------------------------

def test_layout_mirrors_equal_the_library():
    from kdrt.lib import lib
    shapes = [(1, 4, 4), (37, 36, 20), (300, 100, 132), (333, 32, 32), (333, 64, 64), (333, 128, 128), (333, 32, 192), (1000, 64, 384),
              (129, 768, 128), (257, 192, 64), (131173, 128, 128), (131000, 128, 128), (43557, 32, 192), (70000, 64, 128), (333, 256, 64)]
    prev_split, prev_stream = lib.kd_set_gemm_split(1), lib.kd_set_gemm_stream(2)
    try:
        for M, K, N in shapes:
            for pro, epis in ((0, (0, 1, 5)), (1, (0, 1, 5)), (2, (0, 2))):
                for epi in epis:
                    for add in (0, 1):
                        for mode, form in ((0, "tiled"), (2, "stream")):
                            lib.kd_set_gemm_stream(mode)
                            want = R.gemm_layout(M, K, N, pro, epi, add, form)["rows"]
                            assert lib.kd_pwconv_stat_rows_for(M, K, N, pro, epi, add) == want, (M, K, N, pro, epi, add, form)
            lib.kd_set_gemm_split(0)
            lib.kd_set_gemm_stream(2)
            assert lib.kd_pwconv_stat_rows_for(M, K, N, 1, 1, 0) == R.tiled_layout(M, N)["rows"]
            lib.kd_set_gemm_split(1)
        for M, N, K in [(17, 384, 64), (777, 192, 32), (777, 768, 128), (777, 64, 192), (777, 64, 384), (777, 128, 384), (777, 128, 768),
                        (777, 128, 128), (777, 128, 64), (777, 64, 128), (777, 128, 256), (777, 256, 256), (777, 64, 256), (129, 768, 768),
                        (37, 20, 36), (100, 32, 32), (40000, 384, 64), (300000, 128, 128)]:
            assert lib.kd_pwconv_wgrad_ws_bytes(M, N, K) == R.wgrad_ws_bytes(M, N, K), (M, N, K)
    finally:
        lib.kd_set_gemm_split(prev_split)
        lib.kd_set_gemm_stream(prev_stream)
