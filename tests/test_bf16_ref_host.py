"""tests/_bf16_ref.py checked on the CPU: each float64 reference against stock torch on the same bf16-rounded operands, a plain
fp32 evaluation rounded once against the acceptance rule, the exact-input generators against three summation orders, the
listed wrong evaluations against the rule (each must be rejected on exact inputs at the smallest shape of its family), the
loose-interval cap for every (K, N) of tests/test_gpu_bf16_kernels.py, and the layout mirrors against the issue's figures."""
import pytest
import torch
import torch.nn.functional as F

import _bf16_ref as R


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _gemm_fp32(A, W, bias, esc, esh, act_id, res=None, order="fwd"):
    """plain fp32: products of bf16 operands summed in fp32 in the given order, epilogue in fp32, one rounding"""
    a, wb = A.bfloat16().float(), W.bfloat16().float()
    p = a[:, None, :] * wb[None, :, :]                                   # [M, N, K] exact products
    if order == "rev":
        p = p.flip(2)
    if order == "pair":
        while p.shape[2] > 1:
            if p.shape[2] % 2:
                p = torch.cat([p, torch.zeros_like(p[:, :, :1])], 2)
            p = p[:, :, 0::2] + p[:, :, 1::2]
        acc = p[:, :, 0]
    else:
        acc = torch.zeros(p.shape[:2])
        for k in range(p.shape[2]):
            acc = acc + p[:, :, k]
    z = R.act((acc + bias) * esc + esh, act_id)
    if res is not None:
        z = z + res.float()
    return acc, z.bfloat16()


def _all_in(got, value, err, act_id=R.NONE, res=None):
    ok, lo, hi = R.accept(got, value, err, act_id, res)
    return bool(ok.all())


# ---- the references against stock torch ------------------------------------------------------------------------------------

def test_rne_bf16_rounds_a_float64_once():
    x = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -40, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8 + 2.0 ** -40), 257.0, 258.0],
                     dtype=torch.float64)
    want = torch.tensor([1.0 + 2.0 ** -7, 1.0, 1.0 + 2.0 ** -6, -(1.0 + 2.0 ** -7), 256.0, 258.0], dtype=torch.float64)
    assert torch.equal(R.rne_bf16(x), want)
    assert x[0].float().bfloat16().double() == 1.0                       # what rounding twice would give
    assert torch.equal(R.trunc_bf16(torch.tensor([1.0 + 3 * 2.0 ** -8, -1.0 - 3 * 2.0 ** -8])), torch.tensor([1.0 + 2.0 ** -7, -1.0 - 2.0 ** -7]).double())
    assert R.sig_bits_over_8(torch.tensor([257.0, 256.0, 3.0, 258.5], dtype=torch.float64)) == (0.5, 1)


@pytest.mark.parametrize("K,N", [(32, 32), (40, 24), (128, 64)])
def test_pwconv_reference_against_matmul(K, N):
    A, W, b, sc, sh = R.random_gemm_inputs(_g(K + N), 37, K, N, "cpu")
    z, e = R.pwconv(A, W, b, sc, sh)
    want = (A.double() @ W.bfloat16().double().t() + b.double()) * sc.double() + sh.double()
    assert torch.allclose(z, want, rtol=1e-13, atol=1e-13) and bool((e > 0).all())
    acc32 = A.float() @ W.bfloat16().float().t()
    assert bool((((acc32 + b) * sc + sh).double() - z).abs().le(e).all())


@pytest.mark.parametrize("stride", [1, 2])
def test_conv_references_against_conv2d(stride):
    g = _g(stride)
    x = torch.randn(2, 7, 5, 16, generator=g).bfloat16()
    w, sc, sh = torch.randn(16, 1, 3, 3, generator=g), torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g)
    z, e = R.dwconv(x, w, sc, sh, stride)
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride, padding=1, groups=16).permute(0, 2, 3, 1) * sc.double() + sh.double()
    assert z.shape == want.shape and torch.allclose(z, want, rtol=1e-13, atol=1e-13)
    xs, ws = torch.randn(2, 3, 9, 6, generator=g), torch.randn(8, 3, 3, 3, generator=g)
    z, e = R.stem(xs, ws, sc[:8], sh[:8])
    want = F.conv2d(xs.double(), ws.double(), stride=2, padding=1).permute(0, 2, 3, 1) * sc[:8].double() + sh[:8].double()
    assert z.shape == want.shape and torch.allclose(z, want, rtol=1e-13, atol=1e-13)
    z32 = F.conv2d(xs, ws, stride=2, padding=1).permute(0, 2, 3, 1) * sc[:8] + sh[:8]
    assert _all_in(z32.clamp(0, 6).bfloat16(), z, e, R.RELU6)


@pytest.mark.parametrize("Hi,Wi,Ho,Wo", [(8, 6, 8, 6), (8, 6, 16, 12), (4, 3, 16, 12), (45, 9, 64, 7), (64, 5, 45, 5), (7, 7, 64, 3), (1, 1, 5, 5), (5, 5, 1, 1)])
def test_bilinear_reference_against_interpolate(Hi, Wi, Ho, Wo):
    g = _g(Hi + Ho)
    xs = [torch.randn(2, Hi, Wi, 8, generator=g).bfloat16(), torch.randn(2, Hi, Wi, 8, generator=g).bfloat16()]
    z, e = R.bilinear_sum(xs, Ho, Wo)
    want = sum(F.interpolate(x.double().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for x in xs)
    assert torch.allclose(z, want, rtol=0, atol=2e-5)                    # fp32 source coordinates against aten's float64 ones
    z32 = sum(F.interpolate(x.float().permute(0, 3, 1, 2), size=(Ho, Wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1) for x in xs)
    if Ho % Hi == 0 and Wo % Wi == 0:                                    # dyadic weights: aten's fp32 coefficients are the kernel's
        assert _all_in(z32.bfloat16(), z, e)
    # every ratio: a plain fp32 evaluation with the kernel's own fp32 coefficients, rounded once
    mh, mw = R.bilinear_matrix(Hi, Ho, dtype=torch.float32), R.bilinear_matrix(Wi, Wo, dtype=torch.float32)
    k32 = sum(torch.einsum("pw,bowc->bopc", mw, torch.einsum("oh,bhwc->bowc", mh, x.float())) for x in xs)
    assert _all_in(k32.bfloat16(), z, e)


def test_cls_and_weighted_tail_references_against_torch():
    g = _g(5)
    x, w, b = torch.randn(24, 32, generator=g).bfloat16(), torch.randn(3, 32, generator=g), torch.randn(3, generator=g)
    z, e = R.cls_conv(x, w, b, 2)
    want = (x.double() @ w.double().t() + b.double()).reshape(2, 12, 3).permute(0, 2, 1)
    assert torch.equal(z, want)
    assert bool(((x.float() @ w.t() + b).reshape(2, 12, 3).permute(0, 2, 1).double() - z).abs().le(e).all())
    C = 64
    h, cat = torch.randn(19, C, generator=g).relu().bfloat16(), torch.randn(19, 2 * C, generator=g).relu().bfloat16()
    w2, b2 = torch.randn(2, C, generator=g) * 0.3, torch.randn(2, generator=g) * 0.1
    z, e = R.weighted_tail(h, cat, w2, b2)
    sm = torch.softmax(h.double() @ w2.double().t() + b2.double(), 1)
    assert torch.allclose(z, cat[:, :C].double() * sm[:, :1] + cat[:, C:].double() * sm[:, 1:], rtol=1e-13, atol=1e-13)
    sm32 = torch.softmax(h.float() @ w2.t() + b2, 1)
    assert _all_in((cat[:, :C].float() * sm32[:, :1] + cat[:, C:].float() * sm32[:, 1:]).bfloat16(), z, e)


def test_scatter_max_and_lidar_references():
    g = _g(9)
    P, ncells = 300, 400
    cell = R.cell_pattern(P, ncells, n_skip=9)
    assert bool((cell[:-9][1:] >= cell[:-9][:-1]).all()) and bool((cell[-9:] < 0).all()) and int(cell.max()) < ncells
    v = torch.rand(P, 8, generator=g).double()
    val, err = R.scatter_max(v, v * 1e-3, cell, ncells)
    for c in (0, int(cell[50]), int(cell[-10])):
        assert torch.equal(val[c], v[cell == c].max(0).values) and torch.equal(err[c], (v * 1e-3)[cell == c].max(0).values)
    empty = torch.ones(ncells, dtype=torch.bool)
    empty[cell[cell >= 0].long()] = False
    assert bool(empty.any()) and bool((val[empty] == 0).all()) and bool((err[empty] == 0).all())
    l0, l1, l2, pts = R.lidar_params(g, P, exact=False)
    val, err = R.lidar_encoder(pts, cell, ncells, l0, l1, l2)
    # two plain fp32 launches in torch: the layer-1 activation rounded to bf16 in between
    a0 = R.layer0(pts, *l0, R.RELU)
    _, a1 = _gemm_fp32(a0, *l1, R.RELU)
    acc, _ = _gemm_fp32(a1, *l2, R.RELU)
    v2 = R.act((acc + l2[1]) * l2[2] + l2[3], R.RELU).double()
    got, _ = R.scatter_max(v2, None, cell, ncells)
    assert bool(((got - val).abs() <= err).all()) and bool((val > 0).any())
    full = R.lidar_encoder_fp32(pts, cell, ncells, l0, l1, l2)
    assert (full - val).abs().max() <= 0.05 * full.abs().max()            # the bf16 roundings: percent level


def test_exact_lidar_inputs_are_exact():
    g = _g(11)
    l0, l1, l2, pts = R.lidar_params(g, 200, exact=True)
    a0 = R.layer0(pts, *l0, R.RELU)
    assert torch.equal(a0.double(), R.act(pts.double() @ l0[0].double().t() + l0[1].double() + l0[3].double(), R.RELU))    # no rounding at layer 0
    accs = [_gemm_fp32(a0, *l1, R.RELU, order=o) for o in ("fwd", "rev", "pair")]
    assert torch.equal(accs[0][0], accs[1][0]) and torch.equal(accs[0][0], accs[2][0])
    share, _ = R.sig_bits_over_8(accs[0][0].double().clamp_min(0))
    assert share > 0.1                                                   # layer 1's rounding to bf16 is a real one
    acc2 = [_gemm_fp32(accs[0][1], *l2, R.RELU, order=o)[0] for o in ("fwd", "rev", "pair")]
    assert torch.equal(acc2[0], acc2[1]) and torch.equal(acc2[0], acc2[2])
    R.assert_exact(accs[0][1].double().abs() @ l2[0].double().abs().t() + 8, 1.0)
    cell = R.cell_pattern(200, 300, 5)
    val, err = R.lidar_encoder(pts, cell, 300, l0, l1, l2, exact=True)
    assert float(err.max()) == 0 and bool((val.float().double() == val).all()) and bool((val > 0).any())


# ---- a plain fp32 evaluation passes; the exact inputs are exact; wrong evaluations are rejected --------------------------------

@pytest.mark.parametrize("K,N", [(8, 8), (40, 24), (32, 32), (128, 64)])
@pytest.mark.parametrize("res", [False, True])
def test_gemm_rule_exact_inputs_and_rejections(K, N, res):
    g = _g(K * 7 + N + res)
    M = 34
    act_id = R.RELU6 if K == 32 else R.RELU
    Rs = R.exact_acts(g, (M, N), 8) if res else None
    # random inputs: forward-order fp32 passes
    A, W, b, sc, sh = R.random_gemm_inputs(g, M, K, N, "cpu")
    Rr = torch.randn(M, N, generator=g).bfloat16() if res else None
    z, e = R.pwconv(A, W, b, sc, sh, Rr)
    for order in ("fwd", "rev", "pair"):
        assert _all_in(_gemm_fp32(A, W, b, sc, sh, act_id, Rr, order)[1], z, e, act_id, Rr), order
    # exact inputs: three orders, one fp32 value; the rule collapses to equality
    A, W, b, sc, sh = R.exact_gemm_inputs(g, M, K, N, "cpu", relu6=act_id == R.RELU6)
    z, e = R.pwconv(A, W, b, sc, sh, Rs)
    R.assert_exact(e / (R.C_BOUND * (K + 2 + res) * R.U), 2.0 ** -3 * sc.double(), "gemm")        # units: 2^-3 (weights) * the column's scale
    outs = [_gemm_fp32(A, W, b, sc, sh, act_id, Rs, o) for o in ("fwd", "rev", "pair")]
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:])
    zero = torch.zeros_like(e)
    lo, hi = R.interval(z, zero, act_id, Rs)
    assert torch.equal(lo, hi) and torch.equal(outs[0][1].double(), lo) and R.loose_share(lo, hi) == 0
    share, ties = R.sig_bits_over_8(R.act(z, act_id) + (0 if Rs is None else Rs.double()))
    print(f"exact GEMM K={K} N={N} res={res}: {share:.1%} of the outputs need more than 8 bits, {ties} ties")
    assert share > 0.1 and ties > 0
    want = lo

    def rejected(got):
        return not bool(R.accept(got, z, zero, act_id, Rs)[0].all())

    a, wb = A.double(), W.bfloat16().double()
    epi = lambda acc: R.act((acc + b.double()) * sc.double() + sh.double(), act_id) + (0 if Rs is None else Rs.double())
    assert rejected(R.trunc_bf16(epi(a @ wb.t()))), "truncation instead of round-to-nearest-even"
    assert rejected(R.rne_bf16(epi(a[:, :K - 8] @ wb[:, :K - 8].t()))), "a dropped last K fragment"
    pair = want.clone(); pair[:, N - 2:] = float("nan")
    assert rejected(pair), "a dropped last column pair (never written)"
    pair = want.clone(); pair[:, N - 2:] = want[:, N - 4:N - 2]
    assert rejected(pair), "the last column pair taken from its neighbour"
    rep = a.clone(); rep[M - 2] = rep[M - 1]
    assert rejected(R.rne_bf16(epi(rep @ wb.t()))), "row M - 1 copied into row M - 2 (the reference has no row M: this stands in for 'the row after M repeated into row M - 1')"
    if res:
        late = R.rne_bf16(R.rne_bf16(R.act((a @ wb.t() + b.double()) * sc.double() + sh.double(), act_id)) + Rs.double())
        assert rejected(late), "the residual added after the rounding"


@pytest.mark.parametrize("stride,H,W", [(1, 3, 3), (2, 5, 5), (1, 16, 2)])
def test_depthwise_rule_exact_inputs_and_halo_rejections(stride, H, W):
    g = _g(stride + H)
    C = 8
    x = R.exact_acts(g, (2, H, W, C), 100)
    w = R.exact_weights(g, C, 9, emin=-2).reshape(C, 1, 3, 3)
    sc, sh = R.exact_affine(g, C, -4, -1)
    z, e = R.dwconv(x, w, sc, sh, stride)
    R.assert_exact(e / (R.C_BOUND * 10 * R.U), 2.0 ** -6, "dw")
    lo, hi = R.interval(z, torch.zeros_like(e), R.RELU)
    assert torch.equal(lo, hi)
    ref32 = F.conv2d(x.float().permute(0, 3, 1, 2), w, stride=stride, padding=1, groups=C).permute(0, 2, 3, 1) * sc + sh
    assert torch.equal(ref32.relu().bfloat16().double(), lo)
    share, _ = R.sig_bits_over_8(R.act(z, R.RELU))
    assert share > 0.1
    for pad in ((0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0)):      # top, bottom, left, right halo clamped
        xr = F.pad(x.double().permute(0, 3, 1, 2), pad[2:], mode="replicate")
        xr = F.pad(xr, (1 - pad[2], 1 - pad[3], 1 - pad[4], 1 - pad[5]))
        wrong = F.conv2d(xr, w.double(), stride=stride, groups=C).permute(0, 2, 3, 1) * sc.double() + sh.double()
        assert wrong.shape == z.shape
        assert not bool(R.accept(R.rne_bf16(R.act(wrong, R.RELU)), z, torch.zeros_like(e), R.RELU)[0].all()), f"clamped halo {pad} accepted"
    # random inputs: fp32 conv2d passes the rule
    x = torch.randn(2, H, W, C, generator=g).bfloat16()
    w, sc, sh = torch.randn(C, 1, 3, 3, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    z, e = R.dwconv(x, w, sc, sh, stride)
    r32 = F.conv2d(x.float().permute(0, 3, 1, 2), w, stride=stride, padding=1, groups=C).permute(0, 2, 3, 1) * sc + sh
    assert _all_in(r32.clamp(0, 6).bfloat16(), z, e, R.RELU6)


def test_stem_cls_bilinear_exact_inputs():
    g = _g(21)
    x = R._ints(g, (2, 3, 5, 7), -1000, 1000, "cpu").float()
    w = (R._ints(g, (8, 3, 3, 3), -8, 8, "cpu") / 8).float()
    sc, sh = R.exact_affine(g, 8, -9, -6)
    z, e = R.stem(x, w, sc, sh)
    R.assert_exact(e / (R.C_BOUND * 28 * R.U), 2.0 ** -12, "stem")
    r32 = F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1) * sc + sh
    assert torch.equal(r32.double(), z) and R.sig_bits_over_8(R.act(z, R.RELU))[0] > 0.1
    xc, wc, bc = R.exact_acts(g, (30, 8), 100), R.exact_weights(g, 3, 8), R.exact_bias(g, 3)
    zc, ec = R.cls_conv(xc, wc, bc, 2)
    assert torch.equal((xc.float() @ wc.t() + bc).reshape(2, 15, 3).permute(0, 2, 1).double(), zc)
    for f in (1, 2, 4):
        xs = [R.exact_acts(g, (2, 3, 5, 8), 100) for _ in range(3)]
        zb, eb = R.bilinear_sum(xs, 3 * f, 5 * f)
        assert bool(((zb * 64) == (zb * 64).round()).all()) and float(zb.abs().max()) < 2 ** 10      # multiples of 2^-6 below 2^10: fp32-exact
        assert R.sig_bits_over_8(zb)[0] > (0.1 if f > 1 else 0.0)


# ---- the loose-interval cap, for every (K, N) the GPU file uses ----------------------------------------------------------------

@pytest.mark.parametrize("K,N", R.all_kn(), ids=lambda v: str(v))
def test_loose_interval_cap(K, N):
    g = _g(K + N)
    A, W, b, sc, sh = R.random_gemm_inputs(g, 192, K, N, "cpu")
    for res in (None, torch.randn(192, N, generator=g).bfloat16()):
        z, e = R.pwconv(A, W, b, sc, sh, res)
        for act_id in (R.RELU, R.RELU6):
            lo, hi = R.interval(z, e, act_id, res)
            share = R.loose_share(lo, hi)
            inside = ((z > 0) & (z < 6)).double().mean().item()
            print(f"K={K} N={N} res={res is not None} act={act_id}: {share:.2%} loose intervals, {inside:.0%} of the outputs inside (0, 6)")
            assert share <= R.LOOSE_CAP and inside > 0.3
            assert float(((hi - lo) / R.rne_bf16(z.abs() + 1e-3)).max()) < 2.0 ** -5      # never more than three neighbouring values


# ---- layout mirrors: the figures the issue states ------------------------------------------------------------------------------

def test_layout_mirrors():
    wk = R.gemm_v2_layout(10752 + 1, 128, 768)
    assert (wk["NB"], wk["ntiles"], wk["grid"], wk["per_turn"] * wk["unit"], wk["iters"]) == (4, 6, 42, 10752, 2)
    assert R.gemm_v2_layout(65536, 128, 32)["iters"] == 1 and R.gemm_v2_layout(65537, 128, 32)["iters"] == 2
    wk = R.gemm_v2_layout(21504 + 1, 32, 384, res=True)
    assert (wk["NB"], wk["SL"], wk["unit"], wk["iters"]) == (1, 4, 128, 2)
    assert R.gemm_v2_layout(100, 64, 768, res=True)["NB"] == 2 and R.gemm_v2_layout(100, 64, 768)["NB"] == 4
    assert R.gemm_v2_layout(100, 768, 768)["NB"] == 2 and R.gemm_v2_layout(100, 512, 768)["NB"] == 2 and R.gemm_v2_layout(100, 384, 768)["NB"] == 4
    assert {(res, R.gemm_v2_layout(100, K, N, res)["NB"]) for K, N, res in R.V2_CASES} == {(r, nb) for r in (False, True) for nb in (4, 2, 1)}
    assert {R.gemm_v2_layout(100, K, N)["unit"] for K, N, _ in R.V2_CASES} == {128, 64, 32} and {K for K, _, _ in R.V2_CASES} == set(R.V2_K)
    assert all(R.gemm_v2_layout(M, K, N, res)["iters"] == 1 for M, K, N, res in R.SMALL_CASES)
    assert R.gemm_v2_layout(300, 256, 128, True)["NB"] == 4 and R.gemm_v2_layout(129, 192, 64, True)["NB"] == 2
    assert R.gemm_v2_layout(100, 96, 64) is None and R.gemm_v2_layout(100, 64, 64, m_dev=True) is None and R.gemm_v2_layout(100, 64, 64, ldc=68) is None
    assert [R.gemm_v1_layout(100, k, n)["NB"] for k, n in ((64, 768), (64, 704), (64, 736), (512, 768), (40, 128))] == [4, 2, 1, 2, 1]
    assert R.gemm_v1_layout(100, 40, 128)["tail"] and R.gemm_v1_layout(10 ** 6, 64, 736)["grid"] == 11
    for K, N, res in R.V2_CASES:
        wk = R.gemm_v2_layout(10 ** 6, K, N, res)
        for name, rows in R.gemm_ladder(wk["unit"], wk["grid"]).items():
            R.on_ladder(name, R.gemm_v2_layout(rows, K, N, res))
    for K, N, _ in R.V1_CASES:
        wk = R.gemm_v1_layout(10 ** 6, K, N)
        for name, rows in R.gemm_ladder(32, wk["grid"]).items():
            R.on_ladder(name, R.gemm_v1_layout(rows, K, N))
    assert R.cg8_layout(4097, 1024) == (128, 2, 2048) and R.cg8_layout(5, 8) == (1, 256, 1) and R.cg8_layout(10, 2048) == (256, 1, 10)
    assert R.dw_layout(2, 32, 5, 8, 1)["kernel"] == "dw_bf16_s1_pipe_kernel<16>" and R.dw_layout(2, 32, 5, 8, 1)["nseg"] == 2
    assert R.dw_layout(2, 24, 5, 8, 1)["kernel"] == "dw_bf16_s1_pipe_kernel<8>" and R.dw_layout(2, 24, 5, 8, 1)["nseg"] == 3
    assert R.dw_layout(2, 17, 5, 8, 1)["kernel"] == "dw_bf16_kernel<1>" and R.dw_layout(2, 32, 5, 8, 2)["kernel"] == "dw_bf16_kernel<2>"
    assert R.dw_layout(1, 16, 4097, 1024, 1)["iters"] == 2
    assert R.lidar_layout(65536)["iters"] == 1 and R.lidar_layout(65537)["iters"] == 2
    assert R.pixel_layout("k", 4096 * 256 + 1)["iters"] == 2 and R.weighted_tail_layout(16385, 512)["iters"] == 2
    assert R.bilinear_layout(1, 1, 2049, 2048)["iters"] == 2
