"""The FPN top-down path's fewer-pass forms against the launches they replace, bit for bit (CameraFPNLite.forward,
fusion_module.py:51-64):
  * kd_pwconv_gemm_fpn_sum (inference: the output-size lateral's GEMM adds the resized smaller laterals in its epilogue) against
    kd_pwconv_gemm (raw) followed by kd_bilinear_sum_fwd, refusals, and an eval / no_grad model with the switch off and on;
  * kd_bilinear_sum_fwd's quad body (one 2x2 quad of outputs per thread, a half-size lateral's 3x3 window loaded once)
    against kd_bilinear_accum_fwd applied lateral by lateral, and against the per-pixel body (kd_set_bilinear_2x_mode);
  * kd_bilinear_bwd's 4 x 4 window form for a half-size lateral against the general gather loop;
  * kd_bilinear_bwd2 (two laterals of one geometry, dout read once) against two kd_bilinear_bwd launches, and a train-mode
    student's parameter gradients with the pairing off and on.
Comparisons are torch.equal on int32 views, so NaN payloads and signed zeros count."""
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 3          # NaN rows behind every output


def _lib():
    from kdrt.ops import P, lib, stream
    return lib, P, stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _guarded(rows, C):
    """[rows + GUARD, C] of NaN; the kernel gets the first `rows` rows."""
    return torch.full((rows + GUARD, C), float("nan"), device="cuda")


def _guard_ok(buf, rows):
    return bool(torch.isnan(buf[rows:]).all())


def _lateral(g, B, h, w, C):
    x = torch.randn(B * h * w, C, generator=g)
    x[::7, ::5] = 0.0                              # exact zeros: the ReLU edge and (with a negative scale) -0.0 products
    return x.cuda(), (torch.rand(C, generator=g) - 0.3).cuda(), torch.randn(C, generator=g).cuda()


# (B, C, (Ho, Wo), lateral sizes, activations); the quad body takes: even Ho / Wo, lateral 0 at the output size with an activation, the
# others at exactly half of it.  Everything else must take the per-pixel body and still match.
SUM_CASES = [
    (3, 128, (8, 8), [(8, 8), (4, 4), (4, 4)], [1, 1, 1]),           # the FPN's geometry: quad body, three laterals
    (3, 64, (8, 8), [(8, 8), (4, 4), (4, 4)], [1, 2, 0]),            # 64 channels (4 quads per wave), ReLU6 / no activation below
    (3, 128, (8, 8), [(8, 8), (4, 4)], [1, 1]),                      # quad body, two laterals
    (3, 64, (6, 10), [(6, 10), (3, 5)], [2, 1]),                     # odd half sizes
    (3, 128, (2, 2), [(2, 2), (1, 1), (1, 1)], [1, 1, 1]),           # a one-texel source: every index clamps
    (3, 128, (7, 9), [(7, 9), (4, 5)], [1, 1]),                      # odd sizes: the per-pixel body
    (3, 64, (7, 9), [(7, 9), (4, 5), (4, 5)], [1, 1, 1]),
    (3, 128, (8, 8), [(8, 8), (4, 4), (4, 4)], [0, 1, 1]),           # lateral 0 without activation: the per-pixel body
    (3, 64, (8, 8), [(4, 4), (4, 4)], [1, 1]),                       # no lateral at the output size: the per-pixel body
    (3, 128, (8, 8), [(8, 8), (4, 4), (2, 2)], [1, 1, 1]),           # a quarter-size lateral: the per-pixel body
    (1, 128, (264, 264), [(264, 264), (132, 132), (132, 132)], [1, 1, 1]),   # 17 424 quads > 2048 blocks x 8: the grid-stride loop
]


@pytest.mark.parametrize("B,C,out_hw,geo,acts", SUM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_sum_fwd_equals_accumulate(B, C, out_hw, geo, acts):
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(B * C + out_hw[0] + len(geo))
    Ho, Wo = out_hw
    lats = [_lateral(g, B, h, w, C) for h, w in geo]
    rows = B * Ho * Wo
    ref = torch.empty(rows, C, device="cuda")
    for i, ((x, sc, sh), (h, w)) in enumerate(zip(lats, geo)):
        lib.call("kd_bilinear_accum_fwd", P(x), P(sc), P(sh), acts[i], P(ref), int(i > 0), B, h, w, Ho, Wo, C, stream())
    a = [(P(x), P(sc), P(sh), acts[i], geo[i][0], geo[i][1]) for i, (x, sc, sh) in enumerate(lats)]
    a += [(None, None, None, 0, 0, 0)] * (3 - len(a))
    out = _guarded(rows, C)
    lib.call("kd_bilinear_sum_fwd", *a[0], *a[1], *a[2], P(out), B, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:rows]), _bits(ref))
    assert _guard_ok(out, rows)


def test_sum_fwd_keeps_nonfinite_and_zero_weight_texels():
    """The first output pair of a half-size lateral weighs its second texel with 0: 0 * inf = NaN and a -0.0 term must come
    out as in the per-pixel form, so the quad body may not skip or reorder them."""
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(5)
    B, C, Ho, Wo = 2, 64, 8, 8
    geo = [(8, 8), (4, 4), (4, 4)]
    lats = [_lateral(g, B, h, w, C) for h, w in geo]
    lats[1][0].view(B, 4, 4, C)[:, 1, :, ::3] = float("inf")
    lats[2][0].view(B, 4, 4, C)[:, :, 1, 1::3] = float("-inf")
    acts = [1, 0, 0]
    rows = B * Ho * Wo
    ref = torch.empty(rows, C, device="cuda")
    for i, ((x, sc, sh), (h, w)) in enumerate(zip(lats, geo)):
        lib.call("kd_bilinear_accum_fwd", P(x), P(sc), P(sh), acts[i], P(ref), int(i > 0), B, h, w, Ho, Wo, C, stream())
    a = [(P(x), P(sc), P(sh), acts[i], geo[i][0], geo[i][1]) for i, (x, sc, sh) in enumerate(lats)]
    out = _guarded(rows, C)
    lib.call("kd_bilinear_sum_fwd", *a[0], *a[1], *a[2], P(out), B, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    assert torch.isnan(ref).any() and torch.isfinite(ref).any()
    assert torch.equal(_bits(out[:rows]), _bits(ref))
    assert _guard_ok(out, rows)


# (B, Hi, Wi, Ho, Wo): exactly half the output size (the window form), other ratios and the output size itself (the general loop and
# the identity of the NL = 2 instance); (3, 48, 48, ..): 6912 pixels, several blocks and a partial last one at both widths
BWD2_CASES = [(2, 4, 4, 8, 8), (2, 3, 5, 6, 10), (3, 48, 48, 96, 96), (2, 3, 5, 7, 9), (2, 4, 4, 9, 9), (2, 6, 6, 6, 6)]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo", BWD2_CASES, ids=str)
def test_bilinear_bwd2_equals_two_launches(B, Hi, Wi, Ho, Wo, C):
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(B * Hi * Wi + C + Ho)
    npix = B * Hi * Wi
    rows = lib.kd_rowwise_stat_rows(npix, C)
    dout = torch.randn(B * Ho * Wo, C, generator=g).cuda()
    lat = []
    for act in (1, 2):                             # ReLU and ReLU6: the two masks differ
        x, sc, sh = _lateral(g, B, Hi, Wi, C)
        lat.append((x, sc, sh, act, torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()))
    ref = []
    for x, sc, sh, act, mean, inv in lat:
        gin, part = _guarded(npix, C), _guarded(rows * 2, C)
        lib.call("kd_bilinear_bwd", P(dout), P(x), P(sc), P(sh), act, P(mean), P(inv), P(gin), P(part), B, Hi, Wi, Ho, Wo, C, stream())
        ref.append((gin, part))
    got = [(_guarded(npix, C), _guarded(rows * 2, C)) for _ in lat]
    args = []
    for (x, sc, sh, act, mean, inv), (gin, part) in zip(lat, got):
        args += [P(x), P(sc), P(sh), act, P(mean), P(inv), P(gin), P(part)]
    lib.call("kd_bilinear_bwd2", P(dout), *args, B, Hi, Wi, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    for l in range(2):
        assert not torch.equal(_bits(ref[0][0]), _bits(ref[1][0]))            # the two laterals are different problems
        assert torch.equal(_bits(got[l][0]), _bits(ref[l][0])), f"gin {l}"
        assert torch.equal(_bits(got[l][1]), _bits(ref[l][1])), f"partial {l}"
        assert _guard_ok(got[l][0], npix) and _guard_ok(got[l][1], rows * 2)
        assert not torch.isnan(got[l][1][:rows * 2]).any()


# (B, Hi, Wi, C): exactly-half-size laterals, where kd_bilinear_bwd takes the 4 x 4 window form
WINDOW_CASES = [(2, 1, 1, 64), (2, 1, 4, 128), (3, 2, 2, 64), (2, 4, 4, 128), (2, 3, 5, 64), (3, 48, 48, 128), (1, 136, 136, 128)]


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "plain"])
@pytest.mark.parametrize("B,Hi,Wi,C", WINDOW_CASES, ids=str)
def test_bilinear_bwd_window_form_equals_general_loop(B, Hi, Wi, C, masked):
    """The adjoint of an exactly-half-size lateral: the 4 x 4 window loaded up front (mode 1, the default) against the general
    gather loop (mode 0), bit for bit, on maps whose every pixel is a border pixel (1 x 1, 1 x 4, 2 x 2), odd maps, several
    blocks with a partial last one, and 18 496 pixels (more than the 2048 x 8 a grid covers at once); inf and NaN in dout
    stay where the loop puts them (a skipped zero weight is not a multiplication by zero)."""
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(B * Hi * Wi + C + masked)
    Ho, Wo, npix = 2 * Hi, 2 * Wi, B * Hi * Wi
    rows = lib.kd_rowwise_stat_rows(npix, C)
    dout = torch.randn(B * Ho * Wo, C, generator=g)
    dout[::11, ::3] = float("inf")
    dout[5::13, 1::3] = float("nan")
    dout = dout.cuda()
    x, sc, sh = _lateral(g, B, Hi, Wi, C)
    mean, inv = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    res = []
    prev = lib.kd_set_bilinear_2x_mode(1)
    try:
        for mode in (0, 1):
            lib.kd_set_bilinear_2x_mode(mode)
            gin, part = _guarded(npix, C), _guarded(rows * 2, C)
            if masked:
                lib.call("kd_bilinear_bwd", P(dout), P(x), P(sc), P(sh), 1, P(mean), P(inv), P(gin), P(part), B, Hi, Wi, Ho, Wo, C, stream())
            else:
                lib.call("kd_bilinear_bwd", P(dout), None, None, None, 0, None, None, P(gin), None, B, Hi, Wi, Ho, Wo, C, stream())
            torch.cuda.synchronize()
            res.append((gin, part))
    finally:
        lib.kd_set_bilinear_2x_mode(prev)
    assert prev == 1
    assert torch.isfinite(res[0][0][:npix]).any()
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0]))
    assert torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert _guard_ok(res[1][0], npix) and _guard_ok(res[1][1], rows * 2)


def test_sum_fwd_quad_body_equals_per_pixel_body():
    """kd_bilinear_sum_fwd at the FPN's geometry with the 2x forms on (the quad body) and off (the per-pixel body)."""
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(17)
    B, C, Ho, Wo = 3, 128, 12, 20
    geo = [(12, 20), (6, 10), (6, 10)]
    lats = [_lateral(g, B, h, w, C) for h, w in geo]
    a = [(P(x), P(sc), P(sh), 1, geo[i][0], geo[i][1]) for i, (x, sc, sh) in enumerate(lats)]
    rows = B * Ho * Wo
    outs = []
    prev = lib.kd_set_bilinear_2x_mode(1)
    try:
        for mode in (0, 1):
            lib.kd_set_bilinear_2x_mode(mode)
            out = _guarded(rows, C)
            lib.call("kd_bilinear_sum_fwd", *a[0], *a[1], *a[2], P(out), B, Ho, Wo, C, stream())
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        lib.kd_set_bilinear_2x_mode(prev)
    assert torch.isfinite(outs[0][:rows]).all() and _guard_ok(outs[1], rows)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))


def test_bilinear_bwd2_unmasked_lateral_and_bad_args():
    """One lateral without a mask (no sc: gin is the plain adjoint, its partial is not written), and argument errors launch nothing."""
    from kdrt.lib import KDError
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(9)
    B, Hi, Wi, C = 2, 4, 4, 64
    Ho, Wo, npix = 8, 8, B * Hi * Wi
    rows = lib.kd_rowwise_stat_rows(npix, C)
    dout = torch.randn(B * Ho * Wo, C, generator=g).cuda()
    x, sc, sh = _lateral(g, B, Hi, Wi, C)
    mean, inv = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    r0, rp0, r1 = _guarded(npix, C), _guarded(rows * 2, C), _guarded(npix, C)
    lib.call("kd_bilinear_bwd", P(dout), P(x), P(sc), P(sh), 1, P(mean), P(inv), P(r0), P(rp0), B, Hi, Wi, Ho, Wo, C, stream())
    lib.call("kd_bilinear_bwd", P(dout), None, None, None, 0, None, None, P(r1), None, B, Hi, Wi, Ho, Wo, C, stream())
    g0, p0, g1, p1 = _guarded(npix, C), _guarded(rows * 2, C), _guarded(npix, C), _guarded(rows * 2, C)
    lib.call("kd_bilinear_bwd2", P(dout), P(x), P(sc), P(sh), 1, P(mean), P(inv), P(g0), P(p0),
             None, None, None, 0, None, None, P(g1), P(p1), B, Hi, Wi, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(g0), _bits(r0)) and torch.equal(_bits(p0), _bits(rp0)) and torch.equal(_bits(g1), _bits(r1))
    assert torch.isnan(p1).all()
    bad = _guarded(npix, C)
    with pytest.raises(KDError):                   # the two laterals may not share a gradient buffer
        lib.call("kd_bilinear_bwd2", P(dout), P(x), P(sc), P(sh), 1, P(mean), P(inv), P(bad), P(p0),
                 P(x), P(sc), P(sh), 1, P(mean), P(inv), P(bad), P(p1), B, Hi, Wi, Ho, Wo, C, stream())
    with pytest.raises(KDError):                   # a mask without its input
        lib.call("kd_bilinear_bwd2", P(dout), None, P(sc), P(sh), 1, P(mean), P(inv), P(bad), P(p0),
                 P(x), P(sc), P(sh), 1, P(mean), P(inv), P(g1), P(p1), B, Hi, Wi, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    assert torch.isnan(bad).all()


def test_student_gradients_with_paired_fpn_backward():
    """One KD training step (image 64x64, grid 16x16, B = 2, 512 points; the step installs the gradient sink, so the stage-5
    lateral's gradient is an addend of the stage-4 lateral's data-gradient kernel): every student parameter gradient with the
    stage-4 / stage-5 resize adjoints in one kd_bilinear_bwd2 launch equals, bit for bit, the one with a launch per lateral."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt import units as U
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    B, HW, N, G = 2, 64, 512, 16
    teacher = build_product("concat", G)
    load_random_state(teacher, "concat", 11)
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    cw = torch.tensor([0.4, 3.5]).cuda()
    lib = U.lib
    real_call = lib.call
    prev = U.FPN_BWD_PAIR[0]
    grads, calls = [], []
    try:
        for mode in (0, 1):
            U.FPN_BWD_PAIR[0] = mode
            student = build_product("weighted", G)
            load_random_state(student, "weighted", 12)
            student.train()
            step = KDStep(student, teacher, FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3), cw)
            seen = []
            lib.call = lambda name, *a, _s=seen: (_s.append(name), real_call(name, *a))[1]
            step(images, pts, labels)
            torch.cuda.synchronize()
            del lib.call
            grads.append({k: p.grad.clone() for k, p in student.named_parameters()})
            calls.append(seen)
    finally:
        U.FPN_BWD_PAIR[0] = prev
        lib.__dict__.pop("call", None)
    assert calls[0].count("kd_bilinear_bwd2") == 0 and calls[1].count("kd_bilinear_bwd2") == 1
    assert calls[0].count("kd_bilinear_bwd") - calls[1].count("kd_bilinear_bwd") == 2
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 50
    for k in grads[0]:
        assert torch.equal(_bits(grads[0][k]), _bits(grads[1][k])), k


# ---- the FPN sum written by the output-size lateral's GEMM (inference) ------------------------------------------------------
# (B, (Ho, Wo), smaller laterals): rows B*Ho*Wo = 64, 128, 60, 120, 81, 162 -- whole 32-row slabs and partial last ones; 9 x 9 over 4 x 4
# is a ratio that is not 2 (the epilogue uses the general source index, so it is covered and must match)
GEMM_SUM_CASES = [(1, (8, 8), [(4, 4), (4, 4)]), (2, (8, 8), [(4, 4), (4, 4)]), (1, (8, 8), [(4, 4)]), (2, (8, 8), [(4, 4)]),
                  (1, (6, 10), [(3, 5)]), (2, (6, 10), [(3, 5)]), (1, (9, 9), [(4, 4)]), (2, (9, 9), [(4, 4), (4, 4)]),
                  (3, (40, 40), [(20, 20), (20, 20)])]          # 4800 rows: 150 slabs over several workgroups


def _gemm_sum_inputs(g, B, Ho, Wo, small, K, N):
    M = B * Ho * Wo
    A = torch.randn(M, K, generator=g).cuda()
    W = (torch.randn(N, K, generator=g) / 8).cuda()
    bias = torch.randn(N, generator=g).cuda()
    esc, esh = (torch.rand(N, generator=g) + 0.5).cuda(), torch.randn(N, generator=g).cuda()
    lats = [_lateral(g, B, h, w, N) for h, w in small]
    return A, W, bias, esc, esh, lats


def _gemm_sum_call(lib, P, stream, A, W, bias, esc, esh, act0, lats, small, acts, out, B, Ho, Wo, K, N):
    a = [(P(x), P(sc), P(sh), acts[i], small[i][0], small[i][1]) for i, (x, sc, sh) in enumerate(lats)]
    a += [(None, None, None, 0, 0, 0)] * (2 - len(a))
    lib.call("kd_pwconv_gemm_fpn_sum", P(A), K, P(W), P(bias), P(esc), P(esh), act0, *a[0], *a[1], P(out), B, Ho, Wo, K, N, stream())


@pytest.mark.parametrize("act0", [1, 0], ids=["relu", "none"])
@pytest.mark.parametrize("B,out_hw,small", GEMM_SUM_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_fpn_sum_equals_gemm_then_sum(B, out_hw, small, act0):
    lib, P, stream = _lib()
    K, N = 64, 128
    Ho, Wo = out_hw
    M = B * Ho * Wo
    assert lib.kd_pwconv_gemm_fpn_sum_supported(M, K, N, len(small))
    g = torch.Generator().manual_seed(M + len(small) + act0)
    A, W, bias, esc, esh, lats = _gemm_sum_inputs(g, B, Ho, Wo, small, K, N)
    acts = [1, act0][:len(small)]
    raw = torch.empty(M, N, device="cuda")
    lib.call("kd_pwconv_gemm", P(A), K, None, 0, 0, 0, None, None, None, None, None, P(W), P(bias), P(raw), N, None, 0, 0, None, 0,
             None, None, None, None, 0, None, 0, M, K, N, None, stream())
    a = [(P(raw), P(esc), P(esh), act0, Ho, Wo)] + [(P(x), P(sc), P(sh), acts[i], small[i][0], small[i][1]) for i, (x, sc, sh) in enumerate(lats)]
    a += [(None, None, None, 0, 0, 0)] * (3 - len(a))
    ref = torch.empty(M, N, device="cuda")
    lib.call("kd_bilinear_sum_fwd", *a[0], *a[1], *a[2], P(ref), B, Ho, Wo, N, stream())
    out = _guarded(M, N)
    _gemm_sum_call(lib, P, stream, A, W, bias, esc, esh, act0, lats, small, acts, out, B, Ho, Wo, K, N)
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all()
    assert torch.equal(_bits(out[:M]), _bits(ref))
    assert _guard_ok(out, M)


def test_gemm_fpn_sum_refuses_other_shapes():
    """Shapes without an instance and the exact-fp32 arithmetic raise KDError and launch nothing: the output stays NaN."""
    from kdrt import ops
    from kdrt.lib import KDError
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(1)
    B, Ho, Wo, small = 1, 8, 8, [(4, 4)]
    for K, N in ((32, 128), (64, 64), (128, 128), (64, 256)):
        assert not lib.kd_pwconv_gemm_fpn_sum_supported(B * Ho * Wo, K, N, 1)
        A, W, bias, esc, esh, lats = _gemm_sum_inputs(g, B, Ho, Wo, small, K, N)
        out = _guarded(B * Ho * Wo, N)
        with pytest.raises(KDError):
            _gemm_sum_call(lib, P, stream, A, W, bias, esc, esh, 1, lats, small, [1], out, B, Ho, Wo, K, N)
        torch.cuda.synchronize()
        assert torch.isnan(out).all(), (K, N)
    assert not lib.kd_pwconv_gemm_fpn_sum_supported(64, 64, 128, 0) and not lib.kd_pwconv_gemm_fpn_sum_supported(64, 64, 128, 3)
    K, N = 64, 128
    A, W, bias, esc, esh, lats = _gemm_sum_inputs(g, B, Ho, Wo, small, K, N)
    out = _guarded(B * Ho * Wo, N)
    prev = ops.set_gemm_arithmetic("fp32")
    try:
        assert not lib.kd_pwconv_gemm_fpn_sum_supported(B * Ho * Wo, K, N, 1)
        with pytest.raises(KDError):
            _gemm_sum_call(lib, P, stream, A, W, bias, esc, esh, 1, lats, small, [1], out, B, Ho, Wo, K, N)
    finally:
        ops.set_gemm_arithmetic(prev)
    with pytest.raises(KDError):                   # a smaller lateral without coefficients
        lib.call("kd_pwconv_gemm_fpn_sum", P(A), K, P(W), P(bias), P(esc), P(esh), 1, P(lats[0][0]), None, None, 1, 4, 4,
                 None, None, None, 0, 0, 0, P(out), B, Ho, Wo, K, N, stream())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_teacher_forward_with_sum_in_lateral_gemm():
    """A concat-fusion model in eval() under no_grad (image 64 x 64, grid 16 x 16, B = 2, 512 points): logits and the KD features
    with the output-size lateral's GEMM writing the FPN sum (switch 1) equal, bit for bit, those of the two launches (switch 0)."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt import units as U
    from kdrt.kd import KD_FEATURES
    B, HW, N, G = 2, 64, 512, 16
    model = build_product("concat", G)
    load_random_state(model, "concat", 11)
    model.eval()
    images, pts, _ = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts = images.cuda(), pts.cuda()
    lib = U.lib
    real_call = lib.call
    prev = U.FPN_LATERAL_SUM[0]
    res, calls = [], []
    try:
        for mode in (0, 1):
            U.FPN_LATERAL_SUM[0] = mode
            seen = []
            lib.call = lambda name, *a, _s=seen: (_s.append(name), real_call(name, *a))[1]
            with torch.no_grad():
                z, mids = model(images, pts, return_intermediates=KD_FEATURES)
            torch.cuda.synchronize()
            del lib.call
            res.append({"z": z.clone(), **{k: mids[k].clone() for k in KD_FEATURES}})
            calls.append(seen)
    finally:
        U.FPN_LATERAL_SUM[0] = prev
        lib.__dict__.pop("call", None)
    assert calls[0].count("kd_pwconv_gemm_fpn_sum") == 0 and calls[0].count("kd_bilinear_sum_fwd") == 1
    assert calls[1].count("kd_pwconv_gemm_fpn_sum") == 1 and calls[1].count("kd_bilinear_sum_fwd") == 0
    assert calls[0].count("kd_pwconv_gemm") - calls[1].count("kd_pwconv_gemm") == 1
    for k in res[0]:
        assert torch.isfinite(res[0][k]).all(), k
        assert torch.equal(_bits(res[0][k]), _bits(res[1][k])), k
