"""The float64 references of tests/_fp64_conv_ref.py (the truth of tests/test_gpu_conv_kernels.py) against stock torch in
float64 on the CPU (F.conv2d, F.unfold, autograd through conv2d / batch_norm / ReLU6), the error bound they state met
element by element by a plain fp32 evaluation on every input recipe the GPU file uses, the launch-layout mirrors against the
library's own host-side queries, and -- so that the suite is known to be able to fail -- deliberately wrong evaluations of
each stencil and reduction rejected by the very comparison the GPU tests use."""
import pytest
import torch
import torch.nn.functional as F

import _fp64_conv_ref as R
from test_gpu_tail_kernels import _check

D = torch.float64
CHANNELS = [8, 32, 48, 64, 144, 192, 240, 256, 288, 384, 480, 576, 768, 960, 1024]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _d(*ts):
    return [t.double() if torch.is_tensor(t) else t for t in ts]


def _dw_case(seed, B, H, W, C, stride, act_id):
    g = _g(seed)
    Ho, Wo = R._out_size(H, stride), R._out_size(W, stride)
    x, w = R.rnd(g, B, H, W, C), R.rnd(g, C, 9)
    sc, sh, mean, inv = R.coeffs(g, C, act_id)
    return g, x, w, sc, sh, mean, inv, R.rnd(g, B, Ho, Wo, C), R.rnd(g, B, Ho, Wo, C)


# ---- the references are the operations they claim to be --------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", [(2, 7, 9, 8), (1, 1, 5, 4), (3, 2, 1, 12), (2, 16, 17, 4), (1, 3, 3, 8), (2, 6, 4, 4)])
def test_dw_fwd_is_conv2d(B, H, W, C, stride):
    _, x, w, sc, sh, *_ = _d(*_dw_case(B * H + W, B, H, W, C, stride, 2))
    r = R.dw_fwd(x, sc, sh, 2, w, stride)
    y = F.conv2d(F.relu6(x * sc + sh).permute(0, 3, 1, 2), w.view(C, 1, 3, 3), stride=stride, padding=1, groups=C).permute(0, 2, 3, 1)
    _close(r["y"][0], y)
    _close(r["s1"][0], y.sum((0, 1, 2)))
    _close(r["s2"][0], (y * y).sum((0, 1, 2)))
    _close(R.dw_fwd(x, None, None, 0, w, stride)["y"][0],
           F.conv2d(x.permute(0, 3, 1, 2), w.view(C, 1, 3, 3), stride=stride, padding=1, groups=C).permute(0, 2, 3, 1))


@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", [(2, 7, 9, 8), (1, 1, 5, 4), (3, 2, 1, 12), (2, 16, 17, 4), (2, 6, 4, 4)])
def test_dw_bwd_is_autograd(B, H, W, C, stride, addend):
    _, x, w, sc, sh, mean, inv, Dy, _ = _d(*_dw_case(B * H + W + 1, B, H, W, C, stride, 2))
    x.requires_grad_(); w.requires_grad_()
    add = R.rnd(_g(3), B, H, W, C).double() if addend else None
    a = F.relu6(x * sc + sh)
    y = F.conv2d(a.permute(0, 3, 1, 2), w.view(C, 1, 3, 3), stride=stride, padding=1, groups=C).permute(0, 2, 3, 1)
    loss = (y * Dy).sum() + ((a * add).sum() if addend else 0)            # the addend: a second gradient path into act(x*sc+sh)
    loss.backward()
    r = R.dw_bwd(Dy, None, None, None, None, None, None, 0, x.detach(), sc, sh, 2, mean, inv, w.detach(), stride, addend=add)
    gz = x.grad / sc                         # the kernels return the gradient w.r.t. x*sc+sh: BatchNorm's backward applies sc
    _close(r["gx"][0], gz)
    _close(r["dw"][0], w.grad)
    xh = (x.detach() - mean) * inv
    _close(r["s1"][0], gz.sum((0, 1, 2)))
    _close(r["s2"][0], (gz * xh).sum((0, 1, 2)))


@pytest.mark.parametrize("masked", [True, False])
def test_folded_dyeff_is_batchnorm_backward(masked):
    """dyeff with coefficients computed the way kd_bn_bwd_finalize documents them is autograd through a training-mode
    F.batch_norm (+ ReLU6): the depthwise backward reference stands in for the real BatchNorm."""
    g = _g(5)
    B, H, W, C, eps = 3, 5, 7, 8, 1e-5
    Y = (R.rnd(g, B, H, W, C).double() * 2 + 1).requires_grad_()
    gamma, beta = R.rnd(g, C).double().abs() * 2 + 1.5, R.rnd(g, C).double() + (3.0 if masked else 0.0)
    Dy = R.rnd(g, B, H, W, C).double()
    z = F.batch_norm(Y.permute(0, 3, 1, 2), None, None, gamma, beta, training=True, eps=eps).permute(0, 2, 3, 1)
    ((F.relu6(z) if masked else z) * Dy).sum().backward()
    Yd = Y.detach()
    mean, var = Yd.mean((0, 1, 2)), Yd.var((0, 1, 2), unbiased=False)
    invstd = 1 / torch.sqrt(var + eps)
    dsc, dsh = gamma * invstd, beta - mean * gamma * invstd
    s = R.bn_bwd_reduce(Dy.reshape(-1, C), Yd.reshape(-1, C), dsc, dsh, 2 if masked else 0, mean, invstd)
    n = B * H * W
    c1, c2 = s["s1"][0] / n, s["s2"][0] / n
    al = gamma * invstd
    be, ga = -al * c2 * invstd, al * (c2 * invstd * mean - c1)
    e = R.dyeff(Dy, Yd, al, be, ga, dsc if masked else None, dsh if masked else None, 2 if masked else 0)[0]
    _close(e, Y.grad, 1e-11)
    if masked:
        lo, mid, hi = R.relu6_shares(Yd, dsc, dsh)
        assert min(lo, mid, hi) > 0.01, (lo, mid, hi)


@pytest.mark.parametrize("cin,cout,H,W", [(3, 32, 9, 12), (1, 8, 5, 5), (4, 40, 1, 7), (3, 16, 2, 3)])
def test_stem_is_conv2d_and_im2col_is_unfold(cin, cout, H, W):
    g = _g(cin + cout + H)
    x, w = R.rnd(g, 2, cin, H, W).double(), R.rnd(g, cout, cin, 3, 3).double()
    sc, sh, _, _ = _d(*R.coeffs(g, cout, 2))
    y = F.conv2d(x, w, stride=2, padding=1).permute(0, 2, 3, 1)
    r = R.stem_fwd(x, w)
    _close(r["y"][0], y)
    _close(r["s1"][0], y.sum((0, 1, 2)))
    _close(r["s2"][0], (y * y).sum((0, 1, 2)))
    _close(R.stem_infer(x, w, sc, sh, 2)["y"][0], F.relu6(y * sc + sh))
    Kp = (cin * 9 + 3) // 4 * 4 + 4
    col = R.stem_im2col(x, Kp)
    unf = F.unfold(x, 3, padding=1, stride=2).permute(0, 2, 1).reshape(-1, cin * 9)
    assert torch.equal(col[:, :cin * 9], unf) and bool((col[:, cin * 9:] == 0).all())


def test_bn_rowwise_against_autograd():
    g = _g(9)
    M, C = 61, 12
    x, res, Dy = (R.rnd(g, M, C).double() * 3 for _ in range(3))
    sc, sh, mean, inv = _d(*R.coeffs(g, C, 2))
    rsc, rsh, _, _ = _d(*R.coeffs(g, C, 1))
    _close(R.bn_act_apply(x, sc, sh, 2, res, rsc, rsh, 1)["out"][0], F.relu6(x * sc + sh) + F.relu(res * rsc + rsh))
    _close(R.bn_act_apply(x, sc, sh, 1, res)["out"][0], F.relu(x * sc + sh) + res)
    _close(R.bn_act_apply(x, None, None, 2)["out"][0], F.relu6(x))
    xg = x.clone().requires_grad_()
    (F.relu6(xg * sc + sh) * Dy).sum().backward()
    r = R.bn_bwd_reduce(Dy, x, sc, sh, 2, mean, inv)
    _close(r["s1"][0], (xg.grad / sc).sum(0))
    _close(r["s2"][0], (xg.grad / sc * (x - mean) * inv).sum(0))


# ---- the launch-layout mirrors -----------------------------------------------------------------------------------------

def test_dw_layout_classes():
    """the dw_layout classes the GPU suite is built around (quads, columns per block, idle threads, channel chunks)"""
    want = {48: (12, 21, 1), 144: (36, 7, 1), 240: (60, 4, 1), 288: (72, 3, 1), 480: (120, 2, 1), 576: (144, 1, 1),
            960: (240, 1, 1), 384: (32, 8, 3), 768: (32, 8, 6), 1024: (32, 8, 8), 32: (8, 32, 1), 256: (64, 4, 1)}
    for C, (groups, slots, nchunk) in want.items():
        assert R.dw_layout(10 ** 9, C)[:3] == (groups, slots, nchunk), C
    assert [256 - g * s for g, s, _ in (want[c] for c in (48, 144, 240, 288))] == [4, 4, 16, 40]


def test_dw_layout_mirror_is_the_librarys():
    from kdrt.lib import lib
    for C in CHANNELS:
        for npix in list(R.dw_item_ladder(C).values()) + [1, 7, 256 * 128 * 128, 256 * 32 * 32]:
            rows = R.dw_layout(npix, C)[3]
            assert lib.kd_dwconv_stat_rows(npix, C) == rows == lib.kd_dwconv_bwd_stat_rows(npix, C), (npix, C)
            assert lib.kd_dwconv_bwd_ws_bytes(npix, C) == R.dw_layout(4 * npix, C)[3] * C * 9 * 4
        for W, stride in ((15, 1), (16, 1), (16, 2)):
            assert lib.kd_dwconv3x3_bwd_add_supported(C, W, stride) == int(stride == 1 and R.dw_fused_form(3, C, W, stride) == 1)
    for npix in (1, 255, 256, 257, 1024 * 256, 1024 * 256 + 1, 10 ** 7):
        assert lib.kd_stem_stat_rows(npix) == min(-(-npix // 256), 1024)


# ---- the stated bound is met by a plain fp32 evaluation ----------------------------------------------------------------

def _meets(r64, r32, what):
    for k, (v, err) in r64.items():
        d = (r32[k][0].double() - v).abs()
        assert bool((d <= err).all()), (what, k, (d / err.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("act_id", [None, 0, 1, 2], ids=["plain", "act0", "relu", "relu6"])
@pytest.mark.parametrize("stride", [1, 2])
def test_fp32_dw_meets_the_bound(stride, act_id):
    """every reduction treated as one chain over all pixels (n_part = n_red = pixels)"""
    B, H, W, C = 3, 21, 19, 16
    _, x, w, sc, sh, mean, inv, Dy, Y = _dw_case(40 + stride, B, H, W, C, stride, act_id or 0)
    if act_id is None:
        sc = sh = mean = inv = None
    elif act_id == 2:
        assert min(R.relu6_shares(x, sc, sh)) > 0.01
    n = B * H * W
    a = (x, sc, sh, act_id or 0, w, stride, n)
    _meets(R.dw_fwd(*_d(*a)), R.dw_fwd(*a), "dw_fwd")
    al, be, ga = R.folded(_g(1), C)
    dsc, dsh, _, _ = R.coeffs(_g(2), C, 2)
    add = R.rnd(_g(3), B, H, W, C)
    for fold, ad, Dv in ((0, None, Dy), (1, None, Dy), (2, add if stride == 1 else None, Dy)):
        f = (al, be, ga) if fold else (None, None, None)
        m = (dsc, dsh, 2) if fold == 2 else (None, None, 0)
        b = (Dv, Y, *f, *m, x, sc, sh, act_id or 0, mean, inv, w, stride, ad, n, n)
        _meets(R.dw_bwd(*_d(*b)), R.dw_bwd(*b), f"dw_bwd fold {fold}")


@pytest.mark.parametrize("stride", [1, 2])
def test_fp32_dw_meets_the_bound_on_tail_inputs(stride):
    """the tail-only recipe of the GPU file on a walk of more than one turn, with the chain lengths of the real launch"""
    B, H, W, C, x, w, Dy, names = _tail_case(stride, torch.float32)
    xt = x * R.dw_fwd_tail_mask(B, H, W, C, stride)[..., None]
    a = (xt, None, None, 0, w, stride, R.dw_fwd_chain(B, H, W, C, stride))
    _meets(R.dw_fwd(*_d(*a)), R.dw_fwd(*a), "dw_fwd")
    sc, sh, mean, inv = R.coeffs(_g(1), C, 2)
    _, n_part, n_red = R.dw_bwd_forms(1, B, H, W, C, stride, True, True)
    b = (Dy, None, None, None, None, None, None, 0, x, sc, sh, 2, mean, inv, w, stride, None, n_part, n_red)
    _meets(R.dw_bwd(*_d(*b)), R.dw_bwd(*b), "dw_bwd")


def test_fp32_stem_and_rowwise_meet_the_bound():
    g = _g(23)
    for cin, cout in ((3, 32), (4, 40), (1, 8)):
        x, w = R.rnd(g, 3, cin, 45, 37), R.rnd(g, cout, cin, 3, 3)
        sc, sh, _, _ = R.coeffs(g, cout, 2)
        n = 3 * 23 * 19
        _meets(R.stem_fwd(x.double(), w.double(), n), R.stem_fwd(x, w, n), "stem")
        _meets(R.stem_infer(*_d(x, w, sc, sh), 2), R.stem_infer(x, w, sc, sh, 2), "stem_infer")
    M, C = 3000, 48
    x, res, Dy = R.rnd(g, M, C), R.rnd(g, M, C), R.rnd(g, M, C)
    Dt = Dy * R.row_tail_mask(M, 21, 7)[:, None]
    for a in (0, 1, 2):
        sc, sh, mean, inv = R.coeffs(g, C, a)
        rsc, rsh, _, _ = R.coeffs(g, C, 2)
        for args in ((x, sc, sh, a), (x, sc, sh, a, res), (x, sc, sh, a, res, rsc, rsh, 2), (x, None, None, a)):
            _meets(R.bn_act_apply(*_d(*args)), R.bn_act_apply(*args), "bn_act_apply")
        for Dv in (Dy, Dt):
            _meets(R.bn_bwd_reduce(*_d(Dv, x, sc, sh), a, *_d(mean, inv), M), R.bn_bwd_reduce(Dv, x, sc, sh, a, mean, inv, M), "bn_bwd_reduce")


# ---- the comparison can fail: wrong evaluations of each stencil and reduction are rejected ----------------------------------

def _rejected(what, got, ref):
    with pytest.raises(pytest.fail.Exception, match="outside the bound"):
        _check(what, got, ref)


def _tail_case(stride=1, dtype=D):
    """C = 576: one column per block, 2048 blocks -- 2250 work items are a ragged second turn of the walk; the upstream
    gradient is nonzero only in the tail pixels of the fused column-walk kernel (mode 1)"""
    B, H, W, C = 5, 5, 450 * stride, 576
    g = _g(77)
    Ho, Wo = R._out_size(H, stride), R._out_size(W, stride)
    x, w = R.rnd(g, B, H, W, C).to(dtype), R.rnd(g, C, 9).to(dtype)
    names = R.dw_bwd_forms(1, B, H, W, C, stride, True, True)[0]
    wk = R.dw_walk(R.KERNEL_WALK[names[0]], B, H, W, C, stride)
    assert wk["iters"] == 2 and wk["items"] % wk["per_turn"] != 0 and R.dw_walk("fwd", B, H, W, C, stride)["iters"] == 2
    m = R.dw_bwd_tail_mask(names, B, H, W, C, stride)
    assert 0.02 < m.float().mean().item() < 0.3
    return B, H, W, C, x, w, R.rnd(g, B, Ho, Wo, C).to(dtype) * m[..., None], names


@pytest.mark.parametrize("stride", [1, 2])
def test_a_dropped_last_segment_is_rejected(stride):
    """the last column segment (the last work item of the walk) left out of each reduction, with the tail-only inputs and the
    chain lengths of the real launch"""
    B, H, W, C, x, w, Dy, _ = _tail_case(stride)
    xt = x * R.dw_fwd_tail_mask(B, H, W, C, stride)[..., None]
    assert R.dw_fwd_tail_mask(B, H, W, C, stride).float().mean().item() < 0.3
    n_part = R.dw_fwd_chain(B, H, W, C, stride)
    ref = R.dw_fwd(xt, None, None, 0, w, stride, n_part)
    cut = R.dw_fwd(xt, None, None, 0, w, stride)["y"][0].clone()
    cut[-1, :, -1] = 0
    _check("s1", ref["s1"][0].float(), ref["s1"])                          # (the right value, rounded to fp32, passes)
    _rejected("s1", cut.sum((0, 1, 2)), ref["s1"])
    _rejected("s2", (cut * cut).sum((0, 1, 2)), ref["s2"])
    sc, sh, mean, inv = _d(*R.coeffs(_g(1), C, 2))
    _, n_part, n_red = R.dw_bwd_forms(1, B, H, W, C, stride, True, True)
    args = (None, None, None, None, None, None, 0, x, sc, sh, 2, mean, inv, w, stride)
    ref = R.dw_bwd(Dy, *args, n_part=n_part, n_red=n_red)
    Dc = Dy.clone()
    Dc[-1, :, -1] = 0
    bad = R.dw_bwd(Dc, *args)
    for k in ("s1", "s2", "dw"):
        _check(k, ref[k][0].float(), ref[k])
        _rejected(k, bad[k][0], ref[k])


def test_a_clamped_border_column_is_rejected():
    """the left border column taken from the clamped address (column 0 again) instead of zero"""
    B, H, W, C, x, w, Dy, _ = _tail_case()
    ref = R.dw_fwd(x, None, None, 0, w, 1)
    wide = R.dw_fwd(torch.cat([x[:, :, :1], x], 2), None, None, 0, w, 1)["y"][0][:, :, 1:]
    assert torch.equal(wide[:, :, 1:], ref["y"][0][:, :, 1:])
    _rejected("y", wide, ref["y"])
    refb = R.dw_bwd(Dy, None, None, None, None, None, None, 0, x, None, None, 0, None, None, w, 1)
    wideb = R.dw_bwd(torch.cat([Dy[:, :, :1], Dy], 2), None, None, None, None, None, None, 0, torch.cat([x[:, :, :1], x], 2),
                     None, None, 0, None, None, w, 1)["gx"][0][:, :, 1:]
    _rejected("gx", wideb, refb["gx"])


@pytest.mark.parametrize("stride", [1, 2])
def test_transposed_weight_gradient_taps_are_rejected(stride):
    B, H, W, C, x, w, Dy, _ = _tail_case(stride)
    _, _, n_red = R.dw_bwd_forms(1, B, H, W, C, stride, True, True)
    ref = R.dw_bwd(Dy, None, None, None, None, None, None, 0, x, None, None, 0, None, None, w, stride, n_red=n_red)
    _rejected("dw", ref["dw"][0].view(C, 3, 3).transpose(1, 2).reshape(C, 9), ref["dw"])
    wt = w.view(C, 3, 3).transpose(1, 2).reshape(C, 9)
    _rejected("gx", R.dw_bwd(Dy, None, None, None, None, None, None, 0, x, None, None, 0, None, None, wt, stride)["gx"][0], ref["gx"])


def test_a_slab_row_counted_twice_is_rejected():
    """per-block partial rows as the kernels leave them, the last one added twice"""
    g = _g(31)
    M, C, slots, grid = 5000, 32, 32, 40
    x, Dy = R.rnd(g, M, C).double(), R.rnd(g, M, C).double() * R.row_tail_mask(M, slots, grid)[:, None]
    sc, sh, mean, inv = _d(*R.coeffs(g, C, 2))
    iters = -(-M // (grid * slots))
    ref = R.bn_bwd_reduce(Dy, x, sc, sh, 2, mean, inv, iters + slots)
    last = (torch.arange(M) // slots) % grid == grid - 1
    twice = R.bn_bwd_reduce(Dy * (1 + last[:, None].double()), x, sc, sh, 2, mean, inv)
    for k in ("s1", "s2"):
        _check(k, ref[k][0].float(), ref[k])
        _rejected(k, twice[k][0], ref[k])
    xs = R.rnd(g, 2, 3, 64, 66).double()
    xs[0, :, 2:, :] = 0                                                     # only the first and last pixels contribute
    xs[1, :, :-3, :] = 0
    ws = R.rnd(g, 8, 3, 3, 3).double()
    npix = 2 * 32 * 33
    refs = R.stem_fwd(xs, ws, R.stem_chain(npix, 3))
    y = refs["y"][0].reshape(npix, 8)
    blk = (torch.arange(npix) // 256) == (npix - 1) // 256
    _rejected("stem s1", (y * (1 + blk[:, None].double())).sum(0), refs["s1"])


def test_a_closed_upper_mask_is_rejected():
    """z <= 6 instead of z < 6 on inputs that hold an exact 6.0f after the fma"""
    g = _g(41)
    B, H, W, C = 2, 9, 11, 8
    x, w, Dy = R.rnd(g, B, H, W, C), R.rnd(g, C, 9).double(), R.rnd(g, B, H, W, C).double()
    sc, sh = torch.full((C,), 2.0), torch.full((C,), 1.0)
    at6 = torch.rand(B, H, W, C, generator=g) < 0.05
    x = torch.where(at6, torch.full_like(x, 2.5), x).double()              # 2.5 * 2 + 1 == 6 exactly
    mean, inv = torch.zeros(C, dtype=D), torch.ones(C, dtype=D)
    ref = R.dw_bwd(Dy, None, None, None, None, None, None, 0, x, sc.double(), sh.double(), 2, mean, inv, w, 1, n_part=B * H * W)
    assert bool((ref["gx"][0][at6] == 0).all())
    open_ = R.dw_bwd(Dy, None, None, None, None, None, None, 0, x, None, None, 0, None, None, w, 1)["gx"][0]
    wrong = torch.where(at6, open_, ref["gx"][0])
    _rejected("gx", wrong, ref["gx"])
    _rejected("s1", wrong.sum((0, 1, 2)), ref["s1"])
    r2 = R.bn_bwd_reduce(Dy.reshape(-1, C), x.reshape(-1, C), sc.double(), sh.double(), 2, mean, inv, B * H * W)
    z = x.reshape(-1, C) * 2 + 1
    _rejected("bn s1", (Dy.reshape(-1, C) * ((z > 0) & (z <= 6))).sum(0), r2["s1"])
