"""The float64 references of tests/_fp64_tail_ref.py (the truth of tests/test_gpu_tail_kernels.py) against stock
torch.nn.functional in float64 on the CPU, and the error bound they state met by a plain fp32 evaluation."""
import pytest
import torch
import torch.nn.functional as F

import _fp64_tail_ref as R

D = torch.float64
RESIZE_PAIRS = [(16, 64), (64, 45), (45, 64), (64, 16), (7, 64), (1, 5), (5, 1), (32, 64), (64, 64)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rnd(g, *s, dtype=D):
    return torch.randn(*s, generator=g, dtype=dtype)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


@pytest.mark.parametrize("hi,ho", RESIZE_PAIRS)
def test_bilinear_matrix_is_interpolate(hi, ho):
    """float64 coordinates: exactly aten's float64 path; fp32 coordinates (the kernel's): within a few fp32 ulps of the
    source coordinate of it, so the two weight matrices differ by O(2^-24 * size)."""
    g = _g(hi * 100 + ho)
    wi, wo = max(1, hi // 2 + 3), max(1, ho - 2)
    x = _rnd(g, 2, hi, wi, 3)
    want = F.interpolate(x.permute(0, 3, 1, 2), size=(ho, wo), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    got = R.bilinear_sum_fwd([(x, None, None, 0)], ho, wo)["out"][0]
    mh, mw = R.bilinear_matrix(hi, ho, D), R.bilinear_matrix(wi, wo, D)
    _close(torch.einsum("oh,bhwc,pw->bopc", mh, x, mw), want)
    m32 = R.bilinear_matrix(hi, ho)
    assert (m32 - mh).abs().max().item() <= 4 * R.U * max(hi, ho)
    assert torch.allclose(m32.sum(1), torch.ones(ho, dtype=D), atol=2 * R.U, rtol=0)
    assert (got - want).abs().max().item() <= 16 * R.U * max(hi, ho, wi, wo) * x.abs().max().item()


@pytest.mark.parametrize("hi,ho", RESIZE_PAIRS)
def test_bilinear_adjoint_is_autograd(hi, ho):
    g = _g(7 * hi + ho)
    wi, wo = max(1, hi - 2), max(1, ho // 3 + 1)
    x = _rnd(g, 2, hi, wi, 4).requires_grad_()
    sc, sh = _rnd(g, 4).abs() + 0.5, _rnd(g, 4) * 0.3
    mean, inv = _rnd(g, 4) * 0.1, _rnd(g, 4).abs() + 0.5
    dout = _rnd(g, 2, ho, wo, 4)
    y = R.bilinear_sum_fwd([(x, sc, sh, R.RELU)], ho, wo)["out"][0]
    (y * dout).sum().backward()
    r = R.bilinear_bwd(dout, hi, wi, x.detach(), sc, sh, R.RELU, mean, inv)
    gz = x.grad / sc                       # the kernels return the gradient w.r.t. x*sc+sh: BatchNorm's backward applies sc
    _close(r["gin"][0], gz)
    xh = (x.detach() - mean) * inv
    _close(r["s1"][0], gz.sum((0, 1, 2)))
    _close(r["s2"][0], (gz * xh).sum((0, 1, 2)))


def test_weighted_fuse_against_autograd():
    g = _g(3)
    M, C = 37, 32
    cat, hraw = _rnd(g, M, 2 * C).requires_grad_(), _rnd(g, M, C).requires_grad_()
    sc, sh = _rnd(g, 2 * C).abs() + 0.5, _rnd(g, 2 * C) * 0.2
    w2, b2 = (_rnd(g, 2, C) * 0.3).requires_grad_(), (_rnd(g, 2) * 0.1).requires_grad_()
    r = R.weighted_fuse_fwd(cat, sc, sh, hraw, w2, b2)
    # the module as written: ReLU -> 1x1 conv -> softmax over the 2 logits -> weighted sum
    a = F.conv2d(F.relu(hraw).t().reshape(1, C, M, 1), w2.reshape(2, C, 1, 1), b2).reshape(2, M).t()
    wts = torch.softmax(a, 1)
    z = F.relu(cat * sc + sh)
    out = z[:, :C] * wts[:, :1] + z[:, C:] * wts[:, 1:]
    _close(r["wts"][0], wts)
    _close(r["out"][0], out)
    dout = _rnd(g, M, C)
    (out * dout).sum().backward()
    b = R.weighted_fuse_bwd(dout, cat.detach(), sc, sh, hraw.detach(), w2.detach(), wts.detach(), n_red=M)
    # dcat is the gradient w.r.t. the ACTIVATED concat (the BN+ReLU mask is applied by the consumer)
    dz = torch.autograd.grad((torch.cat([z[:, :C] * wts.detach()[:, :1], z[:, C:] * wts.detach()[:, 1:]], 1) * torch.cat([dout, dout], 1)).sum(), z)[0]
    _close(b["dcat"][0], dz)
    _close(b["gh"][0], hraw.grad)
    _close(b["dw2"][0], w2.grad)
    _close(b["db1"][0], hraw.grad.sum(0))
    _close(b["db2"][0], b2.grad)


@pytest.mark.parametrize("cin,nc", [(4, 1), (32, 2), (64, 4), (12, 3)])
def test_cls_conv_against_conv2d(cin, nc):
    g = _g(cin * 10 + nc)
    B, H, W = 2, 5, 7
    x = _rnd(g, B * H * W, cin).requires_grad_()
    sc, sh = _rnd(g, cin).abs() + 0.5, _rnd(g, cin) * 0.2
    mean, inv = _rnd(g, cin) * 0.1, _rnd(g, cin).abs() + 0.5
    w, b = _rnd(g, nc, cin).requires_grad_(), _rnd(g, nc).requires_grad_()
    xa = F.relu(x * sc + sh).reshape(B, H, W, cin).permute(0, 3, 1, 2)
    want = F.conv2d(xa, w.reshape(nc, cin, 1, 1), b)
    _close(R.cls_conv_fwd(x.detach(), sc, sh, R.RELU, w.detach(), b.detach(), B)["logits"][0], want.reshape(B, nc, H * W))
    dlog = _rnd(g, B, nc, H * W)
    (want * dlog.reshape(B, nc, H, W)).sum().backward()
    r = R.cls_conv_bwd(dlog, x.detach(), sc, sh, R.RELU, mean, inv, w.detach(), 1, 1)
    gz = x.grad / sc
    _close(r["gx"][0], gz)
    _close(r["dw"][0], w.grad)
    _close(r["db"][0], b.grad)
    xh = (x.detach() - mean) * inv
    _close(r["s1"][0], gz.sum(0))
    _close(r["s2"][0], (gz * xh).sum(0))


@pytest.mark.parametrize("cin,nc,hw", [(4, 1, (1, 1)), (16, 2, (6, 9)), (32, 4, (9, 4)), (12, 3, (1, 7))])
def test_cls3x3_against_conv2d(cin, nc, hw):
    g = _g(cin + nc)
    B, (H, W) = 2, hw
    x = _rnd(g, B, H, W, cin).requires_grad_()
    sc, sh = _rnd(g, cin).abs() + 0.5, _rnd(g, cin) * 0.2
    mean, inv = _rnd(g, cin) * 0.1, _rnd(g, cin).abs() + 0.5
    w, b = _rnd(g, nc, cin, 3, 3).requires_grad_(), _rnd(g, nc).requires_grad_()
    want = F.conv2d(F.relu(x * sc + sh).permute(0, 3, 1, 2), w, b, padding=1)
    _close(R.cls3x3_fwd(x.detach(), sc, sh, R.RELU, w.detach(), b.detach())["logits"][0], want)
    dlog = _rnd(g, B, nc, H, W)
    (want * dlog).sum().backward()
    r = R.cls3x3_bwd(dlog, x.detach(), sc, sh, R.RELU, mean, inv, w.detach(), 1, 1)
    gz = x.grad / sc
    _close(r["gx"][0], gz)
    _close(r["dw"][0], w.grad)
    _close(r["db"][0], b.grad)
    xh = (x.detach() - mean) * inv
    _close(r["s1"][0], gz.sum((0, 1, 2)))
    _close(r["s2"][0], (gz * xh).sum((0, 1, 2)))


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
def test_col2im_im2col_against_conv_transpose2d(hw):
    g = _g(hw[0] * 31 + hw[1])
    B, (H, W), Cin, Cout = 2, hw, 6, 8
    x = _rnd(g, B, Cin, H, W)
    wt = _rnd(g, Cin, Cout, 4, 4).requires_grad_()
    xr = x.permute(0, 2, 3, 1).reshape(-1, Cin)
    col = xr @ wt.detach().reshape(Cin, Cout * 16)                    # the GEMM half (kd_pwconv_gemm)
    r = R.col2im_fwd(col, B, H, W, Cout, 1)
    y = F.conv_transpose2d(x, wt, stride=2, padding=1)
    _close(r["out"][0], y.permute(0, 2, 3, 1))
    _close(r["s1"][0], y.sum((0, 2, 3)))
    _close(r["s2"][0], (y * y).sum((0, 2, 3)))
    D, Y = _rnd(g, B, 2 * H, 2 * W, Cout), _rnd(g, B, 2 * H, 2 * W, Cout)
    al, be, ga, msc, msh = _rnd(g, Cout), _rnd(g, Cout) * 0.1, _rnd(g, Cout) * 0.1, _rnd(g, Cout).abs() + 0.5, _rnd(g, Cout) * 0.2
    dcol = R.im2col_bwd(D, Y, al, be, ga, msc, msh, R.RELU, H, W)["dcol"][0]
    dy = (al * D * (Y * msc + msh > 0) + be * Y + ga).permute(0, 3, 1, 2)
    (y * dy).sum().backward()
    _close(xr.t() @ dcol, wt.grad.reshape(Cin, Cout * 16))           # the wgrad GEMM on dcol is the ConvT weight gradient


def test_fp32_evaluation_meets_the_stated_bound():
    """C_BOUND is not fitted to the kernels: the same formulas evaluated in plain fp32 stay within the bound of every output
    they produce (each reduction treated as one chain over all rows, n_seq = rows)."""
    g = _g(17)
    f = torch.float32

    def check(r64, r32, what):
        for k, (v, err) in r64.items():
            d = (r32[k][0].double() - v).abs()
            assert bool((d <= err).all()), (what, k, (d / err.clamp_min(1e-300)).max().item())

    B, H, W, C = 2, 9, 13, 8
    x, sc, sh = _rnd(g, B, H, W, C, dtype=f), _rnd(g, C, dtype=f).abs() + 0.5, _rnd(g, C, dtype=f) * 0.2
    lat = lambda t: [(t, sc, sh, R.RELU), (t[:, :5, :7].contiguous(), sc, sh, R.RELU)]
    check(R.bilinear_sum_fwd([(a.double(), b.double(), c.double(), d) for a, b, c, d in lat(x)], 23, 11),
          R.bilinear_sum_fwd(lat(x), 23, 11), "resize")
    dout, mean, inv = _rnd(g, B, 23, 11, C, dtype=f), _rnd(g, C, dtype=f) * 0.1, _rnd(g, C, dtype=f).abs() + 0.5
    args = (dout, H, W, x, sc, sh, R.RELU, mean, inv)
    n = B * H * W
    check(R.bilinear_bwd(*[a.double() if torch.is_tensor(a) else a for a in args], n_part=n), R.bilinear_bwd(*args), "resize^T")
    M, C = 300, 32
    cat, hraw = _rnd(g, M, 2 * C, dtype=f), _rnd(g, M, C, dtype=f)
    s2, h2 = _rnd(g, 2 * C, dtype=f).abs() + 0.5, _rnd(g, 2 * C, dtype=f) * 0.2
    w2, b2 = _rnd(g, 2, C, dtype=f) * 0.3, _rnd(g, 2, dtype=f) * 0.1
    fa = (cat, s2, h2, hraw, w2, b2)
    check(R.weighted_fuse_fwd(*[a.double() for a in fa]), R.weighted_fuse_fwd(*fa), "fuse")
    wts = R.weighted_fuse_fwd(*fa)["wts"][0]
    ba = (_rnd(g, M, C, dtype=f), cat, s2, h2, hraw, w2, wts)
    check(R.weighted_fuse_bwd(*[a.double() for a in ba], n_red=M), R.weighted_fuse_bwd(*ba, n_red=M), "fuse^T")
    xc, w, b = _rnd(g, M, C, dtype=f), _rnd(g, 3, C, dtype=f), _rnd(g, 3, dtype=f)
    sc, sh, mean, inv = s2[:C], h2[:C], _rnd(g, C, dtype=f) * 0.1, _rnd(g, C, dtype=f).abs() + 0.5
    check(R.cls_conv_fwd(xc.double(), sc.double(), sh.double(), R.RELU, w.double(), b.double(), 3),
          R.cls_conv_fwd(xc, sc, sh, R.RELU, w, b, 3), "cls")
    dlog = _rnd(g, 3, 3, M // 3, dtype=f)
    ca = (dlog, xc, sc, sh, R.RELU, mean, inv, w)
    check(R.cls_conv_bwd(*[a.double() if torch.is_tensor(a) else a for a in ca], M, M), R.cls_conv_bwd(*ca, M, M), "cls^T")
    x4, w4 = xc[:280].reshape(2, 10, 14, C)[..., :16].contiguous(), _rnd(g, 2, 16, 3, 3, dtype=f)
    ta = (x4, sc[:16], sh[:16], R.RELU)
    check(R.cls3x3_fwd(*[a.double() if torch.is_tensor(a) else a for a in ta], w4.double(), b[:2].double()),
          R.cls3x3_fwd(*ta, w4, b[:2]), "cls3x3")
    d4 = _rnd(g, 2, 2, 10, 14, dtype=f)
    ta = (d4, x4, sc[:16], sh[:16], R.RELU, mean[:16], inv[:16], w4)
    check(R.cls3x3_bwd(*[a.double() if torch.is_tensor(a) else a for a in ta], 280, 280), R.cls3x3_bwd(*ta, 280, 280), "cls3x3^T")
    col = _rnd(g, 2 * 5 * 7, 8 * 16, dtype=f)
    check(R.col2im_fwd(col.double(), 2, 5, 7, 8, 280), R.col2im_fwd(col, 2, 5, 7, 8, 280), "col2im")
    Dd, Yd = _rnd(g, 2, 10, 14, 8, dtype=f), _rnd(g, 2, 10, 14, 8, dtype=f)
    ia = [_rnd(g, 8, dtype=f) for _ in range(5)]
    check(R.im2col_bwd(Dd.double(), Yd.double(), *[a.double() for a in ia], R.RELU, 5, 7),
          R.im2col_bwd(Dd, Yd, *ia, R.RELU, 5, 7), "im2col")
