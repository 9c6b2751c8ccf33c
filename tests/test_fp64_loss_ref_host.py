"""The float64 references of tests/_fp64_loss_ref.py (the truth of tests/test_gpu_loss_kernels.py) against independent torch
expressions in float64 on the CPU, and the error bound they state met by a plain fp32 evaluation of the same formulas on the
inputs the GPU tests use at their small and middle sizes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fp64_loss_ref as R
import kd_oracle as O

D = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _d(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("T", [1.0, 4.0])
@pytest.mark.parametrize("ign", [-1, 255])
@pytest.mark.parametrize("teacher", [True, False], ids=["teacher", "ce_only"])
@pytest.mark.parametrize("weights", [True, False], ids=["weights", "unweighted"])
@pytest.mark.parametrize("NC", [2, 3, 4])
def test_seg_loss_is_cross_entropy_plus_kl(NC, weights, teacher, ign, T):
    B, HW = 3, 61
    zs, zt, y, cw = (_d(t) if t is not None and t.is_floating_point() else t
                     for t in R.seg_inputs(B, NC, HW, NC * 7 + ign % 5, "cpu", ign, 3.0, weights, teacher))
    alpha, gs = R.f32(0.7), R.f32(2.5)
    r = R.seg_loss(zs, zt, y, cw, ign, T, alpha, gs, n_seq=1)
    z = zs.clone().requires_grad_()
    # torch refuses labels outside 0..NC-1 other than ignore_index; the kernel drops them like ignore_index
    yt = torch.where((y >= 0) & (y < NC), y, torch.full_like(y, ign))
    ce = F.cross_entropy(z, yt, weight=cw, ignore_index=ign, reduction="mean")
    kl = torch.zeros((), dtype=D)
    if teacher:
        kl = F.kl_div(torch.log_softmax(z / T, 1), torch.log_softmax(zt / T, 1), reduction="sum", log_target=True) / (B * HW)
    (gs * (ce + alpha * T * T * kl)).backward()
    keep = yt != ign
    sw = (cw[yt[keep]].sum() if weights else keep.sum().double())
    _close(r["losses"][0], torch.stack([ce.detach(), kl.detach(), sw]))
    _close(r["dzs"][0], z.grad)
    assert bool((r["losses"][1] > 0).all() | (not teacher)) and bool((r["dzs"][1] >= 0).all())


def test_seg_loss_all_ignored_is_nan_like_torch():
    zs, zt, y, cw = R.seg_inputs(2, 3, 50, 1, "cpu")
    y = torch.full_like(y, -1)
    r = R.seg_loss(zs.double(), zt.double(), y, cw.double(), -1, 4.0, 1.0, 1.0, n_seq=1)
    assert torch.isnan(F.cross_entropy(zs, y, weight=cw, ignore_index=-1)) and torch.isnan(r["losses"][0][0])
    assert r["losses"][0][2].item() == 0 and bool(torch.isfinite(r["dzs"][0]).all()) and bool(torch.isfinite(r["dzs"][1]).all())
    z = zs.double().requires_grad_()
    (16 * F.kl_div(torch.log_softmax(z / 4, 1), torch.log_softmax(zt.double() / 4, 1), reduction="sum", log_target=True) / 100).backward()
    _close(r["dzs"][0], z.grad)


def test_mse_is_mse_loss():
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(3380, generator=g, dtype=D).requires_grad_(), torch.randn(3380, generator=g, dtype=D)
    want = F.mse_loss(a, b)
    (3.0 * 0.25 * want).backward()
    _close(R.mse_value(a.detach(), b, 1, chunk=1000)["loss"][0], want.detach())
    _close(R.mse_grad(a.detach(), b, 2.0 * 0.25 / 3380, 3.0)["da"][0], a.grad)


def test_kd_total_is_the_fp32_tensor_expression():
    g = torch.Generator().manual_seed(6)
    for _ in range(200):
        ce, kl, mc, ml = (torch.rand((), generator=g) * 3 for _ in range(4))
        ckl, beta = np.float32(0.7 * 16), np.float32(1.3)
        want = ce + float(ckl) * kl + float(beta) * (mc + ml)
        got = R.kd_total(ce.item(), kl.item(), mc.item(), ml.item(), ckl, beta)
        assert got.dtype == np.float32 and got == np.float32(want.item())
        assert R.kd_total(ce.item(), kl.item(), None, ml.item(), ckl, beta) == np.float32((ce + float(ckl) * kl + float(beta) * (0 + ml)).item())


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adamw_is_torch_adamw(wd):
    p0, g0, m0, v0 = (t.double() for t in R.adamw_inputs(700, 3, "cpu"))
    g = torch.Generator().manual_seed(4)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([q], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 7):
        lr = 1e-3 if step < 4 else 4e-4                  # a scheduler step in between
        opt.param_groups[0]["lr"] = lr
        grad = g0 * torch.rand(700, generator=g, dtype=D)
        q.grad = grad.clone()
        opt.step()
        bc1, bc2s = R.bias_corrections(0.9, 0.999, step, round32=False)
        r = R.adamw_step(p, grad, m, v, lr, 0.9, 0.999, 1e-8, wd, bc1, bc2s, 1.0)
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        st = opt.state[q]
        _close(p, q.detach()); _close(m, st["exp_avg"]); _close(v, st["exp_avg_sq"])
    # ginv scales the gradient before everything else
    r8 = R.adamw_step(p0, g0 * 8, m0, v0, 1e-3, 0.9, 0.999, 1e-8, wd, 0.5, 0.25, 0.125)
    r1 = R.adamw_step(p0, g0, m0, v0, 1e-3, 0.9, 0.999, 1e-8, wd, 0.5, 0.25, 1.0)
    for k in r1:
        _close(r8[k][0], r1[k][0])
    st, err = R.adamw_tick([1e-3, 37.0, 0.0, 0.0], 0.9, 0.999)
    assert st[1] == 38.0 and abs(st[2] - (1 - 0.9 ** 38)) < 1e-15 and abs(st[3] - (1 - 0.999 ** 38) ** 0.5) < 1e-15 and err[1] == 0


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("NC", [1, 2, 3, 4])
def test_confusion_is_the_oracle(NC, M):
    z, y = R.confusion_inputs(3, NC, 61, NC * 5 + M, "cpu", ignore_index=-1)
    pred, conf = R.confusion(z, y, M, -1)
    assert torch.equal(pred, torch.argmax(z, 1))                 # +-inf and signed-zero ties included
    assert torch.equal(conf, O.confusion_matrix(z.reshape(3, NC, 61, 1), y.reshape(3, 61, 1), M))
    assert conf.sum().item() > 0 or M == 1
    assert int(R.confusion(z, None, M, -1)[1].sum()) == 0


def _within(r64, r32, what):
    for k, (v, err) in r64.items():
        d = (r32[k][0].double() - v).abs()
        ok = (d <= err) | (torch.isnan(v) & torch.isnan(r32[k][0]))
        assert bool(ok.all()), (what, k, (d / err.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("size", ["few", "partial_block", "cap+1"])
@pytest.mark.parametrize("NC", [2, 3, 4])
def test_fp32_seg_loss_meets_the_bound(NC, size):
    B, HW = R.SEG_LADDER[size]
    for scale, T, ign in ((3.0, 4.0, -1), (60.0, 1.0, 255)):
        zs, zt, y, cw = R.seg_inputs(B, NC, HW, 11 + NC, "cpu", ign, scale)
        a = (ign, T, R.f32(0.7), R.f32(2.5 * 0.5), R.seg_n_seq(B * HW))
        _within(R.seg_loss(zs.double(), zt.double(), y, cw.double(), *a), R.seg_loss(zs, zt, y, cw, *a), (size, NC, scale))


@pytest.mark.parametrize("size", ["few", "partial_block", "cap+1"])
def test_fp32_mse_meets_the_bound(size):
    n = R.MSE_LADDER[size]
    g = torch.Generator().manual_seed(n % 1000)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gc = R.f32(2.0 * 1.3 / n)
    _within(R.mse_value(a, b, R.mse_n_seq(n), dtype=D), R.mse_value(a, b, R.mse_n_seq(n)), size)
    _within(R.mse_grad(a.double(), b.double(), gc, R.f32(0.5)), R.mse_grad(a, b, gc, R.f32(0.5)), size)


@pytest.mark.parametrize("n", [R.ADAMW_LADDER["few"], R.ADAMW_LADDER["partial_block"], R.PARAM_COUNTS[0]])
def test_fp32_adamw_meets_the_bound(n):
    p, g, m, v = R.adamw_inputs(n, 21, "cpu")
    for wd, ginv in ((0.0, 1.0), (1e-3, 0.125)):
        bc1, bc2s = R.bias_corrections(R.f32(0.9), R.f32(0.999), 38)
        a = (R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(wd), bc1, bc2s, ginv)
        f = np.float32
        r32 = R.adamw_step(p, g, m, v, *[torch.tensor(x, dtype=torch.float32) for x in a])
        _within(R.adamw_step(p.double(), g.double(), m.double(), v.double(), *a), r32, (n, wd))
