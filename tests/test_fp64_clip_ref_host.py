"""The float64 reference of tests/_fp64_clip_ref.py (the truth of tests/test_gpu_grad_clip.py) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in float64 on the CPU, and the error bound it states met by a plain fp32
evaluation in the kernel's summation order."""
import math

import pytest
import torch

import _fp64_clip_ref as C
import _fp64_loss_ref as R

D = torch.float64
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _flat(ts):
    """the FlatParams layout: every tensor padded with zeros to a multiple of 4 elements"""
    out = []
    for t in ts:
        out.append(t.reshape(-1))
        out.append(torch.zeros(-t.numel() % 4, dtype=t.dtype))
    return torch.cat(out)


CASES = {"one": [(8,)], "vec_mat": [(7,), (37, 5)], "padded": [(1,), (3, 3), (2, 5, 3)], "many": [(300, 9), (5,), (2,), (64, 3, 3)]}


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("rel", [0.1, 0.9, 10.0], ids=["coef0.1", "coef0.9", "unclipped"])
@pytest.mark.parametrize("case", list(CASES))
def test_clipped_step_is_clip_grad_norm_then_adamw(case, rel, wd):
    g = torch.Generator().manual_seed(len(case) + int(10 * rel))
    shapes = CASES[case]
    tq = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=D)) for s in shapes]
    opt = torch.optim.AdamW(tq, weight_decay=wd, **HP)
    p = _flat([q.detach() for q in tq])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2):
        grads = [torch.randn(*s, generator=g, dtype=D) * 10.0 ** float(torch.randint(-3, 2, (1,), generator=g)) for s in shapes]
        for q, gr in zip(tq, grads):
            q.grad = gr.clone()
        gf = _flat(grads)
        max_norm = rel * gf.norm().item()
        total = torch.nn.utils.clip_grad_norm_(tq, max_norm)
        opt.step()
        r = C.clipped_step(p, gf, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, step, 1.0, max_norm, norm_eps=1e-6, round32=False)
        assert not r["skipped"] and (r["coef"][0].item() < 1.0) == (rel < 1.0)
        _close(r["norm"][0], total.detach())
        _close(r["coef"][0], torch.tensor(min(1.0, max_norm / (total.item() + 1e-6)), dtype=D))
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        _close(p, _flat([q.detach() for q in tq]))
        _close(m, _flat([opt.state[q]["exp_avg"] for q in tq]))
        _close(v, _flat([opt.state[q]["exp_avg_sq"] for q in tq]))


def test_ginv_scales_the_norm_not_the_coefficient_floor():
    """the norm is that of the averaged gradient: ginv = 1/4 on 4x the gradient gives the same norm, coefficient and step"""
    g = C.grad_inputs(3380, 5, "cpu").double()
    p, _, m, v = (t.double() for t in R.adamw_inputs(3380, 6, "cpu"))
    a = C.clipped_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 3, 1.0, 0.5 * g.norm().item())
    b = C.clipped_step(p, 4 * g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 3, 0.25, 0.5 * g.norm().item())
    _close(a["norm"][0], b["norm"][0])
    _close(a["coef"][0], b["coef"][0])
    _close(a["gscale"][0], 4 * b["gscale"][0])
    for k in ("p", "m", "v"):
        _close(a[k][0], b[k][0])


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_gradient_skips(bad):
    g = C.grad_inputs(700, 1, "cpu").double()
    g[699] = bad
    p, _, m, v = (t.double() for t in R.adamw_inputs(700, 2, "cpu"))
    r = C.clipped_step(p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 1, 1.0, 1.0)
    assert r["skipped"] and not math.isfinite(r["norm"][0].item())
    assert torch.equal(r["p"][0], p) and torch.equal(r["m"][0], m) and torch.equal(r["v"][0], v)


def test_layout_and_ladder():
    assert C.sumsq_layout(8) == (1, 1) and C.sumsq_layout(3380) == (4, 1)
    assert C.sumsq_layout(C.CAP * C.PER - 4) == (C.CAP, 1) and C.sumsq_layout(C.CAP * C.PER) == (C.CAP, 1)
    assert C.sumsq_layout(C.CAP * C.PER + 4) == (C.CAP, 2) and C.sumsq_layout(C.CLIP_LADDER["ragged"]) == (C.CAP, 3)
    assert C.CLIP_LADDER["ragged"] % C.PER != 0
    assert all(n % 4 == 0 and n > 0 for n in C.CLIP_LADDER.values())
    assert [C.CLIP_LADDER[f"model{i}"] for i in range(3)] == [528132, 573444, 494980]
    assert C.sumsq_n_seq(8) == 10 and C.sumsq_n_seq(C.CLIP_LADDER["ragged"]) == 18


@pytest.mark.parametrize("mode", C.TAIL_MODES)
@pytest.mark.parametrize("size", ["few", "partial_block", "cap+4", "model0"])
def test_fp32_in_kernel_order_meets_the_bound(size, mode):
    n = C.CLIP_LADDER[size]
    g = C.tail_only(C.grad_inputs(n, n % 977, "cpu"), mode)
    assert float(g.abs().max()) > 0 and (mode in ("all", "ragged") or int((g != 0).sum()) == 1)
    n_seq = C.sumsq_n_seq(n)
    s64, e_s = C.sumsq(g.double(), n_seq)
    part64, part32 = C.sumsq_kernel_order(g.double()), C.sumsq_kernel_order(g)
    _close(part64.sum(), s64)                                     # the layout drops and doubles nothing
    s32 = part32.sum()
    assert abs(s32.item() - s64.item()) <= e_s.item(), (size, mode, abs(s32.item() - s64.item()) / max(e_s.item(), 1e-300))
    for ginv in (1.0, 0.25):
        for rel in (0.1, 0.9, 1.0 + 1e-7, 4.0):
            max_norm = R.f32(rel * ginv * math.sqrt(s64.item()))
            ref = C.clip_scalars(s64, e_s, ginv, max_norm)
            # plain fp32: the norm rounded once from the fp32-order sum, then fp32 scalar operations
            norm = torch.tensor(ginv * math.sqrt(s32.item()), dtype=torch.float32)
            c = (torch.tensor(max_norm, dtype=torch.float32) / (norm + torch.tensor(C.NORM_EPS, dtype=torch.float32))).clamp_max(1.0)
            gs = torch.tensor(ginv, dtype=torch.float32) * c
            for k, got in (("norm", norm), ("coef", c), ("gscale", gs)):
                val, err = ref[k]
                assert abs(got.double().item() - val.item()) <= err.item(), (size, mode, ginv, rel, k, got.item(), val.item(), err.item())
            if c.item() == 1.0:
                assert gs.item() == R.f32(ginv)                   # an unclipped step scales by ginv, bit for bit


def test_fp32_clipped_update_meets_the_bound():
    n = C.CLIP_LADDER["partial_block"]
    p, _, m, v = R.adamw_inputs(n, 21, "cpu")
    g = C.grad_inputs(n, 22, "cpu")
    for wd, ginv, rel in ((0.0, 1.0, 0.1), (1e-3, 0.25, 0.9), (1e-3, 1.0, 5.0)):
        max_norm = R.f32(rel * ginv * g.double().norm().item())
        a = (R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(wd))
        r32 = C.clipped_step(p, g, m, v, *[torch.tensor(x, dtype=torch.float32) for x in a], 38, ginv, max_norm)
        gs = r32["gscale"][0].double().item()                     # the fp32 scale the fp32 evaluation used, as the GPU test reads it back
        bc1, bc2s = R.bias_corrections(a[1], a[2], 38)
        r64 = R.adamw_step(p.double(), g.double(), m.double(), v.double(), *a, bc1, bc2s, gs)
        for k in ("p", "m", "v"):
            d = (r32[k][0].double() - r64[k][0]).abs()
            assert bool((d <= r64[k][1]).all()), (wd, ginv, rel, k, (d / r64[k][1].clamp_min(1e-300)).max().item())
