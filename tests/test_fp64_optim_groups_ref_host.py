"""The float64 reference of tests/_fp64_optim_groups_ref.py (the truth of tests/test_gpu_optim_groups.py) against
torch.optim.AdamW with two parameter groups and torch.optim.swa_utils.AveragedModel in float64 on the CPU, and the error bounds
it states met by a plain fp32 evaluation."""
import pytest
import torch

import _fp64_loss_ref as R
import _fp64_optim_groups_ref as G

D = torch.float64
B1, B2, EPS = 0.9, 0.999, 1e-8
SHAPES = [(7,), (37, 5), (1,), (3, 3), (2, 5, 3), (5,)]
GROUP_OF = [1, 0, 1, 0, 0, 1]                       # vectors in group 1 (no decay), the rest in group 0


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


def test_segment_table():
    assert G.segment_table([8], [0]) == ([2], [0])
    assert G.segment_table([7, 185, 1, 9, 30, 5], GROUP_OF) == ([2, 49, 50, 61, 63], [1, 0, 1, 0, 1])
    assert G.segment_table([4, 4, 4], [2, 2, 2]) == ([3], [2])                # neighbours of one group share a segment
    assert G.segment_table([1, 0, 1], [0, 1, 0]) == ([2], [0])                # an empty tensor takes no float4
    assert G.segment_table([5, 5], [0, 1]) == ([2, 4], [0, 1])                # the padding belongs to the tensor before it
    e = G.expand([2, 3], [1, 0], [10.0, 20.0])
    assert e.tolist() == [20.0] * 8 + [10.0] * 4


def test_grouped_reference_is_torch_adamw_with_two_groups():
    """three steps, a cosine scheduler stepping both groups between them"""
    g = torch.Generator().manual_seed(5)
    tq = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=D)) for s in SHAPES]
    groups = [{"params": [q for q, gi in zip(tq, GROUP_OF) if gi == 0], "lr": 1e-3, "weight_decay": 1e-2},
              {"params": [q for q, gi in zip(tq, GROUP_OF) if gi == 1], "lr": 1e-4, "weight_decay": 0.0}]
    opt = torch.optim.AdamW(groups, betas=(B1, B2), eps=EPS)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=3, eta_min=1e-5)
    ends, grp = G.segment_table([q.numel() for q in tq], GROUP_OF)
    p = _flat([q.detach() for q in tq])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    seen = []
    for step in (1, 2, 3):
        grads = [torch.randn(*s, generator=g, dtype=D) for s in SHAPES]
        for q, gr in zip(tq, grads):
            q.grad = gr.clone()
        lrs = [gr["lr"] for gr in opt.param_groups]
        seen.append(tuple(lrs))
        wds = [gr["weight_decay"] for gr in opt.param_groups]
        bc1, bc2s = R.bias_corrections(B1, B2, step, round32=False)
        lr = G.expand(ends, grp, lrs)
        wd = G.expand(ends, grp, wds)
        r = R.adamw_step(p, _flat(grads), m, v, lr, B1, B2, EPS, wd, bc1, bc2s, 1.0)
        opt.step()
        sched.step()
        p, m, v = r["p"][0], r["m"][0], r["v"][0]
        _close(p, _flat([q.detach() for q in tq]))
        _close(m, _flat([opt.state[q]["exp_avg"] for q in tq]))
        _close(v, _flat([opt.state[q]["exp_avg_sq"] for q in tq]))
    assert len(set(seen)) == 3 and all(a > b for a, b in seen), seen          # the scheduler moved both groups


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.999, 1.0])
def test_ema_reference_is_averaged_model(decay):
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3)).double()
    avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=False)
    avg.update_parameters(net)                       # the first call copies: the average starts from the weights, as the optimiser's does
    e = _flat([q.detach().clone() for q in net.parameters()])
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    for _ in range(3):
        net(torch.randn(6, 5, dtype=D)).square().sum().backward()
        opt.step()
        opt.zero_grad()
        avg.update_parameters(net)
        e, _ = G.ema_update(e, _flat([q.detach() for q in net.parameters()]), decay)
        _close(e, _flat([q.detach() for q in avg.module.parameters()]))
    if decay == 1.0:
        assert not torch.equal(e, _flat([q.detach() for q in net.parameters()]))


def test_warmup_schedule():
    for t in (1, 2, 3, 50, 1000):
        exact = G.ema_decay_at(0.999, t, True, round32=False)
        assert exact == min(0.999, (1 + t) / (10 + t))
        got = G.ema_decay_at(0.999, t, True)
        assert got == R.f32(got) and abs(got - exact) <= 3 * R.U * exact      # three fp32 roundings at most
    assert G.ema_decay_at(0.999, 1, True) == R.f32(R.f32(2.0) / R.f32(11.0))
    assert G.ema_decay_at(0.999, 10 ** 6, True) == R.f32(0.999) and G.ema_decay_at(0.25, 50, True) == 0.25
    assert G.ema_decay_at(0.999, 7, False) == R.f32(0.999) and G.ema_decay_at(0.999, 7, False, round32=False) == 0.999


def test_tables_cover_the_edges():
    n = 2048 * 256 * 4 + 4
    t = G.tables_for(n, 3)
    assert set(t) == {"one", "first", "last", "wg_edge", "iter_edge", "many"}
    assert t["iter_edge"][0] == [2048 * 256, n // 4] and t["wg_edge"][0] == [256, n // 4]
    assert len(t["many"][0]) == 300 and set(t["many"][1]) == {0, 1, 2}
    for ends, grp in t.values():
        assert ends == sorted(set(ends)) and ends[-1] == n // 4 and len(ends) == len(grp) and ends[0] > 0
    assert set(G.tables_for(8, 2)) == {"one", "first", "last"} and set(G.tables_for(8, 1)) == {"one"}
    assert G.launch_layout(n) == (2048, 2) and G.launch_layout(8) == (1, 1)


def test_fp32_evaluation_meets_the_bounds():
    n = 3380
    p, g, m, v = R.adamw_inputs(n, 21, "cpu")
    ends, grp = G.tables_for(n, 3)["many"]
    lrs, wds = (1e-3, 1e-5, 0.0), (1e-2, 0.0, 0.1)
    a = (R.f32(B1), R.f32(B2), R.f32(EPS))
    bc1, bc2s = R.bias_corrections(a[0], a[1], 38)
    r64 = G.grouped_step(p.double(), g.double(), m.double(), v.double(), ends, grp, lrs, wds, *a, bc1, bc2s, 0.25)
    t32 = [torch.tensor(x, dtype=torch.float32) for x in a + (bc1, bc2s)]
    r32 = G.grouped_step(p, g, m, v, ends, grp, lrs, wds, *t32, 0.25)
    for k in ("p", "m", "v"):
        d = (r32[k][0].double() - r64[k][0]).abs()
        assert bool((d <= r64[k][1]).all()), (k, (d / r64[k][1].clamp_min(1e-300)).max().item())
    # a wrong lookup is far outside the bound: the same step with the groups of the table rotated by one
    wrong = G.grouped_step(p.double(), g.double(), m.double(), v.double(), ends, [(x + 1) % 3 for x in grp], lrs, wds, *a, bc1, bc2s, 0.25)
    assert bool(((wrong["p"][0] - r64["p"][0]).abs() > 3 * r64["p"][1]).float().mean() > 0.5)
    e = torch.randn(n)
    for d in (0.0, 0.5, G.ema_decay_at(0.999, 3, True), 0.999, 1.0):
        d = R.f32(d)
        e64, err = G.ema_update(e.double(), r32["p"][0].double(), d)
        e32, _ = G.ema_update(e, r32["p"][0], torch.tensor(d, dtype=torch.float32))
        dd = (e32.double() - e64).abs()
        assert bool((dd <= err).all()), (d, (dd / err.clamp_min(1e-300)).max().item())
