"""Global-norm gradient clipping inside the device AdamW step: kd_grad_sumsq_partials and kd_adamw_step_clip_dev called through
the C ABI and compared with the float64 reference of tests/_fp64_clip_ref.py (bound C_BOUND * n_seq * 2^-24 * sum|t_i|, n_seq
from the launch layout), then the optimiser, the steps and the trainers on top of them.

Sizes come from the launch layout (256 threads, one float4 per thread and iteration, at most 2048 blocks): a few elements, one
partial block, cap*per - 4, cap*per, cap*per + 4, a ragged third iteration and the three published parameter counts.  Every size
runs again with only element 0, only element n-1 and only the last ragged iteration non-zero, so a dropped or doubled element
costs O(1).  Workspace and outputs start as NaN and carry sentinel guard tails; the in-place buffers carry guard tails too.

The update is compared with R.adamw_step evaluated with the gradient scale READ BACK from clip_state: that is the fp32 value
the kernel multiplied by, an exact input, so R.adamw_step's own operation counts hold as they stand.

End to end, the moments after the first step are compared with (1 - beta1) * gi and (1 - beta2) * gi^2, gi = the IEEE fp32
product grad * gscale (a defined value: one rounding, the same in any evaluation), in float64.  The kernel rounds once more
for exp_avg ((1 - beta1) * gi) and twice more for exp_avg_sq (((1 - beta2) * gi) * gi): at most 2 roundings of 2^-24
relative each, below 2 ulp."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fp64_clip_ref as C
import _fp64_loss_ref as R
from test_gpu_loss_kernels import B1, B2, EPS, _adamw_ref, _guard_ok, _guarded
from test_gpu_tail_kernels import GUARD, SENT, Buf, _check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")
KD_ERR_ARG, KD_ERR_WORKSPACE = -1, -3


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


class DBuf:
    """a NaN-filled workspace of n doubles followed by a guard of sentinels"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), NAN, device="cuda", dtype=torch.float64)
        self.buf[n:] = SENT
        self.t = self.buf[:n]
        self.nbytes = 8 * n

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == SENT).all()), f"{what}: written past its end"


def _clip_state():
    """clip_state as a caller hands it over: everything NaN but the skipped-steps counter, which the call only increments"""
    cs = Buf(4)
    cs.t[2] = 0.0
    return cs


def _ibits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_ibits(a), _ibits(b))


def _scalar_ok(what, got, ref):
    val, err = ref
    print(f"{what}: got {got:.9g} float64 {val.item():.9g} |d|/err {abs(got - val.item()) / max(err.item(), 1e-300):.3f}")
    assert math.isfinite(got) and abs(got - val.item()) <= err.item(), (what, got, val.item(), err.item())


def _step(lib, P, stream, p, g, m, v, n, state, cs, ws, wd, ginv, max_norm):
    lib.call("kd_adamw_step_clip_dev", P(p), P(g), P(m), P(v), n, P(state), P(cs.t), P(ws.t), ws.nbytes, B1, B2, EPS, wd, ginv,
             max_norm, stream())
    torch.cuda.synchronize()


# ---- norm and coefficient ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", C.TAIL_MODES)
@pytest.mark.parametrize("size", list(C.CLIP_LADDER))
def test_norm_and_coefficient(size, mode):
    lib, P, stream = _lib()
    n = C.CLIP_LADDER[size]
    g, gb = _guarded(C.tail_only(C.grad_inputs(n, n % 977, "cuda"), mode))
    g0 = g.clone()
    grid, iters = C.sumsq_layout(n)
    n_seq = C.sumsq_n_seq(n)
    what = f"[n={n} {mode} grid={grid} iters={iters}]"
    assert lib.kd_grad_sumsq_ws_bytes(n) == grid * 8
    s64, e_s = C.sumsq(g.double(), n_seq)
    # the partial sums on their own, twice: the same bits
    ws, ws2 = DBuf(grid), DBuf(grid)
    lib.call("kd_grad_sumsq_partials", P(g), n, P(ws.t), ws.nbytes, stream())
    lib.call("kd_grad_sumsq_partials", P(g), n, P(ws2.t), ws2.nbytes, stream())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(ws.t).any()), f"{what}: partials never written"
    _scalar_ok(f"sumsq {what}", ws.t.sum().item(), (s64, e_s))
    assert torch.equal(ws.t, ws2.t), what
    ws.guard_ok("ws"); ws2.guard_ok("ws")
    # norm, coefficient and gradient scale through the step
    p0, _, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    norm64 = math.sqrt(s64.item())
    for ginv in (1.0, 0.25):
        for rel in (0.1, 0.9, 4.0):
            (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
            state, cs, ws = Buf(4), _clip_state(), DBuf(grid)
            state.t.copy_(torch.tensor([1e-3, 37.0, NAN, NAN]))
            max_norm = R.f32(rel * ginv * norm64)
            _step(lib, P, stream, p, g, m, v, n, state.t, cs, ws, 1e-3, ginv, max_norm)
            ref = C.clip_scalars(s64, e_s, ginv, max_norm)
            c = cs.t.double().cpu()
            w = f"{what} ginv={ginv} rel={rel}"
            _scalar_ok(f"grad_norm {w}", c[0].item(), ref["norm"])
            _scalar_ok(f"gscale {w}", c[1].item(), ref["gscale"])
            _scalar_ok(f"clip_coef {w}", c[1].item() / ginv, ref["coef"])          # ginv is a power of two: the quotient is exact
            cref = max_norm / (ginv * norm64 + C.NORM_EPS)       # (a lone tiny element: the 1e-6 of the formula decides, not rel)
            if cref > 1.001:
                assert np.float32(c[1].item()) == np.float32(ginv), (w, c)         # not clipped: bit-equal to ginv
            elif cref < 0.999:
                assert c[1].item() < ginv, (w, c)
            assert c[2].item() == 0.0 and c[3].item() == 1.0, (w, c)
            assert state.t[1].item() == 38.0 and not bool(torch.isnan(state.t).any()), w
            assert not bool(torch.isnan(p).any() | torch.isnan(m).any() | torch.isnan(v).any()), w
            for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
                _guard_ok(bf, n, nm)
            for nm, bf in (("state", state), ("clip_state", cs), ("ws", ws)):
                bf.guard_ok(nm)
    assert torch.equal(g, g0), "the gradient is only read"
    _guard_ok(gb, n, "g")


# ---- the update -------------------------------------------------------------------------------------------------------------

def _tick_ok(state, host, what):
    host, herr = R.adamw_tick(host, R.f32(B1), R.f32(B2))
    st = state.double().cpu()
    for i in range(4):
        assert abs(st[i].item() - host[i]) <= herr[i] + (R.U * host[0] if i == 0 else 0), (what, i, st[i].item(), host[i])
    return host, st


@pytest.mark.parametrize("ginv,wd", [(1.0, 0.0), (1.0, 1e-3), (0.25, 0.0), (0.25, 1e-3)])
@pytest.mark.parametrize("size", ["partial_block", "cap+4", "ragged", "model1"])
def test_clipped_update_three_steps(size, ginv, wd):
    """three consecutive steps with the coefficient about 0.1, about 0.9 and exactly 1"""
    lib, P, stream = _lib()
    n = C.CLIP_LADDER[size]
    p0, _, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    g0 = C.grad_inputs(n, n % 977, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    grid = C.sumsq_layout(n)[0]
    state, cs, ws = Buf(4), _clip_state(), DBuf(grid)
    state.t.copy_(torch.tensor([1e-3, 37.0, NAN, NAN]))
    host = [R.f32(1e-3), 37.0, 0.0, 0.0]
    gen = torch.Generator(device="cuda").manual_seed(n)
    for k, rel in enumerate((0.1, 0.9, 3.0)):
        what = f"[n={n} ginv={ginv} wd={wd} step {k} rel={rel}]"
        g = g0 * (torch.rand(n, generator=gen, device="cuda") * 2)
        s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
        max_norm = R.f32(rel * ginv * math.sqrt(s64.item()))
        before = (p.clone(), m.clone(), v.clone())               # the GPU's own state: errors do not compound
        _step(lib, P, stream, p, g, m, v, n, state.t, cs, ws, wd, ginv, max_norm)
        host, st = _tick_ok(state.t, host, what)
        c = cs.t.double().cpu()
        ref = C.clip_scalars(s64, e_s, ginv, max_norm)
        _scalar_ok(f"gscale {what}", c[1].item(), ref["gscale"])
        if rel > 1:
            assert np.float32(c[1].item()) == np.float32(ginv), what     # exactly 1: bit-equal to ginv
        else:
            assert abs(c[1].item() / ginv - rel) < 1e-3 * rel, (what, c[1].item())
        assert c[2].item() == 0.0 and c[3].item() == 1.0
        upd = _adamw_ref(before[0], g, before[1], before[2], st[0].item(), wd, st[2].item(), st[3].item(), c[1].item())
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _check(f"adamw_step_clip_dev.{nm} {what}", got, upd[nm])
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)
    for nm, bf in (("state", state), ("clip_state", cs), ("ws", ws)):
        bf.guard_ok(nm)


@pytest.mark.parametrize("ginv,wd", [(1.0, 0.0), (0.25, 1e-3)])
@pytest.mark.parametrize("size", ["few", "partial_block", "cap+4", "model0"])
def test_unclipped_step_is_bit_identical_to_adamw_step_dev(size, ginv, wd):
    lib, P, stream = _lib()
    n = C.CLIP_LADDER[size]
    p0, _, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    g0 = C.grad_inputs(n, n % 977, "cuda")
    a = [t.clone() for t in (p0, m0, v0)]
    b = [t.clone() for t in (p0, m0, v0)]
    sa = torch.tensor([1e-3, 37.0, 0.0, 0.0], device="cuda")
    sb = sa.clone()
    cs, ws = _clip_state(), DBuf(C.sumsq_layout(n)[0])
    for k in range(3):
        g = g0 * (k + 0.5)
        _step(lib, P, stream, a[0], g, a[1], a[2], n, sa, cs, ws, wd, ginv, 1e30)
        lib.call("kd_adamw_step_dev", P(b[0]), P(g), P(b[1]), P(b[2]), n, P(sb), B1, B2, EPS, wd, ginv, stream())
        torch.cuda.synchronize()
        assert np.float32(cs.t[1].item()) == np.float32(ginv) and cs.t[3].item() == 1.0
        for nm, x, y in (("p", a[0], b[0]), ("m", a[1], b[1]), ("v", a[2], b[2]), ("state", sa, sb)):
            assert _same_bits(x, y), f"[n={n} ginv={ginv} wd={wd} step {k}] {nm} differs from kd_adamw_step_dev"
    assert sa[1].item() == 40.0


# ---- non-finite gradients -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("bad", [float("inf"), NAN], ids=["inf", "nan"])
def test_non_finite_gradient_skips_the_step(bad, where):
    lib, P, stream = _lib()
    n, wd, ginv = C.CLIP_LADDER["cap+4"], 1e-3, 0.25
    p0, _, m0, v0 = R.adamw_inputs(n, 5, "cuda")
    g = C.grad_inputs(n, 6, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    state, cs, ws = Buf(4), _clip_state(), DBuf(C.sumsq_layout(n)[0])
    bc1, bc2s = R.bias_corrections(R.f32(B1), R.f32(B2), 37)
    state.t.copy_(torch.tensor([1e-3, 37.0, bc1, bc2s]))
    s0 = state.t.clone()
    gbad = g.clone()
    gbad[0 if where == "first" else n - 1] = bad
    _step(lib, P, stream, p, gbad, m, v, n, state.t, cs, ws, wd, ginv, 1.0)
    for nm, x, y in (("p", p, p0), ("m", m, m0), ("v", v, v0), ("state", state.t, s0)):
        assert _same_bits(x, y), f"{nm} changed in a skipped step"
    c = cs.t.cpu()
    assert not math.isfinite(c[0].item()) and c[2].item() == 1.0 and c[3].item() == 0.0 and c[1].item() == 0.0, c
    # the next finite step is step 38, and the counter of skipped steps stays
    s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
    max_norm = R.f32(0.5 * ginv * math.sqrt(s64.item()))
    _step(lib, P, stream, p, g, m, v, n, state.t, cs, ws, wd, ginv, max_norm)
    _, st = _tick_ok(state.t, [R.f32(1e-3), 37.0, 0.0, 0.0], "after a skipped step")
    assert st[1].item() == 38.0
    c = cs.t.double().cpu()
    assert c[2].item() == 1.0 and c[3].item() == 1.0
    _scalar_ok("grad_norm after a skipped step", c[0].item(), C.clip_scalars(s64, e_s, ginv, max_norm)["norm"])
    _scalar_ok("gscale after a skipped step", c[1].item(), C.clip_scalars(s64, e_s, ginv, max_norm)["gscale"])
    upd = _adamw_ref(p0, g, m0, v0, 1e-3, wd, st[2].item(), st[3].item(), c[1].item())
    for nm, got in (("p", p), ("m", m), ("v", v)):
        _check(f"adamw_step_clip_dev.{nm} after a skipped step", got, upd[nm])
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)
    for nm, bf in (("state", state), ("clip_state", cs), ("ws", ws)):
        bf.guard_ok(nm)


# ---- graph replay -------------------------------------------------------------------------------------------------------------

def test_adamw_clip_dev_graph_replay():
    """a captured graph of the single kd_adamw_step_clip_dev call (one stream, no branches) replayed three times with a fresh
    gradient copied in before each replay: norm, coefficient, step count and bias corrections advance on the device"""
    lib, P, stream = _lib()
    n, wd, ginv = C.CLIP_LADDER["cap+4"], 1e-3, 1.0
    p0, _, m0, v0 = R.adamw_inputs(n, 77, "cuda")
    g0 = C.grad_inputs(n, 78, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    g = g0.clone()
    state = torch.tensor([1e-3, 37.0, 0.0, 0.0], device="cuda")
    cs, ws = _clip_state(), DBuf(C.sumsq_layout(n)[0])
    s64_0, _ = C.sumsq(g0.double(), C.sumsq_n_seq(n))
    max_norm = R.f32(math.sqrt(s64_0.item()))                    # replay 0 (g0 * 0.5) is not clipped, replays 1 and 2 are
    w = [t.clone() for t in (p0, g0, m0, v0, state)]             # the kernels have run once before the capture
    wcs, wws = _clip_state(), DBuf(C.sumsq_layout(n)[0])
    _step(lib, P, stream, w[0], w[1], w[2], w[3], n, w[4], wcs, wws, wd, ginv, max_norm)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.call("kd_adamw_step_clip_dev", P(p), P(g), P(m), P(v), n, P(state), P(cs.t), P(ws.t), ws.nbytes, B1, B2, EPS, wd, ginv,
                 max_norm, stream())
    torch.cuda.synchronize()
    assert state[1].item() == 37.0 and torch.equal(p, p0) and math.isnan(cs.t[0].item()), "capture must not execute"
    host = [R.f32(1e-3), 37.0, 0.0, 0.0]
    for k in range(3):
        g.copy_(g0 * (k + 0.5))
        before = (p.clone(), m.clone(), v.clone())
        graph.replay()
        torch.cuda.synchronize()
        host, st = _tick_ok(state, host, f"replay {k}")
        assert st[1].item() == 38.0 + k
        s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
        ref = C.clip_scalars(s64, e_s, ginv, max_norm)
        c = cs.t.double().cpu()
        _scalar_ok(f"grad_norm [graph replay {k}]", c[0].item(), ref["norm"])
        _scalar_ok(f"gscale [graph replay {k}]", c[1].item(), ref["gscale"])
        assert (c[1].item() < ginv) == (k > 0) and c[3].item() == 1.0
        upd = _adamw_ref(before[0], g, before[1], before[2], 1e-3, wd, st[2].item(), st[3].item(), c[1].item())
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _check(f"adamw_step_clip_dev.{nm} [graph replay {k}]", got, upd[nm])
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)
    cs.guard_ok("clip_state"); ws.guard_ok("ws")


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    lib, P, stream = _lib()
    n = C.CLIP_LADDER["partial_block"]
    grid = C.sumsq_layout(n)[0]
    p0, _, m0, v0 = R.adamw_inputs(n + 4, 3, "cuda")
    g = C.grad_inputs(n + 4, 4, "cuda")
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    state = torch.tensor([1e-3, 37.0, 0.5, 0.25], device="cuda")
    s0 = state.clone()
    cs, ws = _clip_state(), DBuf(grid)
    cs0 = cs.buf.clone()

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(state, s0), what
        assert _same_bits(cs.buf, cs0) and bool(torch.isnan(ws.t).all()), what
        ws.guard_ok(what)

    def call(n_, max_norm, nbytes):
        return lib.kd_adamw_step_clip_dev(P(p), P(g), P(m), P(v), n_, P(state), P(cs.t), P(ws.t), nbytes, B1, B2, EPS, 1e-3, 1.0,
                                          max_norm, stream())

    for n_bad in (n + 2, n + 1, 0, -4):
        assert call(n_bad, 1.0, ws.nbytes) == KD_ERR_ARG, n_bad
        assert b"kd_adamw_step_clip_dev" in lib.kd_last_error_string()
        untouched(f"n={n_bad}")
    for mn in (0.0, -1.0, float("inf"), float("-inf"), NAN):
        assert call(n, mn, ws.nbytes) == KD_ERR_ARG, mn
        untouched(f"max_norm={mn}")
    assert call(n, 1.0, ws.nbytes - 8) == KD_ERR_WORKSPACE
    untouched("short workspace")
    assert call(n, 1.0, 0) == KD_ERR_WORKSPACE
    untouched("no workspace bytes")
    # the partial sums on their own
    for n_bad in (n + 2, 0):
        assert lib.kd_grad_sumsq_partials(P(g), n_bad, P(ws.t), ws.nbytes, stream()) == KD_ERR_ARG
        untouched(f"partials n={n_bad}")
    assert lib.kd_grad_sumsq_partials(P(g), n, P(ws.t), ws.nbytes - 8, stream()) == KD_ERR_WORKSPACE
    untouched("partials short workspace")
    assert call(n, 1.0, ws.nbytes) == 0                           # and the same buffers are accepted when the arguments are right
    torch.cuda.synchronize()
    assert cs.t[3].item() == 1.0 and state[1].item() == 38.0


# ---- optimiser, steps and trainers -----------------------------------------------------------------------------------------------

def _loaders(n=8, bs=4):
    from torch.utils.data import DataLoader
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    ds = SyntheticPandaSet(n_frames=n, num_points=1024, image_size=64, bev_size=16, seed=3, pad_tail=64)
    return DataLoader(ds, batch_size=bs, shuffle=False), DataLoader(ds, batch_size=bs, shuffle=False)


def _model(fusion):
    from _gpu_util import build_product
    torch.manual_seed(0)
    return build_product(fusion, 16)


def _trainer(tmp_path, max_grad_norm, tag):
    from src.training.trainer import Trainer
    tl, vl = _loaders()
    kw = {} if max_grad_norm is None else {"max_grad_norm": max_grad_norm}
    tr = Trainer(_model("weighted"), tl, vl, torch.device("cuda"), lr=1e-3, weight_decay=1e-3, save_dir=str(tmp_path / tag),
                 class_weights=[0.4, 3.5], num_epochs=3, **kw)
    tr.model.train()
    return tr, [tuple(b[k].cuda() for k in ("image", "points", "segmentation")) for b in tl]


def _norm_ok(opt, max_norm, what):
    """opt.last_grad_norm against the float64 norm of opt.flat.grad (which the step leaves unclipped) -> the gscale used"""
    n = opt.flat.numel
    s64, e_s = C.sumsq(opt.flat.grad.double(), C.sumsq_n_seq(n))
    ref = C.clip_scalars(s64, e_s, R.f32(opt.grad_scale), R.f32(max_norm))
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda
    _scalar_ok(f"last_grad_norm {what}", opt.last_grad_norm.item(), ref["norm"])
    _scalar_ok(f"gscale {what}", opt.clip_state[1].item(), ref["gscale"])
    return opt.clip_state[1].item()


def _first_step_moments_ok(opt, gs, what):
    b1, b2 = (R.f32(b) for b in opt.param_groups[0]["betas"])
    gi = (opt.flat.grad * torch.tensor(gs, device="cuda", dtype=torch.float32)).double()      # one IEEE fp32 product
    for nm, got, want in (("exp_avg", opt.exp_avg, (1.0 - b1) * gi), ("exp_avg_sq", opt.exp_avg_sq, (1.0 - b2) * gi * gi)):
        ulp = torch.maximum(want.abs() * 2.0 ** -23, torch.full_like(want, 2.0 ** -149))
        d = (got.double() - want).abs()
        worst = (d / ulp).max().item()
        print(f"{nm} {what}: worst {worst:.3f} ulp")
        assert worst <= 2.0, (what, nm, worst)
    assert float(opt.exp_avg.abs().max()) > 0


def test_trainer_steps_clip_and_default_is_unchanged(tmp_path, monkeypatch):
    from kdrt.lib import lib
    calls = []
    real = type(lib).call

    def counting(self, name, *a):
        calls.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(type(lib), "call", counting)
    # default: exactly today's call, no clipping state, the reference's history layout
    tr0, batches = _trainer(tmp_path, None, "off")
    for b in batches[:2]:
        tr0._step(*b)
    torch.cuda.synchronize()
    assert calls.count("kd_adamw_step_dev") == 2 and "kd_adamw_step_clip_dev" not in calls and "kd_grad_sumsq_partials" not in calls
    assert tr0.optimizer.max_grad_norm is None and tr0.optimizer.clip_state is None and tr0.optimizer.skipped_steps() == 0
    assert list(tr0.history) == ["train_loss", "train_miou", "val_loss", "val_miou", "lr"]
    with pytest.raises(RuntimeError):
        tr0.optimizer.last_grad_norm
    # a bound that never clips: the same bits
    calls.clear()
    tr1, _ = _trainer(tmp_path, 1e30, "never")
    norms = []
    for b in batches[:2]:
        tr1._step(*b)
        norms.append(tr1.optimizer.last_grad_norm.item())
    assert calls.count("kd_adamw_step_clip_dev") == 2 and "kd_adamw_step_dev" not in calls
    o0, o1 = tr0.optimizer, tr1.optimizer
    assert torch.equal(o0.flat.data, o1.flat.data) and torch.equal(o0.exp_avg, o1.exp_avg) and torch.equal(o0.exp_avg_sq, o1.exp_avg_sq)
    assert torch.equal(o0.flat.grad, o1.flat.grad) and _same_bits(o0.dev_state, o1.dev_state)
    assert all(math.isfinite(x) and x > 0 for x in norms), norms
    # a bound below the observed norm
    max_norm = 0.5 * min(norms)
    tr2, _ = _trainer(tmp_path, max_norm, "on")
    opt = tr2.optimizer
    tr2._step(*batches[0])
    torch.cuda.synchronize()
    gs = _norm_ok(opt, max_norm, "Trainer step 1")
    assert 0.4 < gs < 0.6, gs
    _first_step_moments_ok(opt, gs, "Trainer step 1")
    tr2._step(*batches[1])
    torch.cuda.synchronize()
    gs2 = _norm_ok(opt, max_norm, "Trainer step 2")
    assert gs2 < 1.0 and not torch.equal(opt.flat.data, o1.flat.data)
    # state_dict: torch.optim.AdamW's layout, loads into torch.optim.AdamW, the step count is the device counter
    sd = opt.state_dict()
    assert "max_grad_norm" not in sd["param_groups"][0] and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    ref_params = [torch.nn.Parameter(q.detach().clone()) for q in opt.flat.params]
    topt = torch.optim.AdamW(ref_params, lr=1e-3, weight_decay=1e-3)
    topt.load_state_dict(sd)
    assert float(topt.state[ref_params[0]]["step"]) == 2.0
    assert torch.equal(topt.state[ref_params[0]]["exp_avg"], opt.state[opt.flat.params[0]]["exp_avg"])
    # a non-finite gradient: the optimiser skips, the step count stays, the history reports it
    before = (opt.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone())
    opt.flat.grad[opt.flat.numel - 1] = float("inf")
    opt.step()
    assert opt.skipped_steps() == 1 and not math.isfinite(opt.last_grad_norm.item())
    assert torch.equal(before[0], opt.flat.data) and torch.equal(before[1], opt.exp_avg) and torch.equal(before[2], opt.exp_avg_sq)
    assert opt._step == 3                                         # the host-side hint counted the skipped step ...
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0 and opt._step == 2      # ... the device counter did not, and it decides
    assert list(tr2.history) == ["train_loss", "train_miou", "val_loss", "val_miou", "lr", "grad_norm", "skipped_steps"]
    tr2.last_epoch_grad_norm = 0.5 * (norms[0] + norms[1])
    tr2.update_history(1.0, 0.5, 1.0, 0.5, 1e-3)
    hist = json.load(open(os.path.join(tr2.save_dir, "training_history.json")))
    assert hist["skipped_steps"] == [1] and len(hist["grad_norm"]) == 1


def test_kd_step_clips_and_reports_the_norm():
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    B, HW, N, G = 2, 64, 512, 16
    images, pts, labels = (t.cuda() for t in O.make_inputs(B, HW, N, G, 4, pad_tail=40))
    cw = torch.tensor([0.4, 3.5]).cuda()

    def make(max_grad_norm):
        teacher = build_product("concat", G); load_random_state(teacher, "concat", 11)
        student = build_product("weighted", G); load_random_state(student, "weighted", 12); student.train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3, max_grad_norm=max_grad_norm)
        return opt, KDStep(student, teacher, opt, cw)

    opt0, step0 = make(None)
    parts0 = step0(images, pts, labels)
    assert "grad_norm" not in parts0
    observed = opt0.flat.grad.double().norm().item()
    max_norm = 0.25 * observed
    opt, step = make(max_norm)
    parts = step(images, pts, labels)
    torch.cuda.synchronize()
    assert parts["grad_norm"].is_cuda and parts["grad_norm"].dim() == 0
    assert parts["grad_norm"].data_ptr() == opt.last_grad_norm.data_ptr()
    assert torch.equal(opt.flat.grad, opt0.flat.grad), "p.grad keeps the unclipped gradients"
    gs = _norm_ok(opt, max_norm, "KDStep")
    assert 0.2 < gs < 0.3, gs
    _first_step_moments_ok(opt, gs, "KDStep")
    assert not torch.equal(opt.exp_avg, opt0.exp_avg)
    with pytest.raises(ValueError):
        make(0.0)
    with pytest.raises(ValueError):
        make(float("inf"))


# ---- forced reducer, a world of one rank ------------------------------------------------------------------------------------------

def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_forced_reducer_clips_after_finish(tmp_path):
    out = tmp_path / "res.json"
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()),
               KD_CLIP_OUT=str(out), OMP_NUM_THREADS="2")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_grad_clip_world1_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    print(res)
    assert res["world"] == 1 and res["collectives"] == 3 * res["steps"], res       # 3 buckets per step really went to RCCL
    assert res["bit_identical_steps"] == [True] * res["steps"], res                 # parameters, gradients, moments, clip state
    assert all(res["norm_within_bound"]) and all(g < 1.0 for g in res["gscale"]), res
