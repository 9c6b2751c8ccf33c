"""Parameter groups and the EMA weight copy inside the device AdamW step: kd_adamw_step_groups_dev called through the C ABI on
raw buffers, then FusedAdamW on top of it.

The existing kernels are element-wise, so the grouped step is compared BIT FOR BIT with kd_adamw_step_dev run on each segment's
slice with that group's lr and weight_decay, each from a copy of the same starting state; with one group it is the whole-buffer
call, and with clipping kd_adamw_step_clip_dev (clip_state included).  The group hyper-parameters lie far apart (lr 1e-3 / 1e-5 /
0, weight decay 1e-2 / 0 / 0.1): a wrong lookup moves a parameter by far more than any rounding.  With clipping and several groups
the update is checked per element against the float64 reference of tests/_fp64_optim_groups_ref.py with the gradient scale read
back from clip_state (the method of tests/test_gpu_grad_clip.py); the EMA against the same reference applied to the pre-step
device state, with d_t read back from ema_state (and compared with the fp32 formula).

Sizes are the float4 grid-cap ladder (256 threads, one float4 per thread and iteration, at most 2048 blocks) and the three
published parameter counts; tables come from G.tables_for: one segment, a split after the first and before the last float4, a
boundary at a workgroup edge and at the iteration edge, 300 alternating segments (more than a workgroup has threads; left out
where the buffer has fewer than 300 float4s)."""
import copy
import math

import numpy as np
import pytest
import torch

import _fp64_clip_ref as C
import _fp64_loss_ref as R
import _fp64_optim_groups_ref as G
from test_gpu_grad_clip import DBuf, _clip_state, _same_bits, _scalar_ok
from test_gpu_loss_kernels import B1, B2, EPS, _guard_ok, _guarded
from test_gpu_tail_kernels import Buf, _check

pytestmark = pytest.mark.gpu

NAN = float("nan")
KD_ERR_ARG, KD_ERR_ALIGN, KD_ERR_SHAPE = -1, -2, -4
CAPN = 2048 * 256 * 4
SIZES = {"few": 8, "partial_block": 704, "cap-4": CAPN - 4, "cap": CAPN, "cap+4": CAPN + 4, "ragged_block": 1223340,
         "ragged_iter": C.CLIP_LADDER["ragged"], "model0": C.CLIP_LADDER["model0"], "model1": C.CLIP_LADDER["model1"],
         "model2": C.CLIP_LADDER["model2"]}
LRS, WDS = (1e-3, 1e-5, 0.0), (1e-2, 0.0, 0.1)


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


class Table:
    """a segment table as the entry point takes it: int32 device arrays and the host copies it validates"""

    def __init__(self, ends, groups):
        self.ends, self.groups, self.n = list(ends), list(groups), len(ends)
        self.he, self.hg = torch.tensor(ends, dtype=torch.int32), torch.tensor(groups, dtype=torch.int32)
        self.de, self.dg = self.he.cuda(), self.hg.cuda()


def _gstate(G_, lrs=LRS, wds=WDS):
    gs = Buf(G_, 2)
    gs.t.copy_(torch.tensor([[lrs[i], wds[i]] for i in range(G_)]))
    return gs


def _args(P, p, g, m, v, n, state, tab, gs, G_, ema=None, ema_state=None, decay=0.0, warm=0, cs=None, ws=None, ginv=1.0, max_norm=0.0):
    return (P(p), P(g), P(m), P(v), n, P(state), P(tab.de), P(tab.dg), P(tab.he), P(tab.hg), tab.n, P(gs.t), G_, P(ema), P(ema_state),
            decay, warm, None if cs is None else P(cs.t), None if ws is None else P(ws.t), 0 if ws is None else ws.nbytes, B1, B2, EPS, ginv,
            max_norm)


def _groups_step(p, g, m, v, n, state, tab, gs, G_, **kw):
    lib, P, stream = _lib()
    lib.call("kd_adamw_step_groups_dev", *_args(P, p, g, m, v, n, state, tab, gs, G_, **kw), stream())
    torch.cuda.synchronize()


def _slice_steps(p, g, m, v, state, tab, ginv, lrs=LRS, wds=WDS):
    """kd_adamw_step_dev on every segment's slice with its group's lr / wd, each from a copy of `state` -> the state after"""
    lib, P, stream = _lib()
    lo, st = 0, None
    for e, gi in zip(tab.ends, tab.groups):
        st = state.clone()
        st[0] = lrs[gi]
        a, b = 4 * lo, 4 * e
        lib.call("kd_adamw_step_dev", P(p[a:b]), P(g[a:b]), P(m[a:b]), P(v[a:b]), b - a, P(st), B1, B2, EPS, wds[gi], ginv, stream())
        lo = e
    torch.cuda.synchronize()
    return st


# ---- bit for bit against the existing kernels ---------------------------------------------------------------------------------

@pytest.mark.parametrize("G_", [1, 2, 3])
@pytest.mark.parametrize("size", list(SIZES))
def test_grouped_step_is_bit_identical_to_adamw_step_dev_on_the_slices(size, G_):
    n = SIZES[size]
    ginv = (1.0, 0.25, 1.0)[G_ - 1]
    p0, g0, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    gs = _gstate(G_)
    tables = G.tables_for(n, G_)
    assert ("many" in tables) == (G_ > 1 and n // 4 >= 300) and ("iter_edge" in tables) == (G_ > 1 and n > CAPN)
    for name, (ends, groups) in tables.items():
        tab = Table(ends, groups)
        (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
        rp, rm, rv = p0.clone(), m0.clone(), v0.clone()
        state = Buf(4)
        state.t.copy_(torch.tensor([NAN, 37.0, NAN, NAN]))          # state[0], the single learning rate, is neither read nor written
        rstate = state.t.clone()
        for k in range(3):
            what = f"[n={n} G={G_} table {name} ({tab.n} segments) step {k}]"
            g = g0 * (k + 0.5)
            _groups_step(p, g, m, v, n, state.t, tab, gs, G_, ginv=ginv)
            rstate = _slice_steps(rp, g, rm, rv, rstate, tab, ginv)
            for nm, x, y in (("p", p, rp), ("m", m, rm), ("v", v, rv), ("state[1:]", state.t[1:], rstate[1:])):
                assert _same_bits(x, y), f"{what} {nm} differs from kd_adamw_step_dev on the segments' slices"
            assert math.isnan(state.t[0].item()), what
        assert state.t[1].item() == 40.0 and not bool(torch.isnan(p).any())
        for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
            _guard_ok(bf, n, nm)
        state.guard_ok("state"); gs.guard_ok("group_state")
    if G_ > 1:                                                       # the groups really differ: the far-apart lr moved the parameters apart
        assert not torch.equal(rp, _one_group_result(p0, g0, m0, v0, n, ginv))


def test_longest_table_4096_segments():
    """the most segments the entry point accepts (32 KiB of dynamic LDS for the table), spread over both iterations of the
    grid-stride loop: bit for bit against kd_adamw_step_dev on the 4096 slices, two steps"""
    n, G_, ginv = SIZES["cap+4"], 3, 0.25
    n4 = n // 4
    stride = n4 // 4096                                              # boundaries all over the buffer, lengths stride - 3 .. stride + 3
    ends = [(i + 1) * stride + (i % 7) - 3 for i in range(4095)] + [n4]
    assert len(ends) == 4096 and ends == sorted(set(ends)) and ends[0] > 0 and sum(e > 2048 * 256 for e in ends) == 1
    tab, gs = Table(ends, [i % G_ for i in range(4096)]), _gstate(G_)
    p0, g0, m0, v0 = R.adamw_inputs(n, 11, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    rp, rm, rv = p0.clone(), m0.clone(), v0.clone()
    state = torch.tensor([NAN, 37.0, NAN, NAN], device="cuda")
    rstate = state.clone()
    for k in range(2):
        g = g0 * (k + 0.5)
        _groups_step(p, g, m, v, n, state, tab, gs, G_, ginv=ginv)
        rstate = _slice_steps(rp, g, rm, rv, rstate, tab, ginv)
        for nm, x, y in (("p", p, rp), ("m", m, rm), ("v", v, rv), ("state[1:]", state[1:], rstate[1:])):
            assert _same_bits(x, y), f"[4096 segments, step {k}] {nm} differs from kd_adamw_step_dev on the segments' slices"
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)
    lib, P, stream = _lib()
    longer = Table(list(range(1, 4097)) + [n4], [0] * 4097)
    assert lib.kd_adamw_step_groups_dev(*_args(P, p, g0, m, v, n, state, longer, gs, G_), stream()) == KD_ERR_SHAPE
    torch.cuda.synchronize()
    assert _same_bits(p, rp) and state[1].item() == 39.0


def _one_group_result(p0, g0, m0, v0, n, ginv):
    p, m, v = p0.clone(), m0.clone(), v0.clone()
    state = torch.tensor([NAN, 37.0, NAN, NAN], device="cuda")
    tab = Table([n // 4], [0])
    gs = _gstate(1)
    for k in range(3):
        _groups_step(p, g0 * (k + 0.5), m, v, n, state, tab, gs, 1, ginv=ginv)
    return p


@pytest.mark.parametrize("ginv,wd", [(1.0, 0.0), (0.25, 1e-3)])
@pytest.mark.parametrize("size", ["few", "partial_block", "cap+4", "ragged_iter", "model0"])
def test_one_group_with_clipping_is_bit_identical_to_adamw_step_clip_dev(size, ginv, wd):
    """coefficients about 0.1 and 0.9 and an unclipped step; parameters, moments, state and clip_state"""
    lib, P, stream = _lib()
    n = SIZES[size]
    p0, _, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    g0 = C.grad_inputs(n, n % 977, "cuda")
    a = [t.clone() for t in (p0, m0, v0)]
    b = [t.clone() for t in (p0, m0, v0)]
    sa = torch.tensor([1e-3, 37.0, 0.0, 0.0], device="cuda")
    sb = sa.clone()
    grid = C.sumsq_layout(n)[0]
    ca, wa, cb, wb = _clip_state(), DBuf(grid), _clip_state(), DBuf(grid)
    tab, gs = Table([n // 4], [0]), _gstate(1, (1e-3,), (wd,))
    for k, rel in enumerate((0.1, 0.9, 3.0)):
        g = g0 * (k + 0.5)
        max_norm = R.f32(rel * ginv * g.double().norm().item())
        _groups_step(a[0], g, a[1], a[2], n, sa, tab, gs, 1, cs=ca, ws=wa, ginv=ginv, max_norm=max_norm)
        lib.call("kd_adamw_step_clip_dev", P(b[0]), P(g), P(b[1]), P(b[2]), n, P(sb), P(cb.t), P(wb.t), wb.nbytes, B1, B2, EPS, wd, ginv,
                 max_norm, stream())
        torch.cuda.synchronize()
        assert n == 8 or (cb.t[1].item() < ginv) == (rel < 1.0)
        for nm, x, y in (("p", a[0], b[0]), ("m", a[1], b[1]), ("v", a[2], b[2]), ("state", sa, sb), ("clip_state", ca.t, cb.t), ("ws", wa.t, wb.t)):
            assert _same_bits(x, y), f"[n={n} ginv={ginv} wd={wd} step {k}] {nm} differs from kd_adamw_step_clip_dev"
    assert sa[1].item() == 40.0
    ca.guard_ok("clip_state"); wa.guard_ok("ws")


# ---- clipping with several groups ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("G_", [2, 3])
@pytest.mark.parametrize("size", ["partial_block", "cap+4", "model1"])
def test_clipped_groups(size, G_):
    lib, P, stream = _lib()
    n, ginv = SIZES[size], 0.25
    p0, _, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    g0 = C.grad_inputs(n, n % 977, "cuda")
    tables = G.tables_for(n, G_)
    ends, groups = tables["many"] if "many" in tables else tables["first"]
    tab, gs = Table(ends, groups), _gstate(G_)
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    grid = C.sumsq_layout(n)[0]
    state, cs, ws = Buf(4), _clip_state(), DBuf(grid)
    state.t.copy_(torch.tensor([NAN, 37.0, NAN, NAN]))
    ref_cs, ref_ws = _clip_state(), DBuf(grid)
    host = [0.0, 37.0, 0.0, 0.0]
    for k, rel in enumerate((0.1, 0.9, 3.0)):
        what = f"[n={n} G={G_} step {k} rel={rel}]"
        g = g0 * (k + 0.5)
        s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
        max_norm = R.f32(rel * ginv * math.sqrt(s64.item()))
        before = (p.clone(), m.clone(), v.clone())
        _groups_step(p, g, m, v, n, state.t, tab, gs, G_, cs=cs, ws=ws, ginv=ginv, max_norm=max_norm)
        # the same reduction: clip_state has the bits kd_adamw_step_clip_dev leaves on the same gradient
        scratch = [t.clone() for t in before]
        rst = torch.tensor([1e-3, 37.0 + k, 0.0, 0.0], device="cuda")
        lib.call("kd_adamw_step_clip_dev", P(scratch[0]), P(g), P(scratch[1]), P(scratch[2]), n, P(rst), P(ref_cs.t), P(ref_ws.t), ref_ws.nbytes,
                 B1, B2, EPS, 0.0, ginv, max_norm, stream())
        torch.cuda.synchronize()
        assert _same_bits(cs.t, ref_cs.t) and _same_bits(state.t[1:], rst[1:]), what
        c = cs.t.double().cpu()
        _scalar_ok(f"gscale {what}", c[1].item(), C.clip_scalars(s64, e_s, ginv, max_norm)["gscale"])
        assert (c[1].item() < ginv) == (rel < 1.0) and c[2].item() == 0.0 and c[3].item() == 1.0
        st = state.t.double().cpu()
        host, _ = R.adamw_tick(host, R.f32(B1), R.f32(B2))
        assert st[1].item() == host[1]
        upd = G.grouped_step(before[0].double(), g.double(), before[1].double(), before[2].double(), ends, groups, LRS, WDS, R.f32(B1), R.f32(B2),
                             R.f32(EPS), st[2].item(), st[3].item(), c[1].item())
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _check(f"adamw_step_groups_dev.{nm} {what}", got, upd[nm])
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)
    for nm, bf in (("state", state), ("clip_state", cs), ("ws", ws), ("group_state", gs)):
        bf.guard_ok(nm)


# ---- the EMA ------------------------------------------------------------------------------------------------------------------

TENSORS = [7, 185, 1, 9, 30, 5, 2048 * 3 + 1, 6]                    # no size is a multiple of 4: every tensor is padded
GROUP_OF = [1, 0, 1, 0, 0, 1, 0, 1]


def _padded(x, device="cuda"):
    """flat values laid out as FlatParams lays tensors of TENSORS out: zeros in the padding -> (buffer, padding mask)"""
    out, pad, pos = [], [], 0
    for nt in TENSORS:
        out += [x[pos:pos + nt], torch.zeros(-nt % 4, device=device)]
        pad += [torch.zeros(nt, dtype=torch.bool, device=device), torch.ones(-nt % 4, dtype=torch.bool, device=device)]
        pos += nt
    return torch.cat(out), torch.cat(pad)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("decay,warm", [(0.999, 0), (0.9, 1), (0.5, 0), (0.0, 0), (1.0, 0), (1.0, 1)])
def test_ema_update(decay, warm, clip):
    """three steps on a layout with padding: the EMA after each step against the reference applied to the EMA before it and the
    parameters after it, d_t read back and compared with the fp32 formula; decay 0 and 1 bit for bit; the padding stays 0"""
    ends, groups = G.segment_table(TENSORS, GROUP_OF)
    ntot = sum(TENSORS)
    raw = R.adamw_inputs(ntot, 31, "cuda")
    (p0, pad), (g0, _), (m0, _), (v0, _) = (_padded(t) for t in raw)
    n = p0.numel()
    assert n == 4 * ends[-1] and int(pad.sum()) == 20
    tab, gs = Table(ends, groups), _gstate(2)
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    e0 = _padded(torch.randn(ntot, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)))[0]
    (e, eb) = _guarded(e0)
    es, state = Buf(2), Buf(4)
    state.t.copy_(torch.tensor([NAN, 0.0, NAN, NAN]))               # a fresh run: the warm-up starts at t = 1
    cs, ws = (_clip_state(), DBuf(C.sumsq_layout(n)[0])) if clip else (None, None)
    for k in range(3):
        what = f"[decay={decay} warmup={warm} clip={clip} step {k}]"
        g = g0 * (k + 0.5)
        e_before = e.clone()
        max_norm = R.f32(0.5 * g.double().norm().item()) if clip else 0.0
        _groups_step(p, g, m, v, n, state.t, tab, gs, 2, ema=e, ema_state=es.t, decay=decay, warm=warm, cs=cs, ws=ws, max_norm=max_norm)
        t = state.t[1].item()
        assert t == k + 1.0
        d = es.t[0].item()
        assert d == G.ema_decay_at(decay, t, warm), (what, d)
        assert es.t[1].item() == R.f32(1.0 - d), what               # 1 - d_t: one fp32 subtraction
        if d == 0.0:
            assert _same_bits(e, p), f"{what}: decay 0 must store the new parameters bit for bit"
        elif d == 1.0:
            assert _same_bits(e, e_before), f"{what}: decay 1 must leave the EMA alone"
        else:
            _check(f"ema {what}", e, G.ema_update(e_before.double(), p.double(), d))
            assert not torch.equal(e, e_before) and not torch.equal(e, p)
        assert float(e[pad].abs().max()) == 0.0 and float(p[pad].abs().max()) == 0.0, f"{what}: padding elements stay 0"
    assert (decay, warm) != (1.0, 1) or es.t[0].item() == R.f32(R.f32(4.0) / R.f32(13.0))      # the warm-up, not the decay, decided
    for nm, bf in (("p", pb), ("m", mb), ("v", vb), ("ema", eb)):
        _guard_ok(bf, n, nm)
    es.guard_ok("ema_state"); state.guard_ok("state")
    # the EMA rides along: p, m, v are what the same steps give without it
    (p2, _), (m2, _), (v2, _) = _guarded(p0), _guarded(m0), _guarded(v0)
    st2 = torch.tensor([NAN, 0.0, NAN, NAN], device="cuda")
    cs2, ws2 = (_clip_state(), DBuf(C.sumsq_layout(n)[0])) if clip else (None, None)
    for k in range(3):
        g = g0 * (k + 0.5)
        _groups_step(p2, g, m2, v2, n, st2, tab, gs, 2, cs=cs2, ws=ws2, max_norm=R.f32(0.5 * g.double().norm().item()) if clip else 0.0)
    assert _same_bits(p, p2) and _same_bits(m, m2) and _same_bits(v, v2)


@pytest.mark.parametrize("size", ["cap+4", "ragged_block", "model2"])
def test_ema_at_scale(size):
    """the EMA over every launch shape of the ladder that differs: a second iteration, a ragged last block, a published model"""
    n = SIZES[size]
    p0, g0, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    ends, groups = G.tables_for(n, 3)["many"]
    tab, gs = Table(ends, groups), _gstate(3)
    (p, pb), (e, eb) = _guarded(p0), _guarded(p0 * 0.5 + 0.25)
    m, v = m0.clone(), v0.clone()
    es, state = Buf(2), torch.tensor([NAN, 37.0, NAN, NAN], device="cuda")
    e_before = e.clone()
    _groups_step(p, g0, m, v, n, state, tab, gs, 3, ema=e, ema_state=es.t, decay=0.999, warm=1)
    d = es.t[0].item()
    assert d == G.ema_decay_at(0.999, 38.0, True) == R.f32(R.f32(39.0) / R.f32(48.0))
    _check(f"ema [n={n}]", e, G.ema_update(e_before.double(), p.double(), d))
    _guard_ok(pb, n, "p"); _guard_ok(eb, n, "ema")


@pytest.mark.parametrize("t", [1, 2, 3, 50])
def test_warmup_values(t):
    n = 8
    p, g, m, v = R.adamw_inputs(n, 3, "cuda")
    e, es = p.clone(), Buf(2)
    state = torch.tensor([NAN, t - 1.0, NAN, NAN], device="cuda")
    _groups_step(p, g, m, v, n, state, Table([2], [0]), _gstate(1), 1, ema=e, ema_state=es.t, decay=0.999, warm=1)
    want = np.float32(min(np.float32(0.999), (np.float32(1) + np.float32(t)) / (np.float32(10) + np.float32(t))))
    assert state[1].item() == t and np.float32(es.t[0].item()) == want and np.float32(es.t[1].item()) == np.float32(1) - want
    assert (t < 50) == (want < np.float32(0.8)) and es.t[0].item() < R.f32(0.999)
    es.guard_ok("ema_state")


# ---- non-finite gradients -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("inf"), NAN], ids=["inf", "nan"])
def test_non_finite_gradient_skips_parameters_moments_and_ema(bad):
    n, ginv = SIZES["cap+4"], 0.25
    p0, _, m0, v0 = R.adamw_inputs(n, 5, "cuda")
    g = C.grad_inputs(n, 6, "cuda")
    ends, groups = G.tables_for(n, 2)["iter_edge"]
    tab, gs = Table(ends, groups), _gstate(2)
    e0 = p0 * 0.5
    (p, pb), (m, mb), (v, vb), (e, eb) = _guarded(p0), _guarded(m0), _guarded(v0), _guarded(e0)
    state, cs, ws, es = Buf(4), _clip_state(), DBuf(C.sumsq_layout(n)[0]), Buf(2)
    bc1, bc2s = R.bias_corrections(R.f32(B1), R.f32(B2), 37)
    state.t.copy_(torch.tensor([NAN, 37.0, bc1, bc2s]))
    es.t.copy_(torch.tensor([0.125, 0.875]))
    s0, es0 = state.t.clone(), es.t.clone()
    gbad = g.clone()
    gbad[n - 1] = bad
    kw = dict(ema=e, ema_state=es.t, decay=0.9, warm=1, cs=cs, ws=ws, ginv=ginv)
    for skipped in (1, 2):
        _groups_step(p, gbad, m, v, n, state.t, tab, gs, 2, max_norm=1.0, **kw)
        for nm, x, y in (("p", p, p0), ("m", m, m0), ("v", v, v0), ("ema", e, e0), ("state", state.t, s0), ("ema_state", es.t, es0)):
            assert _same_bits(x, y), f"{nm} changed in a skipped step"
        c = cs.t.cpu()
        assert not math.isfinite(c[0].item()) and c[1].item() == 0.0 and c[2].item() == float(skipped) and c[3].item() == 0.0, c
    # the next finite step is step 38 (the warm-up reads 38 too), and the counter of skipped steps stays
    s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
    max_norm = R.f32(0.5 * ginv * math.sqrt(s64.item()))
    _groups_step(p, g, m, v, n, state.t, tab, gs, 2, max_norm=max_norm, **kw)
    st, c = state.t.double().cpu(), cs.t.double().cpu()
    assert st[1].item() == 38.0 and c[2].item() == 2.0 and c[3].item() == 1.0
    assert es.t[0].item() == G.ema_decay_at(0.9, 38.0, True)
    upd = G.grouped_step(p0.double(), g.double(), m0.double(), v0.double(), ends, groups, LRS, WDS, R.f32(B1), R.f32(B2), R.f32(EPS),
                         st[2].item(), st[3].item(), c[1].item())
    for nm, got in (("p", p), ("m", m), ("v", v)):
        _check(f"adamw_step_groups_dev.{nm} after skipped steps", got, upd[nm])
    _check("ema after skipped steps", e, G.ema_update(e0.double(), p.double(), es.t[0].item()))
    for nm, bf in (("p", pb), ("m", mb), ("v", vb), ("ema", eb)):
        _guard_ok(bf, n, nm)
    for nm, bf in (("state", state), ("clip_state", cs), ("ws", ws), ("ema_state", es)):
        bf.guard_ok(nm)


# ---- graph replay -------------------------------------------------------------------------------------------------------------

def test_groups_ema_graph_replay():
    """a captured graph of the single call (one stream, no branches) replayed three times with the per-group lr table rewritten
    and a fresh gradient copied in before each replay: the lr, the norm, the step count, the bias corrections and the EMA warm-up
    all advance on the device"""
    lib, P, stream = _lib()
    n, ginv = SIZES["cap+4"], 1.0
    p0, _, m0, v0 = R.adamw_inputs(n, 77, "cuda")
    g0 = C.grad_inputs(n, 78, "cuda")
    ends, groups = G.tables_for(n, 3)["many"]
    tab, gs = Table(ends, groups), _gstate(3)
    (p, pb), (m, mb), (v, vb), (e, eb) = _guarded(p0), _guarded(m0), _guarded(v0), _guarded(p0)
    g = g0.clone()
    state = torch.tensor([NAN, 0.0, NAN, NAN], device="cuda")
    cs, ws, es = _clip_state(), DBuf(C.sumsq_layout(n)[0]), Buf(2)
    max_norm = R.f32(g0.double().norm().item())                      # replay 0 (g0 * 0.5) is not clipped, replays 1 and 2 are
    kw = dict(decay=0.999, warm=1, ginv=ginv, max_norm=max_norm)
    w = [t.clone() for t in (p0, g0, m0, v0, p0, state)]             # the kernels have run once before the capture
    wcs, wws, wes = _clip_state(), DBuf(C.sumsq_layout(n)[0]), Buf(2)
    _groups_step(w[0], w[1], w[2], w[3], n, w[5], tab, gs, 3, ema=w[4], ema_state=wes.t, cs=wcs, ws=wws, **kw)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.call("kd_adamw_step_groups_dev", *_args(P, p, g, m, v, n, state, tab, gs, 3, ema=e, ema_state=es.t, cs=cs, ws=ws, **kw), stream())
    torch.cuda.synchronize()
    assert state[1].item() == 0.0 and torch.equal(p, p0) and math.isnan(cs.t[0].item()) and math.isnan(es.t[0].item()), "capture must not execute"
    host = [0.0, 0.0, 0.0, 0.0]
    for k in range(3):
        lrs = tuple(R.f32(x * (1.0 - 0.3 * k)) for x in (1e-3, 1e-5, 2e-4))     # a scheduler step: every group moves
        gs.t[:, 0].copy_(torch.tensor(lrs))
        g.copy_(g0 * (k + 0.5))
        before = (p.clone(), m.clone(), v.clone(), e.clone())
        graph.replay()
        torch.cuda.synchronize()
        host, herr = R.adamw_tick(host, R.f32(B1), R.f32(B2))
        st, c = state.double().cpu(), cs.t.double().cpu()
        assert st[1].item() == k + 1.0 and abs(st[2].item() - host[2]) <= herr[2] and abs(st[3].item() - host[3]) <= herr[3]
        s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
        ref = C.clip_scalars(s64, e_s, ginv, max_norm)
        _scalar_ok(f"grad_norm [graph replay {k}]", c[0].item(), ref["norm"])
        _scalar_ok(f"gscale [graph replay {k}]", c[1].item(), ref["gscale"])
        assert (c[1].item() < ginv) == (k > 0) and c[3].item() == 1.0
        upd = G.grouped_step(before[0].double(), g.double(), before[1].double(), before[2].double(), ends, groups, lrs, WDS, R.f32(B1),
                             R.f32(B2), R.f32(EPS), st[2].item(), st[3].item(), c[1].item())
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _check(f"adamw_step_groups_dev.{nm} [graph replay {k}]", got, upd[nm])
        d = es.t[0].item()
        assert d == G.ema_decay_at(0.999, k + 1.0, True)
        _check(f"ema [graph replay {k}]", e, G.ema_update(before[3].double(), p.double(), d))
    for nm, bf in (("p", pb), ("m", mb), ("v", vb), ("ema", eb)):
        _guard_ok(bf, n, nm)
    cs.guard_ok("clip_state"); ws.guard_ok("ws"); es.guard_ok("ema_state"); gs.guard_ok("group_state")


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing():
    lib, P, stream = _lib()
    n = SIZES["partial_block"]
    n4 = n // 4
    p0, g, m0, v0 = R.adamw_inputs(n + 8, 3, "cuda")
    p, m, v, e = p0.clone(), m0.clone(), v0.clone(), p0.clone()
    state = torch.tensor([1e-3, 37.0, 0.5, 0.25], device="cuda")
    s0 = state.clone()
    gs, es = _gstate(2), Buf(2)
    good = Table([1, n4], [0, 1])

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(e, p0) and torch.equal(state, s0), what
        assert bool(torch.isnan(es.t).all()), what

    def call(tab=good, n_=n, G_=2, pp=None, ee=None):
        a = list(_args(P, p, g, m, v, n_, state, tab, gs, G_, ema=e, ema_state=es.t, decay=0.9))
        if pp is not None:
            a[0] = pp
        if ee is not None:
            a[13] = ee
        return lib.kd_adamw_step_groups_dev(*a, stream())

    for n_bad in (n + 2, n + 1, 0, -4):
        assert call(n_=n_bad) == KD_ERR_ARG, n_bad
        assert b"kd_adamw_step_groups_dev" in lib.kd_last_error_string()
        untouched(f"n={n_bad}")
    assert call(pp=p.data_ptr() + 4) == KD_ERR_ALIGN and b"aligned" in lib.kd_last_error_string()
    untouched("misaligned p")
    assert call(ee=e.data_ptr() + 8) == KD_ERR_ALIGN
    untouched("misaligned ema")
    for ends in ([1, n4 - 1], [1, n4 + 1]):
        assert call(Table(ends, [0, 1])) == KD_ERR_ARG and b"last segment" in lib.kd_last_error_string(), ends
        untouched(f"ends={ends}")
    assert call(Table([5, 5, n4], [0, 1, 0])) == KD_ERR_ARG and b"ascend" in lib.kd_last_error_string()
    untouched("ends not ascending")
    for grps in ([0, 2], [-1, 1]):
        assert call(Table([1, n4], grps)) == KD_ERR_ARG and b"group" in lib.kd_last_error_string(), grps
        untouched(f"groups={grps}")
    assert call(G_=1) == KD_ERR_ARG
    untouched("group index == G")
    assert call() == 0                                               # and the same buffers are accepted when the arguments are right
    torch.cuda.synchronize()
    assert state[1].item() == 38.0 and es.t[0].item() == R.f32(0.9) and not torch.equal(p, p0)
    es.guard_ok("ema_state"); gs.guard_ok("group_state")


# ---- the optimiser ------------------------------------------------------------------------------------------------------------

def _loaders(n=8, bs=4):
    from torch.utils.data import DataLoader
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    ds = SyntheticPandaSet(n_frames=n, num_points=1024, image_size=64, bev_size=16, seed=3, pad_tail=64)
    return DataLoader(ds, batch_size=bs, shuffle=False), DataLoader(ds, batch_size=bs, shuffle=False)


def _trainer(tmp_path, tag, **kw):
    from _gpu_util import build_product
    from src.training.trainer import Trainer
    tl, vl = _loaders()
    torch.manual_seed(0)
    tr = Trainer(build_product("weighted", 16), tl, vl, torch.device("cuda"), lr=1e-3, weight_decay=1e-2, save_dir=str(tmp_path / tag),
                 class_weights=[0.4, 3.5], num_epochs=3, **kw)
    tr.model.train()
    return tr, [tuple(b[k].cuda() for k in ("image", "points", "segmentation")) for b in tl]


@pytest.fixture
def calls(monkeypatch):
    from kdrt.lib import lib
    seen = []
    real = type(lib).call

    def counting(self, name, *a):
        seen.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(type(lib), "call", counting)
    return seen


OLD = ("kd_adamw_step", "kd_adamw_step_dev", "kd_adamw_step_clip_dev")
NEW = "kd_adamw_step_groups_dev"


def test_optimiser_steps_groups_and_ema_against_the_reference(tmp_path, calls):
    """decay_groups + flat_order = model.parameters() (what Trainer builds), one forward + backward per step, CosineAnnealingLR
    stepped between three steps; every step against the reference from pre-step snapshots"""
    from kdrt.optim import FusedAdamW, decay_groups
    tr, batches = _trainer(tmp_path, "groups", no_decay_norm_bias=True, lr_mult={"camera_encoder": 0.1}, ema_decay=0.9, ema_warmup=True,
                           max_grad_norm=1e-2)
    opt = tr.optimizer
    assert opt.grouped and len(opt.param_groups) == 4 and [id(q) for q in opt.flat.params] == [id(q) for q in tr.model.parameters()]
    numels = [q.numel() for q in opt.flat.params]
    gidx = {id(q): i for i, gr in enumerate(opt.param_groups) for q in gr["params"]}
    ends, groups = G.segment_table(numels, [gidx[id(q)] for q in opt.flat.params])
    assert (opt.seg_end_host.tolist(), opt.seg_group_host.tolist()) == (ends, groups) and len(ends) > 32
    assert torch.equal(opt.seg_end.cpu(), opt.seg_end_host) and torch.equal(opt.seg_group.cpu(), opt.seg_group_host)
    assert torch.equal(opt.ema, opt.flat.data)
    n = opt.flat.numel
    seen_lrs = []
    for k in range(3):
        what = f"[optimiser step {k}]"
        before = (opt.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone())
        tr._step(*batches[k % 2])
        torch.cuda.synchronize()
        lrs = [gr["lr"] for gr in opt.param_groups]
        wds = [gr["weight_decay"] for gr in opt.param_groups]
        seen_lrs.append(tuple(lrs))
        assert torch.equal(opt.group_state.cpu(), torch.tensor([[a, b] for a, b in zip(lrs, wds)], dtype=torch.float32)), what
        g = opt.flat.grad                                           # the step leaves the unclipped gradients
        s64, e_s = C.sumsq(g.double(), C.sumsq_n_seq(n))
        _scalar_ok(f"gscale {what}", opt.clip_state[1].item(), C.clip_scalars(s64, e_s, 1.0, R.f32(1e-2))["gscale"])
        st = opt.dev_state.double().cpu()
        assert st[1].item() == k + 1.0 and opt.clip_state[3].item() == 1.0
        upd = G.grouped_step(before[0].double(), g.double(), before[1].double(), before[2].double(), ends, groups, lrs, wds, R.f32(B1), R.f32(B2),
                             R.f32(EPS), st[2].item(), st[3].item(), opt.clip_state[1].item())
        for nm, got in (("p", opt.flat.data), ("m", opt.exp_avg), ("v", opt.exp_avg_sq)):
            _check(f"FusedAdamW.{nm} {what}", got, upd[nm])
        d = opt.ema_state[0].item()
        assert d == G.ema_decay_at(0.9, k + 1.0, True)
        _check(f"FusedAdamW.ema {what}", opt.ema, G.ema_update(before[3].double(), opt.flat.data.double(), d))
        tr.scheduler.step()
    assert len(set(seen_lrs)) == 3 and sorted({round(a / b, 6) for a, b in zip(seen_lrs[0], [1e-3] * 4)}) == [0.1, 1.0]
    print(f"gscale of the last step: {opt.clip_state[1].item():.6g}")
    assert calls.count(NEW) == 3 and not any(c in calls for c in OLD)
    # state_dict -> torch.optim.AdamW with the same groups -> back
    sd = opt.state_dict()
    ref = {id(q): torch.nn.Parameter(q.detach().clone()) for q in opt.flat.params}
    topt = torch.optim.AdamW([{**{k: v for k, v in gr.items() if k in ("lr", "weight_decay")}, "params": [ref[id(q)] for q in gr["params"]]}
                              for gr in opt.param_groups], betas=(B1, B2), eps=EPS)
    topt.load_state_dict(sd)
    for q in opt.flat.params[:5] + opt.flat.params[-5:]:
        stq = topt.state[ref[id(q)]]
        assert float(stq["step"]) == 3.0 and torch.equal(stq["exp_avg"], opt.state[q]["exp_avg"]) and torch.equal(stq["exp_avg_sq"], opt.state[q]["exp_avg_sq"])
    assert [gr["lr"] for gr in topt.param_groups] == [gr["lr"] for gr in opt.param_groups]
    m_before, v_before = opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    tsd = copy.deepcopy(topt.state_dict())                           # (torch keeps references to the tensors it was given)
    opt.exp_avg.zero_(); opt.exp_avg_sq.zero_()
    opt.load_state_dict(tsd)
    assert torch.equal(opt.exp_avg, m_before) and torch.equal(opt.exp_avg_sq, v_before) and opt.dev_state[1].item() == 3.0
    with pytest.raises(ValueError, match="betas"):
        bad = decay_groups(torch.nn.Linear(3, 3).cuda(), 1e-3, 1e-2)
        bad[1]["betas"] = (0.5, 0.999)
        FusedAdamW(bad, lr=1e-3)


def test_default_optimiser_never_calls_the_new_entry_point(tmp_path, calls):
    tr0, batches = _trainer(tmp_path, "off")
    for b in batches[:2]:
        tr0._step(*b)
    torch.cuda.synchronize()
    assert calls.count("kd_adamw_step_dev") == 2 and NEW not in calls and not tr0.optimizer.grouped
    assert tr0.optimizer.ema is None and tr0.optimizer.group_state is None
    assert list(tr0.history) == ["train_loss", "train_miou", "val_loss", "val_miou", "lr"]
    calls.clear()
    tr1, _ = _trainer(tmp_path, "clip", max_grad_norm=1e30)
    tr1._step(*batches[0])
    assert calls.count("kd_adamw_step_clip_dev") == 1 and NEW not in calls
    # an EMA alone (one group) goes through the new entry point and leaves the weights' bits alone
    calls.clear()
    tr2, _ = _trainer(tmp_path, "ema", ema_decay=0.5)
    for b in batches[:2]:
        tr2._step(*b)
    torch.cuda.synchronize()
    assert calls.count(NEW) == 2 and not any(c in calls for c in OLD)
    o0, o2 = tr0.optimizer, tr2.optimizer
    assert _same_bits(o0.flat.data, o2.flat.data) and _same_bits(o0.exp_avg, o2.exp_avg) and _same_bits(o0.exp_avg_sq, o2.exp_avg_sq)
    assert _same_bits(o0.dev_state[1:], o2.dev_state[1:]) and not torch.equal(o2.ema, o2.flat.data)
    # two groups with the same hyper-parameters: the same bits again, through the table
    calls.clear()
    tr3, _ = _trainer(tmp_path, "same", lr_mult={"camera_encoder": 1.0, "lidar_encoder": 1.0 + 2.0 ** -30})
    assert len(tr3.optimizer.param_groups) == 2 and tr3.optimizer.grouped
    for b in batches[:2]:
        tr3._step(*b)
    torch.cuda.synchronize()
    assert calls.count(NEW) == 2 and not any(c in calls for c in OLD)
    assert _same_bits(o0.flat.data, tr3.optimizer.flat.data) and _same_bits(o0.exp_avg_sq, tr3.optimizer.exp_avg_sq)


def test_graphed_kd_step_follows_group_lrs_and_the_ema_warmup():
    """GraphedKDStep is unchanged: it calls enqueue_update.  N replays == N eager steps with a scheduler that moves every
    group's lr by 10x between steps (a learning rate frozen at capture time would be off by 9e-4 per step) and the EMA warm-up
    advancing on the device; parameters and EMA within the tolerance tests/test_gpu_trainer.py uses for graph against eager
    (atol 1e-6, rtol 1e-5), the device tables exactly."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW, decay_groups
    B, HW, N, G_ = 2, 64, 512, 16
    images, pts, labels = (t.cuda() for t in O.make_inputs(B, HW, N, G_, 4, pad_tail=40))
    cw = torch.tensor([0.4, 3.5]).cuda()

    def make():
        teacher = build_product("concat", G_); load_random_state(teacher, "concat", 11)
        student = build_product("weighted", G_); load_random_state(student, "weighted", 12); student.train()
        opt = FusedAdamW(decay_groups(student, 1e-3, 1e-2, lr_mult={"camera_encoder": 0.5}), lr=1e-3, weight_decay=1e-2,
                         flat_order=student.parameters(), ema_decay=0.999, ema_warmup=True)
        return opt, KDStep(student, teacher, opt, cw), torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)

    opt_e, step_e, sched_e = make()
    for k in range(4):                                               # 1 warm-up + 3: same count as the graphed run below
        step_e(images, pts, labels)
        if k:
            sched_e.step()
    opt_g, step_g, sched_g = make()
    graphed = GraphedKDStep(step_g, images, pts, labels, warmup=1)
    for _ in range(3):
        graphed(images, pts, labels)
        sched_g.step()
    torch.cuda.synchronize()
    assert opt_g.dev_state[1].item() == 4.0 == opt_e.dev_state[1].item() and len(opt_g.param_groups) == 4
    assert torch.equal(opt_g.group_state, opt_e.group_state) and abs(opt_g.group_state[0, 0].item() / 5e-6 - 1.0) < 1e-6
    assert torch.equal(opt_g.ema_state, opt_e.ema_state) and opt_g.ema_state[0].item() == G.ema_decay_at(0.999, 4.0, True)
    for nm, a, b in (("p", opt_e.flat.data, opt_g.flat.data), ("ema", opt_e.ema, opt_g.ema), ("m", opt_e.exp_avg, opt_g.exp_avg)):
        assert torch.allclose(a, b, atol=1e-6, rtol=1e-5), (nm, (a - b).abs().max().item())
    assert not torch.allclose(opt_g.ema, opt_g.flat.data, atol=1e-6, rtol=1e-5)
