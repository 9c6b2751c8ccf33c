"""The loss, metric and optimiser kernels of csrc/kd_loss.hip called directly through the C ABI and compared with a float64
evaluation of the same operation on the same fp32 inputs (tests/_fp64_loss_ref.py, plain torch on the GPU): element-wise
within C_BOUND * n_seq * 2^-24 * sum|t_i| for the loss, its gradient, the MSE and AdamW; bit for bit for the KD total;
exactly for argmax and confusion matrix.

Sizes come from each launch layout (256 threads; at most 1024 blocks for loss and metric, 2048 for MSE and AdamW): a few
elements, one partial block, cap*256 - 1, cap*256, cap*256 + 1, a ragged third iteration and the benchmarked count.  Every
reduction runs again with only its tail contributing (the last ragged iteration, the last block, element 0, element n-1),
so a dropped or doubled element costs O(1).  Every output, slab and workspace starts as NaN and carries a sentinel guard
tail; the in-place AdamW buffers carry guard tails too.  With KD_LOSS_BOUNDS_OUT set, the worst |got - value| / err seen
per kernel output is written to that file (profiles/loss_kernel_bounds.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

import _fp64_loss_ref as R
from test_gpu_tail_kernels import GUARD, SENT, Buf, _big, _check

pytestmark = pytest.mark.gpu

ISENT = -(2 ** 40) - 77
WORST = {}
B1, B2, EPS = 0.9, 0.999, 1e-8


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


@pytest.fixture(scope="module", autouse=True)
def _bounds_report():
    yield
    path = os.environ.get("KD_LOSS_BOUNDS_OUT")
    if path and WORST:
        with open(path, "w") as f:
            f.write("# worst |got - float64| / err per kernel output over all cases of tests/test_gpu_loss_kernels.py (1 = the bound)\n")
            for k in sorted(WORST):
                f.write(f"{k:28s} {WORST[k]:.4f}\n")


def _chk(name, got, ref, what=""):
    val, err = ref
    r = (got.double().reshape(val.shape) - val).abs() / err.clamp_min(1e-300)
    r = r[~torch.isnan(r)]
    if r.numel():
        WORST[name] = max(WORST.get(name, 0.0), r.max().item())
    _check(f"{name} {what}", got, ref)


def _d(t):
    return None if t is None else t.double()


class IBuf:
    """an int64 output of n elements filled with a sentinel, followed by a guard of the same"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + GUARD,), ISENT, device="cuda", dtype=torch.int64)
        self.t = self.buf[:n]

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == ISENT).all()), f"{what}: written past its end"


def _guarded(t):
    """a copy of flat fp32 `t` followed by a guard of sentinels -> (view of the copy, whole buffer)"""
    buf = torch.full((t.numel() + GUARD,), SENT, device="cuda")
    buf[:t.numel()] = t
    return buf[:t.numel()], buf


def _guard_ok(buf, n, what):
    assert bool((buf[n:] == SENT).all()), f"{what}: written past its end"


# ---- segmentation loss ----------------------------------------------------------------------------------------------------

# (ignore_index, T, gscale, gscale_dev)
VARIANTS = [(-1, 4.0, 1.0, None), (255, 1.0, 2.5, None), (-1, 1.0, 1.0, 0.5), (255, 4.0, 2.5, 0.5)]


def _seg_run(size, NC, weights, teacher, grad, variant=0, scale=3.0, mode="all", alpha=0.7):
    lib, P, stream = _lib()
    B, HW = R.SEG_LADDER[size] if isinstance(size, str) else size
    ign, T, gscale, gdev = VARIANTS[variant % 4]
    npix = B * HW
    zs, zt, y, cw = R.seg_inputs(B, NC, HW, npix % 997 + 10 * NC + variant, "cuda", ign, scale, weights, teacher)
    grid, iters = R.seg_layout(npix)
    tail = R.tail_mask(npix, grid, iters, "cuda").view(B, HW)
    if mode == "tail_ce":
        y = torch.where(tail, y.clamp(0, NC - 1), torch.full_like(y, ign))
    elif mode == "tail_kl":
        zt = torch.where(tail[:, None, :], zt, zs)
    elif mode == "all_ignored":
        y = torch.full_like(y, ign)
    nbytes = lib.kd_seg_loss_ws_bytes(npix)
    assert nbytes == grid * 16
    ws, losses = Buf(nbytes // 4), Buf(3)
    dzs = Buf(B, NC, HW) if grad else None
    gd = None if gdev is None else torch.tensor([gdev], device="cuda")
    lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), ign, T, alpha, gscale, P(gd), P(losses.t), P(dzs.t) if grad else None,
             B, NC, HW, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    gs = R.f32(gscale) * (1.0 if gdev is None else R.f32(gdev))
    ref = R.seg_loss(zs.double(), _d(zt), y, _d(cw), ign, R.f32(T), R.f32(alpha), gs, R.seg_n_seq(npix), want_grad=grad)
    what = f"[{size} NC={NC} w={weights} t={teacher} ign={ign} T={T} {mode}]"
    val, err = ref["losses"]
    if mode == "all_ignored":
        assert bool(torch.isnan(losses.t[0])) and bool(torch.isnan(val[0])), f"CE of an all-ignored batch is NaN like torch's {what}"
        assert losses.t[2].item() == 0.0
    else:
        assert bool(val[2] > 0)
        _chk("seg_loss.losses[0] ce", losses.t[0:1], (val[0:1], err[0:1]), what)
        _chk("seg_loss.losses[2] sumw", losses.t[2:3], (val[2:3], err[2:3]), what)
    _chk("seg_loss.losses[1] kl", losses.t[1:2], (val[1:2], err[1:2]), what)
    if not teacher:
        assert losses.t[1].item() == 0.0
    if grad:
        assert bool(torch.isfinite(dzs.t).all()), what
        _chk("seg_loss.dzs", dzs.t, ref["dzs"], what)
        dzs.guard_ok("dzs")
    ws.guard_ok("ws"); losses.guard_ok("losses")
    return zs, zt


CROSS = [(nc, w, t, g) for nc in (2, 3, 4) for w in (True, False) for t in (True, False) for g in (True, False)]
PRUNED = [(2, True, True, True), (3, False, True, True), (4, True, False, True), (3, True, True, False)]


@pytest.mark.parametrize("size", ["few", "partial_block"])
@pytest.mark.parametrize("i", range(len(CROSS)), ids=lambda i: "NC%d-w%d-t%d-g%d" % CROSS[i])
def test_seg_loss_small(size, i):
    _seg_run(size, *CROSS[i], variant=i + i // 4 + (size == "few"))


@pytest.mark.parametrize("size", ["cap-1", "cap", "cap+1", "ragged", "bench"])
@pytest.mark.parametrize("i", range(len(PRUNED)), ids=lambda i: "NC%d-w%d-t%d-g%d" % PRUNED[i])
def test_seg_loss_ladder(size, i):
    _seg_run(size, *PRUNED[i], variant=i + list(R.SEG_LADDER).index(size))


def test_seg_loss_x4_head_count():
    _big()
    _seg_run(R.SEG_X4, 2, True, True, True, variant=0)


@pytest.mark.parametrize("NC", [2, 4])
def test_seg_loss_teacher_probabilities_underflow(NC):
    """logits of scale 60 at T = 1: teacher probabilities underflow to 0 (the `pt > 0` guard of the KL sum)"""
    zs, zt = _seg_run("cap+1", NC, True, True, True, variant=1, scale=60.0)
    assert bool((torch.softmax(zt, 1) == 0).any())


@pytest.mark.parametrize("mode", ["tail_ce", "tail_kl"])
@pytest.mark.parametrize("size,NC", [("partial_block", 3), ("cap+1", 2), ("ragged", 4), ("bench", 2)])
def test_seg_loss_tail_only(size, NC, mode):
    _seg_run(size, NC, True, True, True, variant=list(R.SEG_LADDER).index(size), mode=mode)


@pytest.mark.parametrize("size,NC,variant", [("partial_block", 3, 0), ("cap+1", 2, 3)])
def test_seg_loss_all_ignored(size, NC, variant):
    """losses[0] is NaN like torch's, losses[2] == 0, dzs is the KL part alone and finite"""
    _seg_run(size, NC, True, True, True, variant=variant, mode="all_ignored")


def test_seg_loss_refuses_bad_class_weights():
    from kdrt.lib import KDError
    from kdrt.losses import seg_loss
    z, y = torch.randn(2, 3, 4, 5, device="cuda"), torch.zeros(2, 4, 5, dtype=torch.int64, device="cuda")
    for cw in (torch.ones(2, device="cuda"), torch.ones(4, device="cuda"), torch.ones(3, device="cuda", dtype=torch.float64), torch.ones(3)):
        with pytest.raises(KDError):
            seg_loss(z, y, cw)
    seg_loss(z, y, torch.ones(3, device="cuda"))


# ---- feature MSE and the KD total -----------------------------------------------------------------------------------------

CHUNK = 1 << 26


def _chk_da(name, da, a, b, gc, gd, what):
    for o in range(0, a.numel(), CHUNK):
        s = slice(o, o + CHUNK)
        _chk(name, da[s], R.mse_grad(a[s].double(), b[s].double(), gc, gd)["da"], what)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _mse_run(n, tail=False, huge=False):
    lib, P, stream = _lib()
    g = torch.Generator(device="cuda").manual_seed(n % 1009)
    a = torch.randn(n, generator=g, device="cuda")
    b = torch.randn(n, generator=g, device="cuda")
    grid, iters = R.mse_layout(n)
    if tail:
        b = torch.where(R.tail_mask(n // 4, grid, iters, "cuda").repeat_interleave(4), b, a)
    what = f"[n={n} tail={tail}]"
    nbytes = lib.kd_mse_ws_bytes(n)
    assert nbytes == grid * 4 and lib.kd_mse_slab_blocks(n) == grid
    gc, gdev = R.f32(2.0 * 1.3 / n), 0.5
    gd = torch.tensor([gdev], device="cuda")
    n_seq = R.mse_n_seq(n)
    ref_loss = R.mse_value(a, b, n_seq, dtype=torch.float64, chunk=CHUNK)["loss"]
    # value and gradient in one call, upstream gradient on the device
    ws, loss, da = Buf(grid), Buf(1), Buf(n)
    lib.call("kd_mse_fwd_bwd", P(a), P(b), n, gc, P(gd), P(loss.t), P(da.t), P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    _chk("mse_fwd_bwd.loss", loss.t, ref_loss, what)
    _chk_da("mse_fwd_bwd.da", da.t, a, b, gc, R.f32(gdev), what)
    for nm, bf in (("ws", ws), ("loss", loss), ("da", da)):
        bf.guard_ok(nm)
    if not huge:
        # each output alone gives the same bits
        ws2, loss2, da2 = Buf(grid), Buf(1), Buf(n)
        lib.call("kd_mse_fwd_bwd", P(a), P(b), n, gc, P(gd), P(loss2.t), None, P(ws2.t), nbytes, stream())
        lib.call("kd_mse_fwd_bwd", P(a), P(b), n, gc, P(gd), None, P(da2.t), P(ws2.t), nbytes, stream())
        torch.cuda.synchronize()
        assert torch.equal(loss2.t, loss.t) and torch.equal(da2.t, da.t), what
        ws2.guard_ok("ws"); loss2.guard_ok("loss"); da2.guard_ok("da")
        del ws2, loss2, da2
    del da
    # the slab form: two partial calls (the second over a shorter prefix, operands swapped) and the one-launch final
    n_l = max(4, (n // 3) // 4 * 4)
    slab_c, slab_l = Buf(grid), Buf(lib.kd_mse_slab_blocks(n_l))
    da_c = None if huge else Buf(n)
    lib.call("kd_mse_partial", P(a), P(b), n, gc, None if huge else P(da_c.t), P(slab_c.t), stream())
    lib.call("kd_mse_partial", P(b), P(a), n_l, gc, None, P(slab_l.t), stream())
    ce_kl = torch.tensor([0.8131, 0.0237, 5.0, 0.0], device="cuda")
    ckl, beta = R.f32(0.7 * 16), R.f32(1.3)
    out, total = Buf(3), Buf(1)
    lib.call("kd_kd_objective_final", P(ce_kl), P(slab_c.t), n, P(slab_l.t), n_l, ckl, beta, P(out.t), stream())
    lib.call("kd_kd_total", P(ce_kl), P(out.t[0:1]), P(out.t[1:2]), ckl, beta, P(total.t), stream())
    torch.cuda.synchronize()
    _chk("objective_final.out[0]", out.t[0:1], ref_loss, what)
    _chk("objective_final.out[1]", out.t[1:2], R.mse_value(b[:n_l], a[:n_l], R.mse_n_seq(n_l), dtype=torch.float64, chunk=CHUNK)["loss"], what)
    if not huge:
        _chk_da("mse_partial.da", da_c.t, a, b, gc, 1.0, what)
        da_c.guard_ok("da")
    o = out.t.cpu().numpy()
    want = R.kd_total(0.8131, 0.0237, o[0], o[1], ckl, beta)
    assert _bits(out.t[2:3])[0] == np.array([want]).view(np.uint32)[0], (what, o[2], want)
    assert _bits(total.t)[0] == _bits(out.t[2:3])[0], "kd_kd_total and kd_kd_objective_final disagree"
    for nm, bf in (("slab_c", slab_c), ("slab_l", slab_l), ("out", out), ("total", total)):
        bf.guard_ok(nm)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("size", list(R.MSE_LADDER))
def test_mse_ladder(size, tail):
    _mse_run(R.MSE_LADDER[size], tail)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
def test_mse_bench_count(tail):
    _big()
    _mse_run(R.MSE_BENCH, tail)


def test_mse_above_2_31_elements():
    _big()
    _mse_run(R.MSE_HUGE, huge=True)


def test_kd_total_missing_terms_and_order():
    """kd_kd_total with either MSE missing, against the fp32 order of operations, bit for bit"""
    lib, P, stream = _lib()
    g = torch.Generator().manual_seed(8)
    for k in range(64):
        v = (torch.rand(4, generator=g) * torch.tensor([3.0, 0.1, 2.0, 2.0])).cuda()
        ckl, beta = R.f32(0.3 * (k % 5 + 1) ** 2), R.f32(0.1 + 0.37 * (k % 7))
        ce_kl = torch.cat([v[:2], torch.zeros(2, device="cuda")])
        c, l = (v[2:3] if k % 3 != 1 else None), (v[3:4] if k % 3 != 2 else None)
        total = Buf(1)
        lib.call("kd_kd_total", P(ce_kl), P(c), P(l), ckl, beta, P(total.t), stream())
        torch.cuda.synchronize()
        h = v.cpu().numpy()
        want = R.kd_total(h[0], h[1], None if c is None else h[2], None if l is None else h[3], ckl, beta)
        assert _bits(total.t)[0] == np.array([want]).view(np.uint32)[0], (k, total.t.item(), want)
        total.guard_ok("total")


# ---- argmax + confusion ---------------------------------------------------------------------------------------------------

def _metric_run(size, NC, M, ign=-1):
    lib, P, stream = _lib()
    B, HW = R.SEG_LADDER[size] if isinstance(size, str) else size
    npix = B * HW
    conf = IBuf(M * M)
    conf.t.zero_()
    want_total = torch.zeros(M, M, dtype=torch.int64, device="cuda")
    what = f"[{size} NC={NC} M={M}]"
    for call in range(3):                                       # one matrix accumulated over three calls, checked after each
        z, y = R.confusion_inputs(B, NC, HW, npix % 991 + 16 * NC + 4 * M + call, "cuda", ign)
        pred = IBuf(npix)
        lib.call("kd_argmax_confusion", P(z), P(y), ign, P(conf.t), P(pred.t), B, NC, M, HW, stream())
        torch.cuda.synchronize()
        wp, wc = R.confusion(z, y, M, ign)
        want_total += wc
        assert torch.equal(pred.t.view(B, HW), wp), f"pred {what} call {call}"
        assert torch.equal(conf.t.view(M, M), want_total), f"conf {what} call {call}: {conf.t.tolist()} != {want_total.tolist()}"
        pred.guard_ok("pred"); conf.guard_ok("conf")
    # pred only, conf only, no target
    p2, c2, c3 = IBuf(npix), IBuf(M * M), IBuf(M * M)
    c2.t.zero_(); c3.t.fill_(5)
    lib.call("kd_argmax_confusion", P(z), P(y), ign, None, P(p2.t), B, NC, M, HW, stream())
    lib.call("kd_argmax_confusion", P(z), P(y), ign, P(c2.t), None, B, NC, M, HW, stream())
    lib.call("kd_argmax_confusion", P(z), None, ign, P(c3.t), P(pred.t), B, NC, M, HW, stream())
    torch.cuda.synchronize()
    assert torch.equal(p2.t.view(B, HW), wp) and torch.equal(pred.t.view(B, HW), wp), what
    assert torch.equal(c2.t.view(M, M), wc), what
    assert bool((c3.t == 5).all()), f"no target: the matrix stays as it was {what}"
    for bf in (p2, c2, c3, pred):
        bf.guard_ok("metric output")


@pytest.mark.parametrize("size", ["few", "partial_block", "cap+1"])
@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("NC", [1, 2, 3, 4])
def test_argmax_confusion(NC, M, size):
    _metric_run(size, NC, M, ign=-1 if (NC + M) % 2 else 255)


@pytest.mark.parametrize("size,NC,M", [("cap-1", 2, 2), ("cap", 3, 2), ("ragged", 3, 3), ("ragged", 4, 2), ("bench", 2, 2), ("bench", 3, 2)])
def test_argmax_confusion_ladder(size, NC, M):
    _metric_run(size, NC, M)


def test_argmax_confusion_x4_head_count():
    _big()
    _metric_run(R.SEG_X4, 3, 2)


def test_argmax_confusion_refuses_bad_width():
    from kdrt.lib import KDError
    from kdrt.losses import confusion
    lib, P, stream = _lib()
    z, y = R.confusion_inputs(2, 3, 50, 1, "cuda")
    conf, pred = IBuf(16), IBuf(100)
    for M in (0, 5, -1):
        with pytest.raises(KDError):
            lib.call("kd_argmax_confusion", P(z), P(y), -1, P(conf.t), P(pred.t), 2, 3, M, 50, stream())
    torch.cuda.synchronize()
    assert bool((conf.buf == ISENT).all()) and bool((pred.buf == ISENT).all())
    z4, y4 = z.view(2, 3, 10, 5), y.view(2, 10, 5)
    for out in (torch.zeros(3, 3, dtype=torch.int64, device="cuda"), torch.zeros(2, 2, dtype=torch.int32, device="cuda"),
                torch.zeros(2, 2, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int64, device="cuda")[:, ::2]):
        with pytest.raises(KDError):
            confusion(z4, y4, num_classes=2, out=out)


def test_segmentation_metrics_two_classes_on_three_class_logits():
    """What Trainer.validate does for the 3-class model: SegmentationMetrics(num_classes=2) fed 3-class logits"""
    import kd_oracle as O
    from src.training.trainer import SegmentationMetrics
    met = SegmentationMetrics(num_classes=2)
    want = torch.zeros(2, 2, dtype=torch.int64)
    g = torch.Generator().manual_seed(31)
    for _ in range(2):
        z = torch.randn(3, 3, 17, 23, generator=g)
        y = torch.randint(-1, 3, (3, 17, 23), generator=g)
        met.update(z.cuda(), y.cuda())
        want += O.confusion_matrix(z, y, 2)
    out = met.compute()
    assert np.array_equal(met.confusion, want.numpy()), (met.confusion.tolist(), want.tolist())
    assert abs(out["miou"] - O.miou_from_confusion(want)[1]) < 1e-12


# ---- AdamW ----------------------------------------------------------------------------------------------------------------

def _param_counts():
    """the flat-buffer lengths of the three published models, padded as FlatParams pads them"""
    from _gpu_util import FUSIONS, build_product
    from kdrt.optim import FlatParams
    return sorted(FlatParams(build_product(f, 16).parameters()).numel for f in FUSIONS)


def _adamw_ref(p0, g, m0, v0, lr, wd, bc1, bc2s, ginv):
    return R.adamw_step(p0.double(), g.double(), m0.double(), v0.double(), R.f32(lr), R.f32(B1), R.f32(B2), R.f32(EPS), R.f32(wd),
                        bc1, bc2s, R.f32(ginv))


def _adamw_run(n, ginv, wd):
    lib, P, stream = _lib()
    p0, g0, m0, v0 = R.adamw_inputs(n, n % 983, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    state = Buf(4)
    state.t.copy_(torch.tensor([1e-3, 37.0, float("nan"), float("nan")]))      # a resumed run: step 37 done, corrections stale
    host = [R.f32(1e-3), 37.0, 0.0, 0.0]
    gen = torch.Generator(device="cuda").manual_seed(n)
    what = f"[n={n} ginv={ginv} wd={wd}]"
    for k in range(5):
        if k == 2:                                               # a scheduler step: the learning rate is rewritten on the device
            state.t[0:1].fill_(4e-4)
            host[0] = R.f32(4e-4)
        g = g0 * (torch.rand(n, generator=gen, device="cuda") * 2)
        before = (p.clone(), m.clone(), v.clone())               # the GPU's own state: errors do not compound
        if k == 4:                                               # the host-step form from the same state, for the last step
            (ph, phb), (mh, mhb), (vh, vhb) = _guarded(p), _guarded(m), _guarded(v)
        lib.call("kd_adamw_step_dev", P(p), P(g), P(m), P(v), n, P(state.t), B1, B2, EPS, wd, ginv, stream())
        torch.cuda.synchronize()
        host, herr = R.adamw_tick(host, R.f32(B1), R.f32(B2))
        st = state.t.double().cpu()
        for i in range(4):
            assert abs(st[i].item() - host[i]) <= herr[i] + (R.U * host[0] if i == 0 else 0), (what, k, i, st[i].item(), host[i])
        ref = _adamw_ref(*before[:1], g, *before[1:], st[0].item(), wd, st[2].item(), st[3].item(), ginv)
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _chk(f"adamw_step_dev.{nm}", got, ref[nm], f"{what} step {k}")
    lib.call("kd_adamw_step", P(ph), P(g), P(mh), P(vh), n, R.f32(4e-4), B1, B2, EPS, wd, 42, ginv, stream())
    torch.cuda.synchronize()
    bc1, bc2s = R.bias_corrections(R.f32(B1), R.f32(B2), 42)
    ref = _adamw_ref(*before[:1], g, *before[1:], 4e-4, wd, bc1, bc2s, ginv)
    for nm, got in (("p", ph), ("m", mh), ("v", vh)):
        _chk(f"adamw_step.{nm}", got, ref[nm], what)
    same = torch.equal(ph, p) and torch.equal(mh, m) and torch.equal(vh, v)
    print(f"kd_adamw_step(step=42) vs kd_adamw_step_dev {what}: {'bit-identical' if same else 'differs in the last bits'}")
    for nm, bf in (("p", pb), ("m", mb), ("v", vb), ("p", phb), ("m", mhb), ("v", vhb)):
        _guard_ok(bf, n, nm)
    state.guard_ok("state")


@pytest.mark.parametrize("ginv,wd", [(1.0, 0.0), (0.125, 1e-3)], ids=["plain", "ginv8_wd"])
@pytest.mark.parametrize("size", list(R.ADAMW_LADDER))
def test_adamw_ladder(size, ginv, wd):
    _adamw_run(R.ADAMW_LADDER[size], ginv, wd)


@pytest.mark.parametrize("ginv,wd", [(1.0, 1e-3), (0.125, 0.0)], ids=["wd", "ginv8"])
def test_adamw_published_parameter_counts(ginv, wd):
    counts = _param_counts()
    print("flat parameter counts:", counts)
    assert len(counts) == 3 and all(c % 4 == 0 and c > 2048 * 256 - 40000 for c in counts)
    for n in counts:
        _adamw_run(n, ginv, wd)


def test_adamw_dev_graph_replay():
    """a captured graph of the single kd_adamw_step_dev call (one stream, no branches) replayed three times: the step count
    and the bias corrections advance on the device"""
    lib, P, stream = _lib()
    n, wd, ginv = R.ADAMW_LADDER["cap+1"], 1e-3, 1.0
    p0, g0, m0, v0 = R.adamw_inputs(n, 77, "cuda")
    (p, pb), (m, mb), (v, vb) = _guarded(p0), _guarded(m0), _guarded(v0)
    g = g0.clone()
    state = torch.tensor([1e-3, 37.0, 0.0, 0.0], device="cuda")
    w = [t.clone() for t in (p0, g0, m0, v0, state)]             # the kernels have run once before the capture
    lib.call("kd_adamw_step_dev", P(w[0]), P(w[1]), P(w[2]), P(w[3]), n, P(w[4]), B1, B2, EPS, wd, ginv, stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.call("kd_adamw_step_dev", P(p), P(g), P(m), P(v), n, P(state), B1, B2, EPS, wd, ginv, stream())
    torch.cuda.synchronize()
    assert state[1].item() == 37.0 and torch.equal(p, p0), "capture must not execute"
    host = [R.f32(1e-3), 37.0, 0.0, 0.0]
    for k in range(3):
        g.copy_(g0 * (k + 0.5))
        before = (p.clone(), m.clone(), v.clone())
        graph.replay()
        torch.cuda.synchronize()
        host, herr = R.adamw_tick(host, R.f32(B1), R.f32(B2))
        st = state.double().cpu()
        assert st[1].item() == 38.0 + k
        assert abs(st[2].item() - host[2]) <= herr[2] and abs(st[3].item() - host[3]) <= herr[3]
        ref = _adamw_ref(before[0], g, before[1], before[2], 1e-3, wd, st[2].item(), st[3].item(), ginv)
        for nm, got in (("p", p), ("m", m), ("v", v)):
            _chk(f"adamw_step_dev.{nm}", got, ref[nm], f"[graph replay {k}]")
    for nm, bf in (("p", pb), ("m", mb), ("v", vb)):
        _guard_ok(bf, n, nm)


def test_fused_adamw_resumes_a_torch_adamw_state():
    """FusedAdamW.load_state_dict of a torch.optim.AdamW state saved at step 3, then two steps, against torch's own steps 4
    and 5 in float64.  Both sides get hyper-parameters that are fp32 values, and torch's state is set to the GPU's fp32 state
    before each step, so errors do not compound; what remains between them is the rounding of the two bias corrections to
    fp32, two more operations on the update."""
    from kdrt.optim import FusedAdamW
    lr, wd = R.f32(2e-3), R.f32(1e-3)
    hp = dict(lr=lr, betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS), weight_decay=wd)
    g = torch.Generator().manual_seed(41)
    shapes = [(37, 5), (7,), (300, 9), (1,)]
    tq = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    topt = torch.optim.AdamW(tq, **hp)
    grad = lambda: [torch.randn(*s, generator=g).double() * 10.0 ** float(torch.randint(-6, 2, (1,), generator=g)) for s in shapes]
    for _ in range(3):
        for q, gr in zip(tq, grad()):
            q.grad = gr
        topt.step()

    def to_fp32_values():
        for q in tq:
            q.data = q.data.float().double()
            for k in ("exp_avg", "exp_avg_sq"):
                topt.state[q][k] = topt.state[q][k].float().double()

    to_fp32_values()                                            # the checkpoint holds fp32 values: both sides start from the same state
    gq = [torch.nn.Parameter(q.detach().float().cuda()) for q in tq]
    opt = FusedAdamW(gq, **hp)
    opt.load_state_dict(topt.state_dict())
    assert opt._step == 3
    for step in (4, 5):
        grads = grad()
        pre = [(q.detach().clone(), topt.state[q]["exp_avg"].clone(), topt.state[q]["exp_avg_sq"].clone()) for q in tq]
        opt.zero_grad()
        for q, t, gr in zip(gq, tq, grads):
            q.grad.copy_(gr.float())
            t.grad = gr.float().double()
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        bc1, bc2s = R.bias_corrections(R.f32(B1), R.f32(B2), step)
        for i, (q, t, gr, (p0, m0, v0)) in enumerate(zip(gq, tq, grads, pre)):
            err = R.adamw_step(p0, gr.float().double(), m0, v0, lr, *hp["betas"], hp["eps"], wd, bc1, bc2s, 1.0)
            st, gst = topt.state[t], opt.state[q]
            e_p = err["p"][1] + R.C_BOUND * 2 * R.U * ((t.detach() - p0).abs() + lr * wd * p0.abs())
            _chk("FusedAdamW.p", q.detach(), (t.detach().cuda(), e_p.cuda()), f"[tensor {i} step {step}]")
            _chk("FusedAdamW.exp_avg", gst["exp_avg"], (st["exp_avg"].cuda(), err["m"][1].cuda()), f"[tensor {i} step {step}]")
            _chk("FusedAdamW.exp_avg_sq", gst["exp_avg_sq"], (st["exp_avg_sq"].cuda(), err["v"][1].cuda()), f"[tensor {i} step {step}]")
            assert float(gst["step"]) == step
            t.data = q.detach().double().cpu()                   # torch continues from the GPU's state
            st["exp_avg"], st["exp_avg_sq"] = gst["exp_avg"].double().cpu().clone(), gst["exp_avg_sq"].double().cpu().clone()
    assert opt.dev_state[1].item() == 5.0
