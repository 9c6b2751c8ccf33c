"""The kernels of the 5-to-16-class path called directly through the C ABI: kd_seg_loss_fwd_bwd and kd_cls_conv_fwd / _bwd in their
class buckets of 8 and 16, kd_argmax_confusion16 and kd_semantic_remap_table.  Loss and classifier are compared with the float64
references of tests/_fp64_loss_ref.py and tests/_fp64_tail_ref.py under the bounds tests/test_gpu_loss_kernels.py and
tests/test_gpu_tail_kernels.py form (the same helpers, no new tolerance; tests/test_multiclass_ref_host.py checks the references at
these class counts); argmax, confusion matrix and remap are exact.  Class counts 5, 8, 9 and 16 sit on both edges of the two new
buckets.  Every output starts as NaN or a sentinel and carries a guard tail."""
import numpy as np
import pytest
import torch

import _fp64_loss_ref as L
import _fp64_multiclass_ref as MC
import _fp64_tail_ref as R
import test_gpu_loss_kernels as LK
import test_gpu_tail_kernels as TK
from test_gpu_tail_kernels import SENT, Buf, _check

pytestmark = pytest.mark.gpu

NCS = (5, 8, 9, 16)
SIZES = ("few", "partial_block", "cap+1")


def _lib():
    from kdrt.lib import KDError, lib
    from kdrt.ops import P, stream
    return lib, P, stream, KDError


# ---- segmentation loss --------------------------------------------------------------------------------------------------------

CROSS = [(nc, w, t, g) for nc in NCS for w in (True, False) for t in (True, False) for g in (True, False)]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("i", range(len(CROSS)), ids=lambda i: "NC%d-w%d-t%d-g%d" % CROSS[i])
def test_seg_loss(size, i):
    LK._seg_run(size, *CROSS[i], variant=i + i // 4 + SIZES.index(size))


@pytest.mark.parametrize("size", ["partial_block", "cap+1"])
def test_seg_loss_16_classes_all_ignored(size):
    """losses[0] is NaN like torch's, losses[2] == 0, dzs is the KL part alone and finite"""
    LK._seg_run(size, 16, True, True, True, variant=3, mode="all_ignored")


def test_seg_loss_16_classes_teacher_probabilities_underflow():
    """logits of scale 60 at T = 1: teacher probabilities underflow to 0 (the `pt > 0` guard of the KL sum)"""
    zs, zt = LK._seg_run("cap+1", 16, True, True, True, variant=1, scale=60.0)
    assert bool((torch.softmax(zt, 1) == 0).any())


@pytest.mark.parametrize("NC", [9, 16])
def test_seg_loss_student_equal_to_teacher(NC):
    """zt == zs: both softmaxes run the same operations on the same values, so the KL value and the KL term of the gradient are
    exactly 0 -- the gradient has the bits of the call without a teacher"""
    lib, P, stream, _ = _lib()
    B, HW = L.SEG_LADDER["partial_block"]
    zs, _, y, cw = L.seg_inputs(B, NC, HW, 77 + NC, "cuda", -1, 3.0, True, False)
    nbytes = lib.kd_seg_loss_ws_bytes(B * HW)
    out = []
    for zt in (zs.clone(), None):
        ws, losses, dzs = Buf(nbytes // 4), Buf(3), Buf(B, NC, HW)
        lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), -1, 4.0, 0.7, 1.0, None, P(losses.t), P(dzs.t), B, NC, HW, P(ws.t), nbytes,
                 stream())
        torch.cuda.synchronize()
        out.append((losses.t.clone(), dzs.t.clone()))
        dzs.guard_ok("dzs"); losses.guard_ok("losses"); ws.guard_ok("ws")
    (l_t, g_t), (l_0, g_0) = out
    assert l_t[1].item() == 0.0 and l_0[1].item() == 0.0
    assert torch.equal(l_t.view(torch.int32), l_0.view(torch.int32))
    assert bool(torch.isfinite(g_t).all()) and g_t.abs().max() > 0 and torch.equal(g_t.view(torch.int32), g_0.view(torch.int32))


@pytest.mark.parametrize("NC", [17, 1, 64])
def test_seg_loss_refuses_other_class_counts_and_writes_nothing(NC):
    lib, P, stream, KDError = _lib()
    B, HW = 2, 61
    zs, zt = torch.randn(B, NC, HW, device="cuda"), torch.randn(B, NC, HW, device="cuda")
    y = torch.zeros(B, HW, dtype=torch.int64, device="cuda")
    nbytes = lib.kd_seg_loss_ws_bytes(B * HW)
    bufs = [torch.full((n,), SENT, device="cuda") for n in (nbytes // 4, 4, B * NC * HW)]
    with pytest.raises(KDError, match=r"2\.\.16"):
        lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), None, -1, 4.0, 1.0, 1.0, None, P(bufs[1]), P(bufs[2]), B, NC, HW, P(bufs[0]), nbytes,
                 stream())
    torch.cuda.synchronize()
    assert all(bool((b == SENT).all()) for b in bufs)


def test_seg_loss_function_takes_16_classes_and_region_lovasz_refuse():
    """the Python entry points: seg_loss runs 16 classes; RegionLoss and LovaszLoss name their limit of 4"""
    from kdrt.lib import KDError
    from kdrt.losses import LovaszLoss, RegionLoss, lovasz_seg_loss, region_seg_loss, seg_loss
    z = torch.randn(2, 16, 8, 8, device="cuda", requires_grad=True)
    y = torch.randint(0, 16, (2, 8, 8), device="cuda")
    cw = torch.rand(16, device="cuda") + 0.5
    ce, _ = seg_loss(z, y, cw)
    ce.backward()
    want = torch.nn.functional.cross_entropy(z.detach().double(), y, weight=cw.double())
    assert abs(ce.item() - want.item()) < 1e-5 and bool(torch.isfinite(z.grad).all())
    with pytest.raises(KDError, match="at most 4 classes"):
        region_seg_loss(z, y, RegionLoss())
    with pytest.raises(KDError, match="at most 4 classes"):
        lovasz_seg_loss(z, y, LovaszLoss())


# ---- 1x1 classifier -------------------------------------------------------------------------------------------------------------

CLS_SHAPES = [(32, 5), (32, 16), (64, 9), (4, 8)]
CLS_ROWS = [1000, 20011]            # a partial last block of the forward and of every backward layout; 20011 (a prime: one image)
                                    # is a ragged second iteration at Cin = 64 (16 row slots x 1024 blocks)


def _dwb_floats(Cin, NC):
    return NC * Cin + 4 * ((NC + 3) // 4)


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("M", CLS_ROWS)
@pytest.mark.parametrize("Cin,NC", CLS_SHAPES)
def test_cls_conv_fwd(M, Cin, NC, deferred):
    lib, P, stream, _ = _lib()
    _, x, sc, sh, _, _, w, b = TK._cls_inputs(M, Cin, NC, M + Cin + NC)
    B, _, _ = TK._bhw(M)
    if not deferred:
        sc = sh = None
    logits = Buf(B, NC, M // B)
    lib.call("kd_cls_conv_fwd", P(x), P(sc), P(sh), R.RELU, P(w), P(b), P(logits.t), M, M // B, Cin, NC, stream())
    torch.cuda.synchronize()
    _check("logits", logits.t, R.cls_conv_fwd(*TK._d(x, sc, sh), R.RELU, *TK._d(w, b), B)["logits"])
    logits.guard_ok("logits")


@pytest.mark.parametrize("tail", [False, True], ids=["all_rows", "tail_rows"])
@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("M", CLS_ROWS)
@pytest.mark.parametrize("Cin,NC", CLS_SHAPES)
def test_cls_conv_bwd(M, Cin, NC, deferred, tail):
    lib, P, stream, _ = _lib()
    g, x, sc, sh, mean, inv, w, _ = TK._cls_inputs(M, Cin, NC, M + Cin + NC + 1)
    B, _, _ = TK._bhw(M)
    slots, grid, iters = TK._layout(M, Cin, 1024)
    dl = TK._rnd(g, M, NC)
    if tail:
        dl = dl * TK._tail_rows(M, slots, grid, iters)[:, None]
    dlog = R.nchw_from_rows(dl, B)
    if not deferred:
        sc = sh = mean = inv = None
    rows = lib.kd_cls_conv_bwd_stat_rows(M, Cin)
    nbytes = lib.kd_cls_conv_bwd_ws_bytes(M, Cin, NC)
    nf = _dwb_floats(Cin, NC)
    assert lib.kd_cls_conv_dwb_floats(Cin, NC) == nf and rows == grid and nbytes == grid * nf * 4
    ws, gx, part, dwb = Buf(nbytes // 4), Buf(M, Cin), Buf(rows, 2, Cin), Buf(nf)
    lib.call("kd_cls_conv_bwd", P(dlog), P(x), P(sc), P(sh), R.RELU, P(mean), P(inv), P(w), P(gx.t), P(part.t) if deferred else None,
             P(dwb.t), M, M // B, Cin, NC, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ref = R.cls_conv_bwd(*TK._d(dlog, x, sc, sh), R.RELU, *TK._d(mean, inv, w), n_red=iters + slots + grid + R.SLAB_SPLIT,
                         n_part=iters + slots)
    _check("gx", gx.t, ref["gx"])
    _check("dW", dwb.t[:NC * Cin], ref["dw"])
    _check("db", dwb.t[NC * Cin:NC * Cin + NC], ref["db"])
    assert bool((dwb.t[NC * Cin + NC:] == 0).all()), "the db padding words are written as 0"
    assert bool((ws.t.view(grid, nf)[:, NC * Cin + NC:] == 0).all()), "the padding words of every slab row are written as 0"
    if deferred:
        s = part.t.double().sum(0)
        _check("sum g", s[0], ref["s1"])
        _check("sum g*xhat", s[1], ref["s2"])
    for n, b_ in (("ws", ws), ("gx", gx), ("partial", part), ("dwb", dwb)):
        b_.guard_ok(n)


def test_dwb_layout_of_up_to_four_classes_is_unchanged():
    lib = _lib()[0]
    for Cin in (4, 32, 64):
        for NC in (1, 2, 3, 4):
            assert lib.kd_cls_conv_dwb_floats(Cin, NC) == NC * Cin + 4
    assert lib.kd_cls_conv_dwb_floats(32, 5) == 5 * 32 + 8 and lib.kd_cls_conv_dwb_floats(32, 16) == 16 * 32 + 16


def test_cls_conv_refuses_17_classes_and_writes_nothing():
    lib, P, stream, KDError = _lib()
    M, Cin, NC = 64, 32, 17
    x, w, b, dlog = (torch.randn(*s, device="cuda") for s in ((M, Cin), (NC, Cin), (NC,), (1, NC, M)))
    out = [torch.full((n,), SENT, device="cuda") for n in (NC * M, M * Cin, 4096, 4096)]
    with pytest.raises(KDError, match=r"NC 1\.\.16"):
        lib.call("kd_cls_conv_fwd", P(x), None, None, 0, P(w), P(b), P(out[0]), M, M, Cin, NC, stream())
    with pytest.raises(KDError, match=r"NC 1\.\.16"):
        lib.call("kd_cls_conv_bwd", P(dlog), P(x), None, None, 0, None, None, P(w), P(out[1]), None, P(out[2]), M, M, Cin, NC, P(out[3]),
                 4096 * 4, stream())
    torch.cuda.synchronize()
    assert all(bool((o == SENT).all()) for o in out)


# ---- argmax + confusion matrix, 16 wide ------------------------------------------------------------------------------------------

def _conf_inputs(B, NC, HW, seed, ign, hi=18):
    """logits on a coarse grid (many exact ties) with +-inf and signed zeros; labels -2 .. hi-1 and ignore_index"""
    z, _ = L.confusion_inputs(B, NC, HW, seed, "cuda", ign)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    y = torch.randint(-2, hi, (B, HW), generator=g, device="cuda")
    y = torch.where(torch.rand(B, HW, generator=g, device="cuda") < 0.07, torch.full_like(y, ign), y)
    return z, y


def _conf16(z, y, ign, M, conf, pred):
    lib, P, stream, _ = _lib()
    B, NC, HW = z.shape
    lib.call("kd_argmax_confusion16", P(z), P(y), ign, P(conf), P(pred), B, NC, M, HW, stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("ign", [-1, 255])
@pytest.mark.parametrize("NC,M", [(5, 5), (16, 16), (16, 3), (3, 16), (1, 8)])
def test_argmax_confusion16(NC, M, ign):
    B, HW = 3, 4099                                      # 49 blocks, the last one partial, frame boundaries inside a block
    conf = LK.IBuf(M * M)
    conf.t.zero_()
    want = torch.zeros(M, M, dtype=torch.int64, device="cuda")
    for call in range(2):                                # the second call accumulates into the counts of the first
        z, y = _conf_inputs(B, NC, HW, 100 * NC + M + call, ign)
        pred = LK.IBuf(B * HW)
        _conf16(z, y, ign, M, conf.t, pred.t)
        rp, rc = L.confusion(z, y, M, ign)
        want += rc
        assert torch.equal(pred.t.view(B, HW), rp), "argmax: the lowest index of the maximum"
        assert torch.equal(conf.t.view(M, M), want)
        pred.guard_ok("pred"); conf.guard_ok("conf")
    assert int(want.sum()) > 0 and (NC == 1 or int((rp > 0).sum()) > 0)
    # exact ties: the first of the equal maxima wins
    tie = (z == z.amax(1, keepdim=True)).sum(1) > 1
    assert NC == 1 or bool(tie.any())
    first = (z == z.amax(1, keepdim=True)).float().argmax(1)
    assert torch.equal(pred.t.view(B, HW), first)
    # the pred-only and the conf-only form
    p2 = LK.IBuf(B * HW)
    _conf16(z, None, ign, M, None, p2.t)
    assert torch.equal(p2.t, pred.t)
    c2 = LK.IBuf(M * M)
    c2.t.zero_()
    _conf16(z, y, ign, M, c2.t, None)
    assert torch.equal(c2.t.view(M, M), rc)
    p2.guard_ok("pred"); c2.guard_ok("conf")


def test_argmax_confusion16_handles_nan_like_the_4_wide_entry():
    lib, P, stream, _ = _lib()
    B, NC, HW, M = 2, 4, 1031, 4
    z, y = _conf_inputs(B, NC, HW, 5, -1, hi=6)
    r = torch.rand(B, NC, HW, device="cuda")
    z = torch.where(r < 0.15, torch.full_like(z, float("nan")), z)
    res = []
    for entry in ("kd_argmax_confusion", "kd_argmax_confusion16"):
        conf, pred = LK.IBuf(M * M), LK.IBuf(B * HW)
        conf.t.zero_()
        lib.call(entry, P(z), P(y), -1, P(conf.t), P(pred.t), B, NC, M, HW, stream())
        torch.cuda.synchronize()
        res.append((conf.t.clone(), pred.t.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert bool(torch.isnan(z[:, 0]).any())


@pytest.mark.parametrize("NC,M", [(16, 17), (17, 16), (4, 0)])
def test_argmax_confusion16_refuses_and_leaves_the_buffers(NC, M):
    lib, P, stream, KDError = _lib()
    z = torch.randn(2, NC, 300, device="cuda")
    y = torch.zeros(2, 300, dtype=torch.int64, device="cuda")
    conf, pred = LK.IBuf(17 * 17), LK.IBuf(600)
    with pytest.raises(KDError, match=r"1\.\.16"):
        lib.call("kd_argmax_confusion16", P(z), P(y), -1, P(conf.t), P(pred.t), 2, NC, M, 300, stream())
    torch.cuda.synchronize()
    assert bool((conf.buf == LK.ISENT).all()) and bool((pred.buf == LK.ISENT).all())


def test_confusion_function_dispatch():
    """kdrt.losses.confusion: the 4-wide entry up to 4 classes and a 4 x 4 matrix, the 16-wide one beyond; M = 17 is a KDError"""
    from kdrt.lib import KDError
    from kdrt.losses import confusion
    for NC, M in ((2, 2), (3, 2), (4, 4), (3, 5), (8, 8), (16, 2), (16, 16)):
        z, y = _conf_inputs(2, NC, 35 * 37, NC + M, -1)
        conf, pred = confusion(z.view(2, NC, 35, 37), y.view(2, 35, 37), M)
        rp, rc = L.confusion(z, y, M, -1)
        assert torch.equal(conf, rc) and torch.equal(pred.view(2, -1), rp), (NC, M)
    with pytest.raises(KDError):
        confusion(z.view(2, 16, 35, 37), y.view(2, 35, 37), 17)


# ---- table remap ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 4001, 8192 * 256 + 3])
def test_semantic_remap_table(n):
    lib, P, stream, _ = _lib()
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    table = torch.randint(0, 16, (43,), generator=g, device="cuda")
    raw = torch.randint(-5, 60, (n,), generator=g, device="cuda")
    edge = torch.tensor([42, 43, -1, 0, -(2 ** 40), 2 ** 40, 2 ** 32 + 3], device="cuda")[:n]
    raw[:edge.numel()] = edge
    out = LK.IBuf(n)
    lib.call("kd_semantic_remap_table", P(raw), n, P(table), 43, P(out.t), stream())
    torch.cuda.synchronize()
    r, t = raw.cpu().numpy(), table.cpu().numpy()
    want = np.where((r >= 0) & (r < 43), t[np.clip(r, 0, 42)], 0)
    assert np.array_equal(out.t.cpu().numpy(), want)
    assert torch.equal(out.t, MC.remap_table(raw, table))
    out.guard_ok("out")


def test_remap_semantic_table_function():
    from src.data_loading.pandaset_dataset import class_map_table, remap_semantic_table
    table = class_map_table({7: 1, 13: 2, 30: 15})
    raw = np.array([[7, 13, 30, 31], [-1, 0, 12, 7]], np.int64)
    got = remap_semantic_table(raw, table)
    assert isinstance(got, np.ndarray) and np.array_equal(got, [[1, 2, 15, 0], [0, 0, 0, 1]])
    got = remap_semantic_table(torch.from_numpy(raw), table)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), [[1, 2, 15, 0], [0, 0, 0, 1]])
