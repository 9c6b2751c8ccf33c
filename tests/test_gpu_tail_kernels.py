"""The HIP kernels from the fusion output to the logits and the FPN / LiDAR-map resize (csrc/kd_fuse.hip, csrc/kd_head.hip),
called directly through the C ABI and compared element-wise with a float64 evaluation of the same operation on the same fp32
inputs (tests/_fp64_tail_ref.py, plain torch on the GPU), within C_BOUND * n_seq * 2^-24 * sum|t_i| per output.

Row counts are derived from each kernel's own launch layout: far fewer rows than slots, a partial block, cap*slots - 1,
cap*slots, cap*slots + 1 (the first multi-iteration case), a ragged last iteration, and the benchmarked count.  Every
reduction runs a second time with the upstream gradient nonzero only in the tail rows (the last ragged iteration, the last
block, row 0, row M-1), so a dropped, duplicated or misindexed tail row fails by O(1) instead of hiding under a norm.  Every
output, slab and partial buffer starts as NaN (an unwritten element fails) and carries a sentinel guard tail (an element
written past the end fails)."""
import math

import pytest
import torch

import _fp64_tail_ref as R

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, -1.25e30
NAN = float("nan")
BIG_HBM = 100 * 2 ** 30


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _big():
    if torch.cuda.get_device_properties(0).total_memory < BIG_HBM:
        pytest.skip("needs an MI355X-class HBM")


class Buf:
    """a NaN-filled output of n floats followed by a guard of sentinels"""

    def __init__(self, *shape):
        n = math.prod(shape)
        self.n = n
        self.buf = torch.full((n + GUARD,), NAN, device="cuda")
        self.buf[n:] = SENT
        self.t = self.buf[:n].view(*shape)

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == SENT).all()), f"{what}: written past its end"


def _rnd(g, *s):
    return torch.randn(*s, generator=g, device="cuda")


def _bn(g, C):
    """(sc, sh, mean, invstd) as a training BatchNorm hands them on: positive scale, small shift"""
    return _rnd(g, C).abs() + 0.5, _rnd(g, C) * 0.2, _rnd(g, C) * 0.1, _rnd(g, C).abs() + 0.5


def _d(*ts):
    return [t.double() if torch.is_tensor(t) else t for t in ts]


def _check(what, got, ref):
    val, err = ref
    got = got.double().reshape(val.shape)
    assert not bool(torch.isnan(got).any()), f"{what}: {int(torch.isnan(got).sum())} elements never written"
    d = (got - val).abs()
    bad = d > err
    if bool(bad.any()):
        i = int(torch.nonzero(bad.reshape(-1))[0])
        r = (d / err.clamp_min(1e-300)).max().item()
        pytest.fail(f"{what}: {int(bad.sum())} of {val.numel()} outside the bound (worst {r:.3g}x); first at flat index {i}: "
                    f"got {got.reshape(-1)[i].item():.9g}, float64 {val.reshape(-1)[i].item():.9g}, bound {err.reshape(-1)[i].item():.3g}")


def _layout(rows, C, cap):
    """mirror of kd_cg_layout: (slots, grid, iterations per slot)"""
    slots = max(1, 256 // (C // 4))
    grid = max(1, min(-(-rows // slots), cap))
    return slots, grid, -(-rows // (grid * slots))


def _ladder(slots, cap):
    full = cap * slots
    return {"few": max(1, slots // 3), "partial_block": 3 * slots + slots // 2 + 1, "full-1": full - 1, "full": full,
            "full+1": full + 1, "ragged": 2 * full + full // 3 + 5}


def _tail_rows(rows, slots, grid, iters):
    """the rows a grid-stride reduction handles last or at its edges: the last (ragged) iteration, the last block, 0, M-1"""
    m = torch.arange(rows, device="cuda")
    sel = (m >= (iters - 1) * grid * slots) | ((m // slots) % grid == grid - 1)
    sel[0] = sel[-1] = True
    return sel


def _bhw(rows):
    """rows = B * H * W with small B and non-square maps (a prime count gives a 1-row map)"""
    for B in (3, 5, 2, 7, 1):
        if rows % B == 0:
            n = rows // B
            H = max(h for h in range(1, int(math.isqrt(n)) + 1) if n % h == 0)
            return B, H, n // H
    raise AssertionError


# ---- weighted fusion tail ----------------------------------------------------------------------------------------------

def _wf_inputs(M, C, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    cat, hraw = _rnd(g, M, 2 * C), _rnd(g, M, C)
    sc, sh = _rnd(g, 2 * C).abs() + 0.5, _rnd(g, 2 * C) * 0.2
    return g, cat, sc, sh, hraw, _rnd(g, 2, C) * 0.3, _rnd(g, 2) * 0.1


WF_FWD = [(r, 128) for r in _ladder(8, 4096).values()] + [(4099, 32), (65537, 64), (16389, 256)]
WF_BWD = [(r, 128) for r in _ladder(8, 1024).values()] + [(8 * 1024 * 4 + 3, 32), (16385, 64), (4097, 256)]


@pytest.mark.parametrize("M,C", WF_FWD + [(256 * 64 * 64, 128)], ids=lambda v: str(v))
def test_weighted_fuse_fwd(M, C):
    if M > 2 ** 20 - 1:
        _big()
    lib, P, stream = _lib()
    _, cat, sc, sh, hraw, w2, b2 = _wf_inputs(M, C, M % 1000 + C)
    out, wts = Buf(M, C), Buf(M, 2)
    lib.call("kd_weighted_fuse_fwd", P(cat), P(sc), P(sh), P(hraw), P(w2), P(b2), P(out.t), P(wts.t), M, C, stream())
    torch.cuda.synchronize()
    ref = R.weighted_fuse_fwd(*_d(cat, sc, sh, hraw, w2, b2))
    _check("out", out.t, ref["out"])
    _check("wts", wts.t, ref["wts"])
    out.guard_ok("out"); wts.guard_ok("wts")


@pytest.mark.parametrize("tail", [False, True], ids=["all_rows", "tail_rows"])
@pytest.mark.parametrize("M,C", WF_BWD + [(256 * 64 * 64, 128)], ids=lambda v: str(v))
def test_weighted_fuse_bwd(M, C, tail):
    if M > 2 ** 20 - 1:
        _big()
    lib, P, stream = _lib()
    g, cat, sc, sh, hraw, w2, _ = _wf_inputs(M, C, M % 1000 + C + 1)
    wts = torch.softmax(_rnd(g, M, 2), 1)
    dout = _rnd(g, M, C)
    slots, grid, iters = _layout(M, C, 1024)
    if tail:
        dout = dout * _tail_rows(M, slots, grid, iters)[:, None]
    nbytes = lib.kd_weighted_fuse_bwd_ws_bytes(M, C)
    assert nbytes == grid * (3 * C + 4) * 4
    ws, dcat, gh, dpar = Buf(nbytes // 4), Buf(M, 2 * C), Buf(M, C), Buf(3 * C + 4)
    lib.call("kd_weighted_fuse_bwd", P(dout), P(cat), P(sc), P(sh), P(hraw), P(w2), P(wts), P(dcat.t), P(gh.t), P(dpar.t), M, C,
             P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ref = R.weighted_fuse_bwd(*_d(dout, cat, sc, sh, hraw, w2, wts), n_red=iters + slots + grid + R.SLAB_SPLIT)
    _check("dcat", dcat.t, ref["dcat"])
    _check("gh", gh.t, ref["gh"])
    _check("dW2", dpar.t[:2 * C], ref["dw2"])
    _check("db1", dpar.t[2 * C:3 * C], ref["db1"])
    _check("db2", dpar.t[3 * C:3 * C + 2], ref["db2"])
    assert bool((dpar.t[3 * C + 2:] == 0).all()), "dparams padding"
    for n, b in (("ws", ws), ("dcat", dcat), ("gh", gh), ("dparams", dpar)):
        b.guard_ok(n)


# ---- 1x1 classifier ------------------------------------------------------------------------------------------------------

CLS_LADDER = [(r, 32, 2) for r in _ladder(32, 1024).values()]
CLS_SHAPES = [(9000, cin, nc) for cin in (4, 32, 64) for nc in (1, 2, 3, 4)]


def _cls_inputs(M, Cin, NC, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = _rnd(g, M, Cin)
    return g, x, *_bn(g, Cin), _rnd(g, NC, Cin), _rnd(g, NC)


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("M,Cin,NC", CLS_LADDER + CLS_SHAPES + [(256 * 64 * 64, 32, 2)], ids=lambda v: str(v))
def test_cls_conv_fwd(M, Cin, NC, deferred):
    if M > 2 ** 20 - 1:
        _big()
    lib, P, stream = _lib()
    _, x, sc, sh, _, _, w, b = _cls_inputs(M, Cin, NC, M + Cin + NC)
    B, _, _ = _bhw(M)
    if not deferred:
        sc = sh = None
    logits = Buf(B, NC, M // B)
    lib.call("kd_cls_conv_fwd", P(x), P(sc), P(sh), R.RELU, P(w), P(b), P(logits.t), M, M // B, Cin, NC, stream())
    torch.cuda.synchronize()
    _check("logits", logits.t, R.cls_conv_fwd(*_d(x, sc, sh), R.RELU, *_d(w, b), B)["logits"])
    logits.guard_ok("logits")


@pytest.mark.parametrize("tail", [False, True], ids=["all_rows", "tail_rows"])
@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("M,Cin,NC", CLS_LADDER + CLS_SHAPES + [(256 * 64 * 64, 32, 2)], ids=lambda v: str(v))
def test_cls_conv_bwd(M, Cin, NC, deferred, tail):
    if M > 2 ** 20 - 1:
        _big()
    lib, P, stream = _lib()
    g, x, sc, sh, mean, inv, w, _ = _cls_inputs(M, Cin, NC, M + Cin + NC + 1)
    B, _, _ = _bhw(M)
    slots, grid, iters = _layout(M, Cin, 1024)
    dl = _rnd(g, M, NC)
    if tail:
        dl = dl * _tail_rows(M, slots, grid, iters)[:, None]
    dlog = R.nchw_from_rows(dl, B)
    if not deferred:
        sc = sh = mean = inv = None
    rows = lib.kd_cls_conv_bwd_stat_rows(M, Cin)
    nbytes = lib.kd_cls_conv_bwd_ws_bytes(M, Cin, NC)
    assert rows == grid and nbytes == grid * (NC * Cin + 4) * 4
    ws, gx, part, dwb = Buf(nbytes // 4), Buf(M, Cin), Buf(rows, 2, Cin), Buf(NC * Cin + 4)
    lib.call("kd_cls_conv_bwd", P(dlog), P(x), P(sc), P(sh), R.RELU, P(mean), P(inv), P(w), P(gx.t), P(part.t) if deferred else None,
             P(dwb.t), M, M // B, Cin, NC, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ref = R.cls_conv_bwd(*_d(dlog, x, sc, sh), R.RELU, *_d(mean, inv, w), n_red=iters + slots + grid + R.SLAB_SPLIT,
                         n_part=iters + slots)
    _check("gx", gx.t, ref["gx"])
    _check("dW", dwb.t[:NC * Cin], ref["dw"])
    _check("db", dwb.t[NC * Cin:NC * Cin + NC], ref["db"])
    assert bool((dwb.t[NC * Cin + NC:] == 0).all()), "dwb padding"
    if deferred:
        s = part.t.double().sum(0)
        _check("sum g", s[0], ref["s1"])
        _check("sum g*xhat", s[1], ref["s2"])
    for n, b_ in (("ws", ws), ("gx", gx), ("partial", part), ("dwb", dwb)):
        b_.guard_ok(n)


# ---- 3x3 classifier ------------------------------------------------------------------------------------------------------

def _c3_cases():
    sw = 64                            # Cin 16: 4 channel groups, 64 row slots
    rows = list(_ladder(sw, 256).values()) + [1024 * sw + 1]            # weight pass capped at 256 blocks, data pass at 1024
    cases = [(*_bhw(r), 16, 2) for r in rows]
    cases += [(2, 9, 13, cin, nc) for cin in (4, 16, 32) for nc in (1, 2, 3, 4)]
    cases += [(3, 1, 1, 4, 1), (2, 1, 37, 8, 3)]
    return cases


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("tail", [False, True], ids=["all_rows", "tail_rows"])
@pytest.mark.parametrize("B,H,W,Cin,NC", _c3_cases() + [(32, 256, 256, 16, 2)], ids=lambda v: str(v))
def test_cls3x3_fwd_bwd(B, H, W, Cin, NC, tail, deferred):
    if B * H * W > 2 ** 20:
        _big()
    lib, P, stream = _lib()
    M = B * H * W
    g = torch.Generator(device="cuda").manual_seed(M + Cin * 7 + NC)
    x = _rnd(g, B, H, W, Cin)
    sc, sh, mean, inv = _bn(g, Cin)
    if not deferred:
        sc = sh = mean = inv = None
    w, b = _rnd(g, NC, Cin, 3, 3), _rnd(g, NC)
    if not tail:
        logits = Buf(B, NC, H, W)
        lib.call("kd_cls3x3_fwd", P(x), P(sc), P(sh), R.RELU, P(w), P(b), P(logits.t), B, H, W, Cin, NC, stream())
        torch.cuda.synchronize()
        _check("logits", logits.t, R.cls3x3_fwd(*_d(x, sc, sh), R.RELU, *_d(w, b))["logits"])
        logits.guard_ok("logits")
    slots, grid_w, iters_w = _layout(M, Cin, 256)
    _, grid_d, iters_d = _layout(M, Cin, 1024)
    dlog = _rnd(g, B, NC, H, W)
    if tail:
        sel = _tail_rows(M, slots, grid_w, iters_w) | _tail_rows(M, slots, grid_d, iters_d)
        dlog = dlog * sel.view(B, 1, H, W)
    rows = lib.kd_cls3x3_bwd_stat_rows(M, Cin)
    nbytes = lib.kd_cls3x3_bwd_ws_bytes(M, Cin, NC)
    assert rows == grid_d and nbytes == grid_w * (NC * Cin * 9 + 4) * 4
    ws, gx, part, dwb = Buf(nbytes // 4), Buf(M, Cin), Buf(rows, 2, Cin), Buf(NC * Cin * 9 + 4)
    lib.call("kd_cls3x3_bwd", P(dlog), P(x), P(sc), P(sh), R.RELU, P(mean), P(inv), P(w), P(gx.t), P(part.t) if deferred else None,
             P(dwb.t), B, H, W, Cin, NC, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ref = R.cls3x3_bwd(*_d(dlog, x, sc, sh), R.RELU, *_d(mean, inv, w), n_red=iters_w + slots + grid_w + R.SLAB_SPLIT,
                       n_part=iters_d + slots)
    _check("gx", gx.t, ref["gx"])
    _check("dW", dwb.t[:NC * Cin * 9], ref["dw"])
    _check("db", dwb.t[NC * Cin * 9:NC * Cin * 9 + NC], ref["db"])
    assert bool((dwb.t[NC * Cin * 9 + NC:] == 0).all()), "dwb padding"
    if deferred:
        s = part.t.double().sum(0)
        _check("sum g", s[0], ref["s1"])
        _check("sum g*xhat", s[1], ref["s2"])
    for n, b_ in (("ws", ws), ("gx", gx), ("partial", part), ("dwb", dwb)):
        b_.guard_ok(n)


# ---- ConvTranspose2d(k4, s2, p1) col2im / im2col -----------------------------------------------------------------------

def _c2i_cases():
    full = 2048 * 16                    # Cout 64: 16 channel groups, 16 row slots; the launch cap is 2048 blocks
    cases = [(1, 1, 1, 64), (1, 3, 5, 64), (*_bhw(full // 4 - 1), 64), (*_bhw(full // 4), 64), (*_bhw(full // 4 + 1), 64),
             (*_bhw(2 * full // 4 + 977), 64)]
    cases += [(2, 7, 9, 16), (2, 5, 3, 12), (1, 4, 4, 1024), (2, 3, 2, 4)]
    return cases


@pytest.mark.parametrize("tail", [False, True], ids=["all_rows", "tail_rows"])
@pytest.mark.parametrize("B,H,W,Cout", _c2i_cases() + [(32, 64, 64, 64), (32, 128, 128, 16)], ids=lambda v: str(v))
def test_col2im_fwd(B, H, W, Cout, tail):
    if B * H * W * Cout * 16 > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = torch.Generator(device="cuda").manual_seed(B * H * W + Cout)
    npix = B * 4 * H * W
    slots, grid, iters = _layout(npix, Cout, 2048)
    col = _rnd(g, B * H * W, Cout * 16)
    if tail:
        # keep only the taps that land on a tail output pixel: out[b, 2ih-1+kh, 2iw-1+kw] += col[(b,ih,iw), co, kh, kw]
        sel = _tail_rows(npix, slots, grid, iters).view(B, 2 * H, 2 * W)
        selp = torch.nn.functional.pad(sel, (1, 1, 1, 1))
        keep = torch.zeros(B, H, W, 1, 4, 4, dtype=torch.bool, device="cuda")
        for kh in range(4):
            for kw in range(4):
                keep[:, :, :, 0, kh, kw] = selp[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2]
        col = (col.view(B, H, W, Cout, 4, 4) * keep).view(B * H * W, Cout * 16)
    rows = lib.kd_deconv_stat_rows(npix, Cout)
    assert rows == grid
    out, part = Buf(B, 2 * H, 2 * W, Cout), Buf(rows, 2, Cout)
    lib.call("kd_deconv4x4s2_col2im_fwd", P(col), P(out.t), P(part.t), B, H, W, Cout, stream())
    torch.cuda.synchronize()
    ref = R.col2im_fwd(col.double(), B, H, W, Cout, n_part=iters + slots)
    _check("out", out.t, ref["out"])
    s = part.t.double().sum(0)
    _check("sum y", s[0], ref["s1"])
    _check("sum y^2", s[1], ref["s2"])
    out.guard_ok("out"); part.guard_ok("partial")


@pytest.mark.parametrize("act", [R.RELU, 0], ids=["masked", "unmasked"])
@pytest.mark.parametrize("B,H,W,Cout", [(1, 1, 1, 4), (2, 5, 3, 12), (3, 7, 11, 64), (1, 128, 129, 64), (32, 64, 64, 64),
                                        (32, 128, 128, 16)], ids=lambda v: str(v))
def test_im2col_bwd(B, H, W, Cout, act):
    if B * H * W * Cout * 16 > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = torch.Generator(device="cuda").manual_seed(B * H * W + Cout + act)
    D, Y = _rnd(g, B, 2 * H, 2 * W, Cout), _rnd(g, B, 2 * H, 2 * W, Cout)
    al, be, ga = _rnd(g, Cout), _rnd(g, Cout) * 0.1, _rnd(g, Cout) * 0.1
    msc, msh = (_rnd(g, Cout).abs() + 0.5, _rnd(g, Cout) * 0.2) if act else (None, None)
    dcol = Buf(B * H * W, Cout * 16)
    lib.call("kd_deconv4x4s2_im2col_bwd", P(D), P(Y), P(al), P(be), P(ga), P(msc), P(msh), act, P(dcol.t), B, H, W, Cout,
             stream())
    torch.cuda.synchronize()
    ones = torch.ones(Cout, dtype=torch.float64, device="cuda")
    m = (msc.double(), msh.double()) if act else (ones, ones * 0)
    _check("dcol", dcol.t, R.im2col_bwd(*_d(D, Y, al, be, ga), *m, act, H, W)["dcol"])
    dcol.guard_ok("dcol")


# ---- bilinear resize ---------------------------------------------------------------------------------------------------

RESIZE = [(16, 64), (64, 45), (45, 64), (64, 16), (7, 64), (1, 5), (5, 1)]


def _maps(rows):
    """output map of `rows` pixels and a non-integer-ratio input map for it"""
    B, Ho, Wo = _bhw(rows)
    return B, (Ho * 3) // 4 + 1, Wo // 2 + 1, Ho, Wo


def _fwd_cases():
    cases = [(2, hi, hi + 3, ho, ho - 1 if ho > 1 else 1, 128, 1) for hi, ho in RESIZE]
    cases += [(*_maps(r), 128, 1) for r in _ladder(8, 2048).values()]
    cases += [(2, 16, 16, 64, 64, 4, 1), (1, 7, 5, 9, 13, 1024, 1), (2, 11, 6, 17, 9, 12, 1)]
    cases += [(2, 16, 16, 64, 64, 128, 2), (3, 45, 33, 64, 64, 12, 3), (2, 64, 64, 64, 64, 128, 3)]
    return cases


def _fwd_params():
    # the accumulate form takes one lateral per call; the sum form covers several
    return [(*c, m) for c in _fwd_cases() + [(256, 64, 64, 64, 64, 128, 3)] for m in (("sum", "accum0", "accum1") if c[-1] == 1 else ("sum",))]


@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo,C,nin,mode", _fwd_params(), ids=lambda v: str(v))
def test_bilinear_fwd(B, Hi, Wi, Ho, Wo, C, nin, mode):
    """kd_bilinear_sum_fwd over 1-3 deferred laterals (lateral i: (Hi, Wi) halved i times -- the FPN's 64^2, 32^2, 32^2 at the
    bench shape), and kd_bilinear_accum_fwd with accumulate 0 and 1 on the first lateral alone."""
    if B * Ho * Wo * C > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = torch.Generator(device="cuda").manual_seed(B * Ho * Wo + C + nin)
    lats = []
    for i in range(nin):
        hi, wi = max(1, Hi >> min(i, 1)), max(1, Wi >> min(i, 1))
        x = _rnd(g, B, hi, wi, C)
        sc, sh, _, _ = _bn(g, C)
        lats.append((x, sc, sh, R.RELU) if i != 1 else (x, None, None, 0))      # lateral 1 without a deferred affine
    out = Buf(B, Ho, Wo, C)
    out0 = None
    if mode == "sum":
        a = []
        for i in range(3):
            x, sc, sh, act = lats[i] if i < nin else (None, None, None, 0)
            a += [P(x), P(sc), P(sh), act, x.shape[1] if x is not None else 0, x.shape[2] if x is not None else 0]
        lib.call("kd_bilinear_sum_fwd", *a, P(out.t), B, Ho, Wo, C, stream())
    else:
        if mode == "accum1":
            out0 = _rnd(g, B, Ho, Wo, C)
            out.t.copy_(out0)
        x, sc, sh, act = lats[0]
        lib.call("kd_bilinear_accum_fwd", P(x), P(sc), P(sh), act, P(out.t), int(mode == "accum1"), B, x.shape[1], x.shape[2],
                 Ho, Wo, C, stream())
    torch.cuda.synchronize()
    ref = R.bilinear_sum_fwd([tuple(_d(*l)) for l in lats], Ho, Wo, out0=None if out0 is None else out0.double())
    _check("out", out.t, ref["out"])
    out.guard_ok("out")


def _bwd_cases():
    cases = [(2, hi, hi + 3, ho, ho - 1 if ho > 1 else 1, 128) for hi, ho in RESIZE]
    for r in _ladder(8, 2048).values():
        B, Hi, Wi = _bhw(r)
        cases.append((B, Hi, Wi, 2 * Hi - 1, Wi + 5, 128))
    cases += [(2, 16, 16, 64, 64, 4), (1, 7, 5, 9, 13, 1024), (2, 11, 6, 17, 9, 12), (2, 64, 64, 64, 64, 128)]
    return cases


@pytest.mark.parametrize("masked,tail", [(True, False), (True, True), (False, False)],
                         ids=["masked-all_rows", "masked-tail_rows", "plain"])      # no reduction without the mask
@pytest.mark.parametrize("B,Hi,Wi,Ho,Wo,C", _bwd_cases() + [(256, 32, 32, 64, 64, 128), (256, 64, 64, 64, 64, 128)],
                         ids=lambda v: str(v))
def test_bilinear_bwd(B, Hi, Wi, Ho, Wo, C, masked, tail):
    """the adjoint (gather form) and, masked, its BatchNorm-backward partial rows; the FPN's backward at the bench shape is
    one call per lateral: 64^2 -> 64^2 and 32^2 -> 64^2 (twice, the same shapes)."""
    if B * Ho * Wo * C > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = torch.Generator(device="cuda").manual_seed(B * Hi * Wi + Ho + C)
    npix = B * Hi * Wi
    slots, grid, iters = _layout(npix, C, 2048)
    dout, x = _rnd(g, B, Ho, Wo, C), _rnd(g, B, Hi, Wi, C)
    sc, sh, mean, inv = _bn(g, C)
    if tail:
        # every other input row pushed far below the ReLU threshold: its gradient and partial-sum terms are exactly 0
        sel = _tail_rows(npix, slots, grid, iters).view(B, Hi, Wi, 1)
        x = torch.where(sel, x, -(x.abs() + 10.0))
    if not masked:
        sc = sh = mean = inv = None
    rows = lib.kd_rowwise_stat_rows(npix, C)
    assert rows == grid
    gin, part = Buf(B, Hi, Wi, C), Buf(rows, 2, C)
    lib.call("kd_bilinear_bwd", P(dout), P(x) if masked else None, P(sc), P(sh), R.RELU, P(mean), P(inv), P(gin.t),
             P(part.t) if masked else None, B, Hi, Wi, Ho, Wo, C, stream())
    torch.cuda.synchronize()
    ref = R.bilinear_bwd(*_d(dout), Hi, Wi, *_d(x, sc, sh), R.RELU, *_d(mean, inv), n_part=iters + slots)
    _check("gin", gin.t, ref["gin"])
    if masked:
        s = part.t.double().sum(0)
        _check("sum g", s[0], ref["s1"])
        _check("sum g*xhat", s[1], ref["s2"])
    gin.guard_ok("gin"); part.guard_ok("partial")
