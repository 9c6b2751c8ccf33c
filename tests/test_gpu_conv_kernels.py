"""The camera body's kernels called directly through the C ABI -- the stem, its inference form and its im2col, the
depthwise 3x3 forward (five launches) and backward (seven kernels behind kd_set_dw_bwd_mode), kd_dwconv3x3_bwd_add
(csrc/kd_conv.hip) and the row-wise kd_bn_act_apply / kd_bn_act_apply_res / kd_bn_bwd_reduce (csrc/kd_bn.hip) -- compared
element-wise with a float64 evaluation of the same operation on the same fp32 inputs (tests/_fp64_conv_ref.py, plain torch
on the GPU, large cases in chunks of frames) within C_BOUND * n_seq * 2^-24 * sum|t_i| per output; the im2col bit for bit.
No element is left out of any comparison.

Work-item counts come from a mirror of dw_layout and of each kernel's walk (_fp64_conv_ref.dw_walk; the mirror's rows are
asserted equal to kd_dwconv_stat_rows / kd_dwconv_bwd_stat_rows in every case).  A work item of the depthwise kernels is a
column segment, not a pixel, so the ladders are built over items on one-segment maps: far fewer items than slots, a partial
block, cap*slots - 1, cap*slots, cap*slots + 1 (one item into a second turn of the grid-stride loop) and a ragged third turn
-- for each of the five forward launches and each backward mode, asserted per case (_on_ladder) -- plus the benchmarked
shapes.  Channel counts cover every dw_layout class (8 ... 1024, the chunked 384 / 768 / 1024 and the widths of the 8 / 24 /
40-channel students), each through a three-turn walk of every launch; maps cover H or W of 1-3, W = 15 / 16 / 17 / 33 and
H = 15 / 16 / 17 / 31 / 40.  Every reduction runs a second time with its input nonzero only in the pixels the walk of the
kernel under test handles last or at its edges (_fp64_conv_ref.dw_tail_mask, asserted sparse), so a dropped or doubled edge
costs O(1).  Outputs, slabs and workspaces start as NaN and carry a sentinel guard tail.  A failure names the kernel: the
launch the library selects is mirrored and printed in the message.

Kernel -> tests: dw_fwd_pipe_kernel<1,16> / <1,8> / <2,8>, dw_fwd_sw_kernel<1> / <2>: test_dw_fwd_forms, test_dw_fwd_ladder,
test_dw_fwd_multi_turn_channels (ids carry the kernel), test_dw_fwd_channels_and_edges, test_dw_fwd_bench_shapes,
test_dw_fwd_non_temporal_store_switch.  dw_bwd_data_sw_kernel, dw_bwd_weight_sw_kernel<1> (mode 0), dw_bwd_fused_s1_kernel
(mode 1), dw_bwd_tile_s1_kernel (mode 2), dw_bwd_data_s2_kernel, dw_bwd_weight_sw_kernel<2>, dw_bwd_fused_s2_kernel:
test_dw_bwd_stride1_forms, test_dw_bwd_stride2_forms, test_dw_bwd_ladder, test_dw_bwd_multi_turn_channels,
test_dw_bwd_channels_and_edges (ids carry mode and stride), test_dw_bwd_bench_shapes.  dw_bwd_fused_s1_kernel<ADD>:
test_dw_bwd_add, test_dw_bwd_add_bench_shape.  stem_fwd2_kernel (Cin 3) / stem_fwd_kernel and the inference form:
test_stem_widths, test_stem_ladder, test_stem_bench_shape.  stem_im2col2_kernel / stem_im2col_kernel: test_stem_im2col_bits.
bn_apply_kernel: test_bn_act_apply_ladder, test_bn_act_apply_forms; bn_bwd_reduce_kernel: test_bn_bwd_reduce_ladder,
test_bn_bwd_reduce_forms; both: test_bn_rowwise_bench_counts.

Measured on an MI355X: this file alone 14-16 s of wall time (1747 cases) at a peak of 56 GiB of allocated device
memory (the 0.37e9-element three-turn case of the tile kernel at C = 960 and the bench shapes, references in chunks of 2^25
elements); tests/test_gpu_tail_kernels.py and tests/test_gpu_loss_kernels.py together took 25 s in the same session, so no
bench-count case had to move behind a further gate.

Not covered: a tensor of >= 2^31 elements (the fall-back of the pipelined forward to dw_fwd_sw_kernel by size) -- outside the
benchmarked envelope, whose largest tensor has 0.8e9 elements."""
import pytest
import torch

import _fp64_conv_ref as R
from test_gpu_tail_kernels import Buf, _big, _check, _ladder, _layout

pytestmark = pytest.mark.gpu

CHUNK = 1 << 25                        # elements of the widest tensor of a reference chunk
CHANNELS = [8, 32, 48, 64, 144, 192, 240, 256, 288, 384, 480, 576, 768, 960, 1024]
BENCH_DW = [(256, 128, 128, 32, 1), (256, 128, 128, 192, 2), (256, 64, 64, 384, 1), (256, 64, 64, 384, 2), (256, 32, 32, 768, 1)]


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _gen(*key):
    return torch.Generator(device="cuda").manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _d(*ts):
    return [t.double() if torch.is_tensor(t) else t for t in ts]


def _frames(B, per_frame):
    step = max(1, CHUNK // max(1, per_frame))
    return [slice(b, min(B, b + step)) for b in range(0, B, step)]


def _sl(t, sl):
    return None if t is None else t[sl]


def _add(tot, r, keys):
    for k in keys:
        if k in r:
            tot[k] = r[k] if k not in tot else (tot[k][0] + r[k][0], tot[k][1] + r[k][1])


def _shares_ok(x, sc, sh, what):
    if x.numel() >= 4096:
        lo, mid, hi = R.relu6_shares(x, sc, sh)
        assert min(lo, mid, hi) >= 0.01, f"ReLU6 inputs must exercise both clamps {what}: {lo:.3f} / {mid:.3f} / {hi:.3f}"


def _gate(B, H, W):
    if B * H * W > 2 ** 20:
        _big()


def _split(n):
    """n work items as B frames x n / B column units, B > 1 where n allows it"""
    return next((B, n // B) for B in (7, 5, 11, 13, 8, 4, 3, 2, 1) if n % B == 0)


def _with_tail(cases):
    """every ladder case with all inputs and, where the walk is long enough to have a tail to single out, with tail inputs"""
    return [(*c, t) for c in cases for t in ("all", "tail") if t == "all" or c[-1] not in ("few", "partial_block")]


def _on_ladder(name, wk, what):
    """the walk is what the ladder name says: one turn up to `full`, a second turn of one item, a ragged third turn"""
    if name is None:
        return
    items, per_turn, iters = wk["items"], wk["per_turn"], wk["iters"]
    ok = {"few": iters == 1 and items < wk["slots"] + 1, "partial_block": iters == 1 and items < per_turn,
          "full-1": iters == 1 and items == per_turn - 1, "full": iters == 1 and items == per_turn,
          "full+1": iters == 2 and items == per_turn + 1, "ragged": iters == 3 and items % per_turn != 0}[name]
    assert ok, f"not a '{name}' walk: {wk} {what}"


def _sparse(mask, what):
    f = mask.float().mean().item()
    assert 0 < f < 0.5, f"tail inputs must be sparse: {f:.3f} of the pixels selected {what}"
    return mask[..., None]


# ---- depthwise forward -------------------------------------------------------------------------------------------------

def _dw_fwd_run(B, H, W, C, stride, act_id, partial=True, tail=False, expect=None, ladder=None):
    _gate(B, H, W)
    lib, P, stream = _lib()
    g = _gen(B, H, W, C, stride, 3 if act_id is None else act_id)
    x, w = R.rnd(g, B, H, W, C), R.rnd(g, C, 9)
    sc = sh = None
    form = R.dw_fwd_form(B, H, W, C, stride)[0]
    what = f"[{form} B={B} H={H} W={W} C={C} act={act_id} tail={tail}]"
    assert expect is None or form == expect, what
    if act_id is not None:
        sc, sh, _, _ = R.coeffs(g, C, act_id)
        if act_id == 2:
            _shares_ok(x, sc, sh, what)
    _on_ladder(ladder, R.dw_walk("fwd", B, H, W, C, stride), what)
    if tail:
        x = x * _sparse(R.dw_fwd_tail_mask(B, H, W, C, stride, "cuda"), what)
    Ho, Wo = R._out_size(H, stride), R._out_size(W, stride)
    rows = lib.kd_dwconv_stat_rows(B * Ho * Wo, C)
    assert rows == R.dw_layout(B * Ho * Wo, C)[3], what
    y, part = Buf(B, Ho, Wo, C), Buf(rows, 2, C)
    lib.call("kd_dwconv3x3_fwd", P(x), P(sc), P(sh), act_id or 0, P(w), P(y.t), P(part.t) if partial else None, B, H, W, C, stride,
             stream())
    torch.cuda.synchronize()
    n_part = R.dw_fwd_chain(B, H, W, C, stride)
    tot = {}
    for sl in _frames(B, H * W * C):
        r = R.dw_fwd(x[sl].double(), *_d(sc, sh), act_id or 0, w.double(), stride, n_part)
        _check(f"y {what}", y.t[sl], r["y"])
        _add(tot, r, ("s1", "s2"))
    if partial:
        s = part.t.double().sum(0)
        _check(f"sum y {what}", s[0], tot["s1"])
        _check(f"sum y^2 {what}", s[1], tot["s2"])
    else:
        assert bool(torch.isnan(part.t).all()), what
    y.guard_ok("y"); part.guard_ok("partial")


# the five launches, chosen through H alone: (stride, H, kernel)
FWD_FORMS = [(1, 32, "dw_fwd_pipe_kernel<1,16>"), (1, 24, "dw_fwd_pipe_kernel<1,8>"), (1, 17, "dw_fwd_sw_kernel<1>"),
             (2, 31, "dw_fwd_pipe_kernel<2,8>"), (2, 16, "dw_fwd_pipe_kernel<2,8>"), (2, 33, "dw_fwd_sw_kernel<2>"),
             (1, 15, "dw_fwd_sw_kernel<1>"), (1, 40, "dw_fwd_pipe_kernel<1,8>"), (1, 16, "dw_fwd_pipe_kernel<1,16>")]


@pytest.mark.parametrize("partial", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("act_id", [None, 0, 1, 2], ids=["plain", "act0", "relu", "relu6"])
@pytest.mark.parametrize("stride,H,kernel", FWD_FORMS, ids=lambda v: str(v))
def test_dw_fwd_forms(stride, H, kernel, act_id, partial):
    _dw_fwd_run(3, H, 19, 48, stride, act_id, partial, expect=kernel)


# every dw_layout class on the spatial edges: H or W of 1, 2, 3; W = 15 / 16 / 17 / 33; H = 15 / 16 / 17 / 31 / 40
SHAPES = [(2, 1, 7, 8), (3, 3, 2, 32), (2, 2, 3, 48), (5, 5, 1, 64), (2, 15, 15, 64), (1, 16, 16, 64), (3, 17, 17, 64),
          (2, 31, 33, 64), (1, 40, 16, 128), (2, 16, 33, 32), (1, 17, 15, 48), (2, 40, 17, 144), (1, 31, 16, 192),
          (3, 16, 17, 240), (1, 15, 33, 256), (2, 17, 16, 288), (1, 40, 15, 384), (2, 16, 16, 480), (1, 31, 17, 576),
          (3, 8, 33, 768), (1, 17, 16, 960), (2, 24, 15, 1024), (7, 9, 6, 8)]


def test_shapes_cover_every_channel_class():
    assert {s[3] for s in SHAPES} >= set(CHANNELS)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", SHAPES, ids=lambda v: str(v))
def test_dw_fwd_channels_and_edges(B, H, W, C, stride):
    _dw_fwd_run(B, H, W, C, stride, 2)


# a one-segment map per launch, so that the work items are B x Wo column segments: kernel -> (stride, H)
FWD_LADDER_H = {"dw_fwd_pipe_kernel<1,16>": (1, 16), "dw_fwd_pipe_kernel<1,8>": (1, 8), "dw_fwd_sw_kernel<1>": (1, 5),
                "dw_fwd_pipe_kernel<2,8>": (2, 15), "dw_fwd_sw_kernel<2>": (2, 9)}


def _fwd_ladder_cases(channels, names):
    out = []
    for kernel, (stride, H) in FWD_LADDER_H.items():
        for C in channels:
            for name, n in R.dw_item_ladder(C).items():
                if name in names:
                    B, U = _split(n)
                    out.append((kernel, B, H, U if stride == 1 else 2 * U - 1, C, stride, name))
    return out


@pytest.mark.parametrize("kernel,B,H,W,C,stride,name,tail", _with_tail(_fwd_ladder_cases((32, 64, 384), ("few", "partial_block", "full-1", "full", "full+1", "ragged"))),
                         ids=lambda v: str(v))
def test_dw_fwd_ladder(kernel, B, H, W, C, stride, name, tail):
    """the ladder over WORK ITEMS (column segments) of every forward launch: up to one full turn of the grid, one item into the
    second turn, a ragged third turn"""
    tail = tail == "tail"
    _dw_fwd_run(B, H, W, C, stride, None if tail else 2, tail=tail, expect=kernel, ladder=name)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("kernel,B,H,W,C,stride,name", _fwd_ladder_cases([c for c in CHANNELS if c not in (32, 64, 384)], ("ragged",)),
                         ids=lambda v: str(v))
def test_dw_fwd_multi_turn_channels(kernel, B, H, W, C, stride, name, tail):
    """every other dw_layout class through three turns of every forward launch"""
    _dw_fwd_run(B, H, W, C, stride, None if tail else 2, tail=tail, expect=kernel, ladder=name)


NT_W = {"below_64MiB": 255, "at_64MiB": 256}                 # 8 x 256 x W x 32 floats


@pytest.mark.parametrize("size", list(NT_W))
def test_dw_fwd_non_temporal_store_switch(size):
    assert (8 * 256 * NT_W[size] * 32 * 4 >= 64 << 20) == (size == "at_64MiB")
    _dw_fwd_run(8, 256, NT_W[size], 32, 1, 2)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("B,H,W,C,stride", BENCH_DW, ids=lambda v: str(v))
def test_dw_fwd_bench_shapes(B, H, W, C, stride, tail):
    _dw_fwd_run(B, H, W, C, stride, None if tail else 2, tail=tail)


# ---- depthwise backward ------------------------------------------------------------------------------------------------

def _dw_bwd_run(mode, B, H, W, C, stride, outs="both", fold=2, deferred=True, act_id=2, tail=False, addend=False, expect=None,
                ladder=None):
    """fold 0: D is dy; 1: BatchNorm backward folded into the load of (D, Y); 2: the same under the (dsc, dsh, d_act) mask"""
    _gate(B, H, W)
    lib, P, stream = _lib()
    g = _gen(B, H, W, C, stride, mode, fold, 11)
    Ho, Wo = R._out_size(H, stride), R._out_size(W, stride)
    want_gx, want_dw = outs != "dw", outs != "gx"
    names, n_part, n_red = R.dw_bwd_forms(mode, B, H, W, C, stride, want_gx, want_dw)
    what = f"[{'+'.join(names)} mode={mode} B={B} H={H} W={W} C={C} s={stride} {outs} fold={fold} deferred={deferred} tail={tail}]"
    assert expect is None or names == [expect], what
    x, w, D = R.rnd(g, B, H, W, C), R.rnd(g, C, 9), R.rnd(g, B, Ho, Wo, C)
    Y = al = be = ga = dsc = dsh = sc = sh = mean = inv = add = None
    if fold:
        Y = R.rnd(g, B, Ho, Wo, C)
        al, be, ga = R.folded(g, C)
        if fold == 2:
            dsc, dsh, _, _ = R.coeffs(g, C, 2)
            _shares_ok(Y, dsc, dsh, what)
    if deferred:
        sc, sh, mean, inv = R.coeffs(g, C, act_id)
        if act_id == 2:
            _shares_ok(x, sc, sh, what)
    if addend:
        add = R.rnd(g, B, H, W, C)
    for n in names:
        _on_ladder(ladder, R.dw_walk(R.KERNEL_WALK[n], B, H, W, C, stride), what)
    if tail:
        D = D * _sparse(R.dw_bwd_tail_mask(names, B, H, W, C, stride, "cuda"), what)
    rows = lib.kd_dwconv_bwd_stat_rows(B * H * W, C)
    assert rows == R.dw_layout(B * H * W, C)[3], what
    nbytes = lib.kd_dwconv_bwd_ws_bytes(B * Ho * Wo, C)
    assert nbytes == R.dw_layout(4 * B * Ho * Wo, C)[3] * C * 9 * 4, what
    gx, part, dw, ws = Buf(B, H, W, C), Buf(rows, 2, C), Buf(C, 9), Buf(nbytes // 4)
    prev = lib.kd_set_dw_bwd_mode(mode)
    try:
        common = (P(D), P(Y), P(al), P(be), P(ga), P(dsc), P(dsh), 2 if fold == 2 else 0, P(x), P(sc), P(sh), act_id if deferred else 0,
                  P(mean), P(inv), P(w))
        tail_args = (P(gx.t) if want_gx else None, P(part.t), P(dw.t) if want_dw else None, B, H, W, C, stride, P(ws.t), nbytes, stream())
        if addend:
            lib.call("kd_dwconv3x3_bwd_add", *common, P(add), *tail_args)
        else:
            lib.call("kd_dwconv3x3_bwd", *common, *tail_args)
        torch.cuda.synchronize()
    finally:
        lib.kd_set_dw_bwd_mode(prev)
    tot = {}
    for sl in _frames(B, H * W * C):
        r = R.dw_bwd(*_d(D[sl], _sl(Y, sl), al, be, ga, dsc, dsh), 2 if fold == 2 else 0, *_d(x[sl], sc, sh), act_id if deferred else 0,
                     *_d(mean, inv, w), stride, None if add is None else add[sl].double(), n_part, n_red)
        if want_gx:
            _check(f"gx {what}", gx.t[sl], r["gx"])
        _add(tot, r, ("s1", "s2", "dw"))
    if want_dw:
        _check(f"dw {what}", dw.t, tot["dw"])
    else:
        assert bool(torch.isnan(dw.t).all()), what
    if want_gx and deferred:
        s = part.t.double().sum(0)
        _check(f"sum gx {what}", s[0], tot["s1"])
        _check(f"sum gx*xhat {what}", s[1], tot["s2"])
    else:
        assert bool(torch.isnan(part.t).all()), what
    if not want_gx:
        assert bool(torch.isnan(gx.t).all()), what
    for nm, b in (("gx", gx), ("partial", part), ("dw", dw), ("ws", ws)):
        b.guard_ok(nm)


S1_KERNEL = {0: None, 1: "dw_bwd_fused_s1_kernel", 2: "dw_bwd_tile_s1_kernel"}


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("fold", [0, 1, 2], ids=["dy", "folded", "folded_masked"])
@pytest.mark.parametrize("outs", ["both", "gx", "dw"])
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,W,C", [(2, 17, 19, 8), (1, 33, 16, 64), (2, 16, 15, 64)], ids=lambda v: str(v))
def test_dw_bwd_stride1_forms(B, H, W, C, mode, outs, fold, deferred):
    """C = 64 at W = 16 / 15 sits on either side of the line where mode 3 switches from the tile to the column-walk kernel"""
    expect = None
    if outs == "both" and mode:
        expect = S1_KERNEL[R.dw_fused_form(mode, C, W, 1)]
    _dw_bwd_run(mode, B, H, W, C, 1, outs, fold, deferred, expect=expect)


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("fold", [0, 1, 2], ids=["dy", "folded", "folded_masked"])
@pytest.mark.parametrize("outs", ["both", "gx", "dw"])
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("B,H,W,C", [(2, 17, 19, 8), (1, 32, 18, 64)], ids=lambda v: str(v))
def test_dw_bwd_stride2_forms(B, H, W, C, mode, outs, fold, deferred):
    _dw_bwd_run(mode, B, H, W, C, 2, outs, fold, deferred, expect="dw_bwd_fused_s2_kernel" if outs == "both" and mode else None)


@pytest.mark.parametrize("act_id", [0, 1])
@pytest.mark.parametrize("stride", [1, 2])
def test_dw_bwd_other_input_activations(stride, act_id):
    _dw_bwd_run(3, 2, 18, 21, 48, stride, act_id=act_id)


@pytest.mark.parametrize("mode,stride", [(0, 1), (1, 1), (2, 1), (3, 1), (0, 2), (3, 2)], ids=lambda v: str(v))
@pytest.mark.parametrize("B,H,W,C", SHAPES, ids=lambda v: str(v))
def test_dw_bwd_channels_and_edges(B, H, W, C, mode, stride):
    _dw_bwd_run(mode, B, H, W, C, stride)


BWD_MODES = [(0, 1), (1, 1), (2, 1), (3, 1), (0, 2), (3, 2)]                # (kd_set_dw_bwd_mode, stride)


def _bwd_ladder_cases(channels, names):
    """maps of one segment (5 rows; 15 under stride 2), so that the work items of the kernels of (mode, stride) are B x column
    units: columns, 16-column strips with a ragged last one (tile form) or 2-column quads of an odd-width map (stride 2)"""
    out = []
    for mode, stride in BWD_MODES:
        for C in channels:
            kind = R.KERNEL_WALK[R.dw_bwd_forms(mode, 1, 5, 64, C, stride, True, True)[0][0]]
            colw = {"bwd_tile": 16, "bwd_quad": 2}.get(kind, 1)
            for name, n in R.dw_item_ladder(C, tile=kind == "bwd_tile").items():
                if name in names:
                    B, U = _split(n)
                    W = U * colw - {16: 5 if U > 1 else 0, 2: 1, 1: 0}[colw]
                    out.append((mode, stride, B, 5 if stride == 1 else 15, W, C, name))
    return out


@pytest.mark.parametrize("mode,stride,B,H,W,C,name,tail", _with_tail(_bwd_ladder_cases((32, 64, 384), ("few", "partial_block", "full-1", "full", "full+1", "ragged"))),
                         ids=lambda v: str(v))
def test_dw_bwd_ladder(mode, stride, B, H, W, C, name, tail):
    """the ladder over WORK ITEMS of every backward kernel (both gradients; mode 0: the separate data and weight kernels, whose
    walks have the same item count here)"""
    tail = tail == "tail"
    _dw_bwd_run(mode, B, H, W, C, stride, fold=0 if tail else 2, tail=tail, ladder=name)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("mode,stride,B,H,W,C,name", _bwd_ladder_cases([c for c in CHANNELS if c not in (32, 64, 384)], ("ragged",)),
                         ids=lambda v: str(v))
def test_dw_bwd_multi_turn_channels(mode, stride, B, H, W, C, name, tail):
    """every other dw_layout class through three turns of every backward kernel"""
    _dw_bwd_run(mode, B, H, W, C, stride, fold=0 if tail else 2, tail=tail, ladder=name)


@pytest.mark.parametrize("size", list(NT_W))
def test_dw_bwd_non_temporal_store_switch(size):
    _dw_bwd_run(3, 8, 256, NT_W[size], 32, 1)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("B,H,W,C,stride", BENCH_DW, ids=lambda v: str(v))
def test_dw_bwd_bench_shapes(B, H, W, C, stride, tail):
    _dw_bwd_run(3, B, H, W, C, stride, fold=0 if tail else 2, tail=tail)


@pytest.mark.parametrize("deferred", [True, False], ids=["deferred", "plain"])
@pytest.mark.parametrize("B,H,W,C", [(2, 13, 19, 8), (2, 40, 36, 32), (1, 17, 9, 48), (2, 16, 15, 64), (1, 18, 20, 144)], ids=lambda v: str(v))
def test_dw_bwd_add(B, H, W, C, deferred):
    lib, _, _ = _lib()
    assert lib.kd_dwconv3x3_bwd_add_supported(C, W, 1) == 1
    _dw_bwd_run(3, B, H, W, C, 1, deferred=deferred, addend=True, expect="dw_bwd_fused_s1_kernel")


def test_dw_bwd_add_bench_shape():
    _dw_bwd_run(3, 256, 128, 128, 32, 1, addend=True, expect="dw_bwd_fused_s1_kernel")


@pytest.mark.parametrize("B,H,W,C,stride", [(1, 16, 16, 64, 1), (2, 8, 8, 8, 2)], ids=lambda v: str(v))
def test_dw_bwd_add_refuses_other_forms(B, H, W, C, stride):
    lib, P, stream = _lib()
    assert lib.kd_dwconv3x3_bwd_add_supported(C, W, stride) == 0
    g = _gen(B, H, W, C)
    Ho, Wo = R._out_size(H, stride), R._out_size(W, stride)
    D, x, w, add = R.rnd(g, B, Ho, Wo, C), R.rnd(g, B, H, W, C), R.rnd(g, C, 9), R.rnd(g, B, H, W, C)
    nbytes = lib.kd_dwconv_bwd_ws_bytes(B * Ho * Wo, C)
    gx, dw, ws = Buf(B, H, W, C), Buf(C, 9), Buf(nbytes // 4)
    rc = lib.kd_dwconv3x3_bwd_add(P(D), None, None, None, None, None, None, 0, P(x), None, None, 0, None, None, P(w), P(add), P(gx.t), None,
                                  P(dw.t), B, H, W, C, stride, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    assert rc < 0
    assert bool(torch.isnan(gx.t).all()) and bool(torch.isnan(dw.t).all()) and bool(torch.isnan(ws.t).all())


@pytest.mark.parametrize("C", [6, 1028])
def test_dw_refuses_unsupported_channel_counts(C):
    lib, P, stream = _lib()
    B, H, W = 2, 5, 6
    g = _gen(C)
    x, w, D = R.rnd(g, B, H, W, C), R.rnd(g, C, 9), R.rnd(g, B, H, W, C)
    y, part, gx, dw, ws = Buf(B, H, W, C), Buf(64, 2, C), Buf(B, H, W, C), Buf(C, 9), Buf(64 * C * 9)
    rc = lib.kd_dwconv3x3_fwd(P(x), None, None, 0, P(w), P(y.t), P(part.t), B, H, W, C, 1, stream())
    rb = lib.kd_dwconv3x3_bwd(P(D), None, None, None, None, None, None, 0, P(x), None, None, 0, None, None, P(w), P(gx.t), P(part.t), P(dw.t),
                              B, H, W, C, 1, P(ws.t), 64 * C * 9 * 4, stream())
    torch.cuda.synchronize()
    assert rc < 0 and rb < 0
    for b in (y, part, gx, dw, ws):
        assert bool(torch.isnan(b.t).all())
        b.guard_ok("refused")


# ---- stem --------------------------------------------------------------------------------------------------------------

def _stem_tail(B, Ho, Wo):
    """output pixels the stem's walk over 256-pixel batches handles last or at its edges"""
    npix = B * Ho * Wo
    grid = min(-(-npix // 256), 1024)
    sel = R.row_tail_mask(npix, 256, grid, "cuda").view(B, Ho, Wo)
    sel[0, 0, :] = sel[0, :, 0] = sel[-1, -1, :] = sel[-1, :, -1] = True
    return sel


def _stem_run(cout, cin, B, H, W, tail=False):
    Ho, Wo = R._out_size(H, 2), R._out_size(W, 2)
    _gate(B, Ho, Wo)
    lib, P, stream = _lib()
    g = _gen(cout, cin, B, H, W)
    x, w = R.rnd(g, B, cin, H, W), R.rnd(g, cout, cin, 3, 3) * 0.4
    npix = B * Ho * Wo
    what = f"[{'stem_fwd2_kernel' if cin == 3 else 'stem_fwd_kernel'} Cout={cout} Cin={cin} B={B} H={H} W={W} tail={tail}]"
    if tail:
        x = x * _stem_tail(B, Ho, Wo).repeat_interleave(2, 1).repeat_interleave(2, 2)[:, None, :H, :W]
    rows = lib.kd_stem_stat_rows(npix)
    assert rows == min(-(-npix // 256), 1024)
    y, part = Buf(B, Ho, Wo, cout), Buf(rows, 2, cout)
    lib.call("kd_stem_conv_fwd", P(x), P(w), P(y.t), P(part.t), B, cin, H, W, cout, stream())
    yi = None
    if cin == 3 and not tail:
        sc, sh, _, _ = R.coeffs(g, cout, 2)
        yi = Buf(B, Ho, Wo, cout)
        lib.call("kd_stem_conv_fwd_infer", P(x), P(w), P(sc), P(sh), 2, P(yi.t), B, cin, H, W, cout, stream())
    torch.cuda.synchronize()
    tot = {}
    for sl in _frames(B, max(cin * H * W, Ho * Wo * cout)):
        r = R.stem_fwd(x[sl].double(), w.double(), R.stem_chain(npix, cin))
        _check(f"raw {what}", y.t[sl], r["y"])
        _add(tot, r, ("s1", "s2"))
        if yi is not None:
            _check(f"infer {what}", yi.t[sl], R.stem_infer(*_d(x[sl], w, sc, sh), 2)["y"])
    s = part.t.double().sum(0)
    _check(f"sum y {what}", s[0], tot["s1"])
    _check(f"sum y^2 {what}", s[1], tot["s2"])
    y.guard_ok("y"); part.guard_ok("partial")
    if yi is not None:
        _shares_ok(y.t, sc, sh, what)
        yi.guard_ok("y infer")


# B, H, W of the image: one partial block; 1023 / 1024 / 1025 pixel-batches of 256 and one pixel either side of 1024; a
# ragged multi-iteration count with odd H and W
STEM_SIZES = {"partial_block": (3, 17, 13), "1023_batches": (3, 681, 512), "1024_batches-1px": (1, 1021, 1025),
              "1024_batches": (4, 512, 512), "1024_batches+1px": (5, 961, 217), "1025_batches": (5, 409, 512),
              "ragged": (7, 601, 589)}


def test_stem_sizes_are_what_they_say():
    px = {k: B * R._out_size(H, 2) * R._out_size(W, 2) for k, (B, H, W) in STEM_SIZES.items()}
    assert px["partial_block"] < 256 and px["1023_batches"] == 1023 * 256 and px["1024_batches-1px"] == 1024 * 256 - 1
    assert px["1024_batches"] == 1024 * 256 and px["1024_batches+1px"] == 1024 * 256 + 1 and px["1025_batches"] == 1025 * 256
    assert px["ragged"] > 2 * 1024 * 256 and px["ragged"] % (1024 * 256) != 0


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("size", ["partial_block", "ragged"])
@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("cout", [8, 16, 24, 32, 40])
def test_stem_widths(cout, cin, size, tail):
    _stem_run(cout, cin, *STEM_SIZES[size], tail=tail)


@pytest.mark.parametrize("size", [k for k in STEM_SIZES if "batches" in k])
@pytest.mark.parametrize("cin", [1, 3, 4])
@pytest.mark.parametrize("cout", [8, 16, 24, 32, 40])
def test_stem_ladder(cout, cin, size):
    _stem_run(cout, cin, *STEM_SIZES[size])


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
def test_stem_bench_shape(tail):
    _stem_run(32, 3, 256, 256, 256, tail=tail)


@pytest.mark.parametrize("B,H,W", [(3, 45, 37), (2, 1, 3), (7, 601, 589), (4, 1024, 1024)], ids=lambda v: str(v))
@pytest.mark.parametrize("cin,Kp,offset,kernel", [(3, 32, 0, "stem_im2col2_kernel"), (3, 32, 1, "stem_im2col_kernel"), (4, 36, 0, "stem_im2col_kernel"),
                                                  (1, 12, 0, "stem_im2col_kernel")], ids=lambda v: str(v))
def test_stem_im2col_bits(cin, Kp, offset, kernel, B, H, W):
    """both forms (Cin 3, Kp 32, aligned; the generic kernel otherwise, also through a `col` pointer 4 bytes off alignment), below and
    above the 2048-block cap of the first (7 x 301 x 295 and 4 x 512 x 512 output pixels)"""
    lib, P, stream = _lib()
    Ho, Wo = R._out_size(H, 2), R._out_size(W, 2)
    _gate(B, Ho, Wo)
    x = R.rnd(_gen(cin, Kp, B, H, W), B, cin, H, W)
    col = Buf(B * Ho * Wo * Kp + offset)
    out = col.t[offset:]
    lib.call("kd_stem_im2col", P(x), P(out), B, cin, H, W, Kp, stream())
    torch.cuda.synchronize()
    for sl in _frames(B, Ho * Wo * Kp):
        want = R.stem_im2col(x[sl], Kp)
        got = out.view(B, Ho * Wo, Kp)[sl].reshape(-1, Kp)
        assert torch.equal(got, want), f"[{kernel} Cin={cin} Kp={Kp} B={B} H={H} W={W}]"
    assert offset == 0 or bool(torch.isnan(col.t[:offset]).all())
    col.guard_ok("col")


# ---- row-wise BatchNorm kernels ----------------------------------------------------------------------------------------

def _strided(g, M, C, pad, lead):
    """an [M, C] column slice, starting at column `lead`, of a wider buffer"""
    buf = R.rnd(g, M, C + pad)
    return buf[:, lead:lead + C]


def _rows(M, C):
    step = max(1, CHUNK // C)
    return [slice(m, min(M, m + step)) for m in range(0, M, step)]


def _bn_apply_run(M, C, act_id, res_mode, strided=True):
    if M * C > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = _gen(M, C, act_id, len(res_mode))
    pads = (8, 4, 12) if strided else (0, 0, 0)                 # every slice starts on a 16-byte boundary
    x = _strided(g, M, C, pads[0], pads[0] // 2)
    sc, sh, _, _ = R.coeffs(g, C, act_id)
    res = rsc = rsh = None
    if res_mode != "none":
        res = _strided(g, M, C, pads[1], pads[1])
    if res_mode == "deferred":
        rsc, rsh, _, _ = R.coeffs(g, C, 2)
    what = f"[M={M} C={C} act={act_id} res={res_mode} strided={strided}]"
    if act_id == 2:
        _shares_ok(x, sc, sh, what)
    ob = Buf(M, C + pads[2])
    lo = 2 * pads[2] // 3
    out = ob.t[:, lo:lo + C]
    ldr = res.stride(0) if res is not None else 0
    if res_mode == "deferred":
        lib.call("kd_bn_act_apply_res", P(x), x.stride(0), P(sc), P(sh), act_id, P(res), ldr, P(rsc), P(rsh), 2, P(out), out.stride(0), M, C,
                 stream())
    else:
        lib.call("kd_bn_act_apply", P(x), x.stride(0), P(sc), P(sh), act_id, P(res), ldr, P(out), out.stride(0), M, C, stream())
    torch.cuda.synchronize()
    for sl in _rows(M, C):
        ref = R.bn_act_apply(*_d(x[sl], sc, sh), act_id, *_d(_sl(res, sl), rsc, rsh), 2)
        _check(f"out {what}", out[sl].contiguous(), ref["out"])
    if strided:
        assert bool(torch.isnan(ob.t[:, :lo]).all()) and bool(torch.isnan(ob.t[:, lo + C:]).all()), f"written outside its C columns {what}"
    ob.guard_ok("out")


def _bn_reduce_run(M, C, act_id, tail, strided=True):
    if M * C > 2 ** 26:
        _big()
    lib, P, stream = _lib()
    g = _gen(M, C, act_id, 5)
    pads = (8, 4) if strided else (0, 0)
    Dv, X = _strided(g, M, C, pads[0], pads[0]), _strided(g, M, C, pads[1], 0)
    sc, sh, mean, inv = R.coeffs(g, C, act_id)
    slots, grid, iters = _layout(M, C, 2048)
    what = f"[M={M} C={C} act={act_id} tail={tail} strided={strided}]"
    if act_id == 2:
        _shares_ok(X, sc, sh, what)
    if tail:
        Dv = Dv * R.row_tail_mask(M, slots, grid, "cuda")[:, None]
    rows = lib.kd_rowwise_stat_rows(M, C)
    assert rows == grid, what
    part = Buf(rows, 2, C)
    plain = act_id == 0
    lib.call("kd_bn_bwd_reduce", P(Dv), Dv.stride(0), P(X), X.stride(0), None if plain else P(sc), None if plain else P(sh), act_id, P(mean),
             P(inv), P(part.t), M, C, stream())
    torch.cuda.synchronize()
    tot = {}
    for sl in _rows(M, C):
        _add(tot, R.bn_bwd_reduce(*_d(Dv[sl], X[sl], sc, sh), act_id, *_d(mean, inv), iters + slots), ("s1", "s2"))
    s = part.t.double().sum(0)
    _check(f"sum G {what}", s[0], tot["s1"])
    _check(f"sum G*xhat {what}", s[1], tot["s2"])
    part.guard_ok("partial")


def _bn_cases():
    """the kd_cg_layout ladder of tests/test_gpu_tail_kernels.py (cap 2048); C = 48 and 192 leave threads idle"""
    return [(n, C, name) for C in (32, 48, 64, 128, 192, 768) for name, n in _ladder(max(1, 256 // (C // 4)), 2048).items()]


RES = ["none", "plain", "deferred"]


@pytest.mark.parametrize("res_mode", RES)
@pytest.mark.parametrize("act_id", [0, 1, 2], ids=["act0", "relu", "relu6"])
@pytest.mark.parametrize("M,C,name", _bn_cases(), ids=lambda v: str(v))
def test_bn_act_apply_ladder(M, C, name, act_id, res_mode):
    _bn_apply_run(M, C, act_id, res_mode)


@pytest.mark.parametrize("res_mode", RES)
@pytest.mark.parametrize("act_id", [0, 1, 2])
def test_bn_act_apply_forms(act_id, res_mode):
    _bn_apply_run(4099, 48, act_id, res_mode)
    _bn_apply_run(517, 192, act_id, res_mode, strided=False)


@pytest.mark.parametrize("tail", [False, True], ids=["all", "tail"])
@pytest.mark.parametrize("M,C,name", _bn_cases(), ids=lambda v: str(v))
def test_bn_bwd_reduce_ladder(M, C, name, tail):
    _bn_reduce_run(M, C, list(_ladder(1, 1)).index(name) % 3, tail)


@pytest.mark.parametrize("act_id", [0, 1, 2])
def test_bn_bwd_reduce_forms(act_id):
    _bn_reduce_run(4099, 48, act_id, False)
    _bn_reduce_run(517, 192, act_id, True, strided=False)


@pytest.mark.parametrize("M,C", [(256 * 128 * 128, 32), (256 * 64 * 64, 64)], ids=lambda v: str(v))
def test_bn_rowwise_bench_counts(M, C):
    _bn_apply_run(M, C, 2, "deferred")
    _bn_apply_run(M, C, 2, "none", strided=False)
    _bn_reduce_run(M, C, 2, False)
    _bn_reduce_run(M, C, 2, True, strided=False)


def test_bn_rowwise_refuses_row_strides_off_float4():
    lib, P, stream = _lib()
    M, C = 100, 32
    g = _gen(M, C)
    wide, sc, sh = R.rnd(g, M, C + 2), R.rnd(g, C), R.rnd(g, C)
    x, good = wide[:, :C], R.rnd(g, M, C)
    out, part = Buf(M, C + 2), Buf(lib.kd_rowwise_stat_rows(M, C), 2, C)
    assert lib.kd_bn_act_apply(P(x), C + 2, P(sc), P(sh), 1, None, 0, P(out.t), C, M, C, stream()) < 0
    assert lib.kd_bn_act_apply(P(good), C, P(sc), P(sh), 1, None, 0, P(out.t), C + 2, M, C, stream()) < 0
    assert lib.kd_bn_act_apply(P(good), C, P(sc), P(sh), 1, P(x), C + 2, P(out.t), C, M, C, stream()) < 0
    assert lib.kd_bn_act_apply_res(P(good), C, P(sc), P(sh), 1, P(x), C + 2, P(sc), P(sh), 1, P(out.t), C, M, C, stream()) < 0
    assert lib.kd_bn_bwd_reduce(P(x), C + 2, P(good), C, P(sc), P(sh), 1, P(sc), P(sh), P(part.t), M, C, stream()) < 0
    assert lib.kd_bn_bwd_reduce(P(good), C, P(x), C + 2, P(sc), P(sh), 1, P(sc), P(sh), P(part.t), M, C, stream()) < 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.t).all()) and bool(torch.isnan(part.t).all())
    out.guard_ok("out"); part.guard_ok("partial")
