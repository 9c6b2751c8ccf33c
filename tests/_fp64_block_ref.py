"""Float64 references for the fused inference block kernels of csrc/kd_block.hip -- dw_pw_infer_kernel (kd_dw_pw_infer: depthwise
3x3 + BatchNorm + activation -> 1x1 + BatchNorm + activation (+ residual)) and block_infer_kernel (kd_block_infer: the same behind
the expand 1x1 + BatchNorm + activation of an InvertedResidual) -- with the rounding-error bound each output must meet, an fp32
emulation of the kernels' arithmetic, the input recipes and the case table shared by tests/test_gpu_block_kernels.py and the CPU
self-check tests/test_fp64_block_ref_host.py.  Same conventions as tests/_fp64_conv_ref.py and tests/_fp64_gemm_ref.py: plain torch,
evaluated in the dtype of the inputs (float64 for the truth, float32 for the self-check of the bound), nine explicit shifted
multiply-adds over a zero-padded NHWC tensor, a matmul for the 1x1s, nothing from the library and no F.conv2d; every function
returns (value, err) with

    err = C_BOUND * n_seq * U * sum |t_i|

`sum |t_i|` evaluated alongside the value.  The zero padding of the depthwise input is applied AFTER the input's BatchNorm and
activation, as the kernels do (act(0 * sc + sh) != 0).

n_seq, counted from the kernel source (every kd_affine is one fmaf; `acc + bias` with a null bias adds an exact 0.f):

  deferred input affine        1       (dw_pw_infer_kernel, isc given: kd_affine_act4 on the staged halo tile)
  expand                       Cin + SPLIT_TERMS (+ 1 ebias) + 1    (block_infer_kernel: K ascending MFMA chain, e + eb, kd_affine_act4)
  depthwise                    9 + 1   (dw_phase: three rows of three nested fmaf, kd_affine_act4)
  project                      Ch + SPLIT_TERMS (+ 1 pbias) + 1     (project_chunk over Ch / 32 chunks, tail_epilogue: acc + bias, kd_affine)
  residual                     + 1     (tail_epilogue: v += res, after the activation)

Terms propagate linearly: through a 1x1 they are multiplied by |W|, through the depthwise conv by |taps|, through an affine they
become t |sc| + |sh|.

Activations.  The deferred first-level input of kd_dw_pw_infer is exact, so act_in of _fp64_conv_ref applies unchanged (its mask
z <= 0 is decided by the inputs).  Every later pre-activation is a ROUNDED intermediate: the clamp is 1-Lipschitz, so the value
is compared as it is, and its terms pass through unmasked except where the float64 value is decided beyond its own bound at that
point of the chain -- 0 where v <= -err(v) (the kernel's value is <= 0 too and clamps to an exact 0), 6 where v >= 6 + err(v)
under ReLU6 (an exact 6 that takes part in later sums).  A mask from v <= 0 alone would not be valid there (act_mid).

`wrong=` evaluates a deliberately wrong reading of the contract, for the negative controls of both suites (WRONGS)."""
from collections import namedtuple

import torch

from _fp64_conv_ref import C_BOUND, U, _out_size, _taps, act_in, relu6_shares, rnd, z32    # noqa: F401  (re-exported)
from _fp64_gemm_ref import SMALLEST_FIRST, SPLIT_TERMS, probe_values, split3               # noqa: F401
from _fp64_tail_ref import _bound, _pad_hw, act

KC = 32                 # hidden channels per chunk (KC in kd_block.hip)
DROPPED_TAP = 5         # (kh, kw) = (1, 2): the right-hand neighbour
WRONGS = {
    "no_res": "the residual omitted",
    "tap": "one depthwise tap dropped",
    "chunk": "the last 32-channel chunk of the hidden tensor dropped",
    "border": "the border padded with act(sh) instead of 0",
    "s2_taps": "stride-2 taps taken from 2*ho + kh instead of 2*ho - 1 + kh",
    "bias_after_bn": "the project bias added after the BatchNorm instead of before it",
    "esh_neighbour": "the expand's BatchNorm shift taken from the neighbouring channel",
}


def act_mid(v, t, n, act_id):
    """(value, terms) of act(v) for a rounded intermediate v with terms t after n roundings"""
    if act_id == 0:
        return v, t
    e = _bound(n, t)
    t = torch.where(v <= -e, torch.zeros_like(t), t)
    if act_id == 2:
        t = torch.where(v >= 6 + e, torch.full_like(t, 6.0), t)
    return act(v, act_id), t


def _tail(a, t, n, fill, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride, wrong, pre):
    """the phases both kernels share, from the activated depthwise input a [B, H, W, Ch] (terms t, n roundings so far; fill: what
    the "border" wrong pads with) to the output [B*Ho*Wo, Cout]"""
    B, H, W, Ch = a.shape
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    ap, tp = _pad_hw(a), _pad_hw(t)
    if wrong == "border":
        ap[:, 0], ap[:, -1], ap[:, :, 0], ap[:, :, -1] = fill, fill, fill, fill
    if wrong == "s2_taps":
        ap, tp = (torch.nn.functional.pad(v[:, 1:, 1:], (0, 0, 0, 1, 0, 1)) for v in (ap, tp))
    y, yt = 0, 0
    for (k, v), (_, vt) in zip(_taps(ap, Ho, Wo, stride), _taps(tp, Ho, Wo, stride)):
        if wrong == "tap" and k == DROPPED_TAP:
            continue
        y, yt = y + v * wd[:, k], yt + vt * wd[:, k].abs()
    n += 9
    if pre is not None:
        pre["d_raw"] = y
    h, ht = act_mid(y * dsc + dsh, yt * dsc.abs() + dsh.abs(), n + 1, dact)
    n += 1
    h, ht = h.reshape(-1, Ch), ht.reshape(-1, Ch)
    if wrong == "chunk":
        h = torch.cat([h[:, :-KC], torch.zeros_like(h[:, -KC:])], 1)
    o, ot = h @ wp.t(), ht @ wp.abs().t()
    n += Ch + SPLIT_TERMS
    if pre is not None:
        pre["p_terms"] = ot
    if pbias is not None and wrong != "bias_after_bn":
        o, ot, n = o + pbias, ot + pbias.abs(), n + 1
    o, ot, n = o * psc + psh, ot * psc.abs() + psh.abs(), n + 1
    if pbias is not None and wrong == "bias_after_bn":
        o, ot, n = o + pbias, ot + pbias.abs(), n + 1
    o, ot = act_mid(o, ot, n, pact)
    if res is not None and wrong != "no_res":
        o, ot, n = o + res, ot + res.abs(), n + 1
    if pre is not None:
        pre["n_seq"] = n
    return o, _bound(n, ot)


def dw_pw_infer(x, isc, ish, iact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride, wrong=None, pre=None):
    """x [B, H, W, Ch] (isc None: as it is, iact ignored), wd [Ch, 9], wp [Cout, Ch], res [B*Ho*Wo, Cout] or None
    -> out [B*Ho*Wo, Cout] = pact((dact(dw3x3(iact(x*isc+ish)) * dsc + dsh) . wp^T + pbias) * psc + psh) + res
    n_seq: (1) + 9 + 1 + Ch + 4 (+ 1) + 1 (+ 1).  pre: a dict that receives the raw depthwise output ("d_raw"),
    the terms of the project sums ("p_terms") and the count of roundings ("n_seq")"""
    a, t = act_in(x, isc, ish, iact)
    fill = act(ish, iact) if isc is not None else 0.0
    return _tail(a, t, int(isc is not None), fill, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride, wrong, pre)


def block_infer(x, we, ebias, esc, esh, eact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride, wrong=None, pre=None):
    """x [B, H, W, Cin] finished values, we [Ch, Cin]: the hidden tensor eact((x . we^T + ebias) * esc + esh), then the tail of
    dw_pw_infer.  n_seq: Cin + 4 (+ 1) + 1 + 9 + 1 + Ch + 4 (+ 1) + 1 (+ 1).  pre also receives "e_raw" (bias included)"""
    if wrong == "esh_neighbour":
        esh = esh.roll(1)
    e, et, n = x @ we.t(), x.abs() @ we.abs().t(), x.shape[-1] + SPLIT_TERMS
    if ebias is not None:
        e, et, n = e + ebias, et + ebias.abs(), n + 1
    if pre is not None:
        pre["e_raw"] = e
    n += 1
    a, t = act_mid(e * esc + esh, et * esc.abs() + esh.abs(), n, eact)
    return _tail(a, t, n, act(esh, eact), wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride, wrong, pre)


# ---- fp32 emulation of the kernels' arithmetic -------------------------------------------------------------------------------

def _fma(a, b, c):
    """fmaf: the exact product and sum rounded once to fp32 (up to a 53 -> 24 bit double rounding)"""
    return (a.double() * b.double() + c.double()).float()


def split_matmul(a, w):
    """a [M, K] . w [N, K]^T in the split arithmetic: three bf16 pieces per operand, K ascending, the six leading piece products
    smallest first, one nearest-rounded fp32 add per piece product"""
    pa, pw = split3(a), split3(w)
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k in range(a.shape[1]):
        for i, j in SMALLEST_FIRST:
            acc = acc + pa[i][:, k, None] * pw[j][None, :, k]
    return acc


def _emulate_tail(a, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride):
    B, H, W, Ch = a.shape
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    v = dict(_taps(_pad_hw(a), Ho, Wo, stride))
    y = torch.zeros(B, Ho, Wo, Ch)
    for kh in range(3):                                                # dw_phase: fmaf(l, w0, fmaf(c, w1, fmaf(r, w2, v))) per row
        for kw in (2, 1, 0):
            y = _fma(v[kh * 3 + kw], wd[:, kh * 3 + kw], y)
    h = act(_fma(y, dsc, dsh), dact).reshape(-1, Ch)
    o = split_matmul(h, wp)
    if pbias is not None:
        o = o + pbias
    o = act(_fma(o, psc, psh), pact)
    return o if res is None else o + res


def emulate_dw_pw(x, isc, ish, iact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride):
    a = x if isc is None else act(_fma(x, isc, ish), iact)
    return _emulate_tail(a, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride)


def emulate_block(x, we, ebias, esc, esh, eact, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride):
    e = split_matmul(x.reshape(-1, x.shape[-1]), we)
    if ebias is not None:
        e = e + ebias
    a = act(_fma(e, esc, esh), eact).reshape(*x.shape[:-1], we.shape[0])
    return _emulate_tail(a, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride)


# ---- the case table ------------------------------------------------------------------------------------------------------------

INST = {                # instance -> (entry point, stride, Cin of the block, Cout)
    "dwpw_s1_32": ("kd_dw_pw_infer", 1, None, 32),
    "dwpw_s1_64": ("kd_dw_pw_infer", 1, None, 64),
    "dwpw_s2_64": ("kd_dw_pw_infer", 2, None, 64),
    "block_s1": ("kd_block_infer", 1, 64, 64),
    "block_s2": ("kd_block_infer", 2, 32, 64),
}
# (H, W, Ch, B) per stride: every map of the tiling (8 x 16 outputs at stride 1, 8 x 8 at stride 2) and every hidden width --
# one chunk, one prefetch, an odd chunk count, the teacher's width -- on every instance, B = 1 and 3
SHAPES = {
    1: [(1, 1, 32, 3), (1, 23, 64, 1), (23, 1, 96, 3), (5, 7, 384, 3), (8, 16, 64, 1), (9, 17, 96, 3), (20, 36, 384, 1)],
    2: [(1, 1, 32, 3), (1, 23, 64, 1), (23, 1, 96, 3), (5, 7, 192, 3), (15, 15, 64, 1), (16, 16, 96, 1), (17, 19, 192, 3)],
}
INPUT_MODES = ("asis", "none", "relu", "relu6")     # kd_dw_pw_infer's input: as it is, or deferred with activation 0 / 1 / 2
ACT_OF = {"asis": 2, "none": 0, "relu": 1, "relu6": 2}                # (as is: the id is passed and must be ignored)

Case = namedtuple("Case", "inst B H W Ch inp dact pact pbias res pad eact ebias")


def _cases():
    out = []
    for j, inst in enumerate(INST):
        fn, stride, _, _ = INST[inst]
        for i, (H, W, Ch, B) in enumerate(SHAPES[stride]):
            out.append(Case(inst, B, H, W, Ch,
                            inp=INPUT_MODES[(i + j) % 4] if fn == "kd_dw_pw_infer" else None,
                            dact=(2, 1)[i % 2], pact=(0, 1)[(i >> 1) % 2], pbias=i % 3 != 0, res=bool(i >> 2), pad=(0, 4)[(i + (i >> 1)) % 2],
                            eact=(1 if i % 3 == 1 else 2) if fn == "kd_block_infer" else None,
                            ebias=i % 2 == 0 if fn == "kd_block_infer" else None))
    return out


CASES = _cases()
# one case per instance for the negative controls: a deferred input / an expand, and a residual
RED = {"dwpw_s1_32": (9, 17), "dwpw_s1_64": (20, 36), "dwpw_s2_64": (16, 16), "block_s1": (9, 17), "block_s2": (17, 19)}


def case_id(c):
    s = f"{c.inst}-{c.B}x{c.H}x{c.W}x{c.Ch}"
    s += f"-in_{c.inp}" if c.inp else f"-eact{c.eact}-ebias{int(c.ebias)}"
    return s + f"-dact{c.dact}-pact{c.pact}-pbias{int(c.pbias)}-res{int(c.res)}-ldo+{c.pad}"


def seed_of(c, exact=False):
    return sum((i + 1) * v for i, v in enumerate((c.B, c.H, c.W, c.Ch))) + 1000 * list(INST).index(c.inst) + int(exact)


def red_case(inst):
    return next(c for c in CASES if c.inst == inst and (c.H, c.W) == RED[inst])


# ---- input recipes -------------------------------------------------------------------------------------------------------------

def affine(g, n, act_id):
    """BatchNorm as (scale, shift): magnitudes 0.5 .. 1.5, about a third of the scales negative; in front of a ReLU6 the shift is
    3 -+ (2.5 + |randn|), the sign alternating over the channels (coeffs of _fp64_conv_ref), so that a visible share of the
    pre-activations lies below 0, inside (0, 6) and above 6"""
    dev = g.device
    sc = (torch.rand(n, generator=g, device=dev) + 0.5) * torch.where(torch.rand(n, generator=g, device=dev) < 0.3, -1.0, 1.0)
    sh = rnd(g, n)
    if act_id == 2:
        sh = 3.0 + (1.0 - 2.0 * (torch.arange(n, device=dev) % 2)) * (2.5 + sh.abs())
    return sc, sh


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g, device=g.device).float()


def _pow2(g, n, e):
    return 2.0 ** e * torch.where(torch.rand(n, generator=g, device=g.device) < 0.3, -1.0, 1.0)


def inputs(g, c, exact=False):
    """the fp32 arguments of case c as a dict keyed by the references' parameter names (+ "stride").  exact: the recipe on which
    every intermediate is exact in fp32 and in the three-piece split -- integers x -4 .. 4 (the deferred input of kd_dw_pw_infer:
    -64 .. 160, so that x 2^-4 + shift spans both clamps; as it is: multiples of 2^-4 in 0 .. 6), we -2 .. 2, wd and wp -4 .. 4,
    biases -8 .. 8, residual -16 .. 16; scales +-2^-4 (expand / deferred input), +-2^-3 (depthwise), +-2^-2 (project); integer
    shifts 0 .. 6 in front of the hidden activations and -4 .. 4 at the end.  Every pre-activation is then a multiple of 2^-7, every
    clamped value has at most 10 significant bits under ReLU6, and every product and partial sum is exact as long as the project
    sums stay below 2^24 units of 2^-7, which the suites assert from the terms of the float64 reference."""
    fn, stride, Cin, Cout = INST[c.inst]
    B, H, W, Ch = c.B, c.H, c.W, c.Ch
    Mo = B * _out_size(H, stride) * _out_size(W, stride)
    d = dict(stride=stride, dact=c.dact, pact=c.pact)
    if fn == "kd_block_infer":
        d["eact"] = c.eact
        if exact:
            d.update(x=_ints(g, -4, 4, B, H, W, Cin), we=_ints(g, -2, 2, Ch, Cin), ebias=_ints(g, -8, 8, Ch), esc=_pow2(g, Ch, -4),
                     esh=_ints(g, 0, 6, Ch))
        else:
            d.update(x=rnd(g, B, H, W, Cin), we=2.0 * rnd(g, Ch, Cin) / Cin ** 0.5, ebias=rnd(g, Ch))
            d["esc"], d["esh"] = affine(g, Ch, c.eact)
        if not c.ebias:
            d["ebias"] = None
    else:
        d["iact"] = ACT_OF[c.inp]
        if exact:
            d.update(x=_ints(g, 0, 96, B, H, W, Ch) / 16.0 if c.inp == "asis" else _ints(g, -64, 160, B, H, W, Ch), isc=_pow2(g, Ch, -4),
                     ish=_ints(g, 0, 6, Ch))
        else:
            d["x"] = (2.0 * rnd(g, B, H, W, Ch) + 2.0).clamp(0, 6) if c.inp == "asis" else 2.0 * rnd(g, B, H, W, Ch)
            d["isc"], d["ish"] = affine(g, Ch, d["iact"])
        if c.inp == "asis":
            d["isc"] = d["ish"] = None
    if exact:
        d.update(wd=_ints(g, -4, 4, Ch, 9), dsc=_pow2(g, Ch, -3), dsh=_ints(g, 0, 6, Ch), wp=_ints(g, -4, 4, Cout, Ch),
                 pbias=_ints(g, -8, 8, Cout), psc=_pow2(g, Cout, -2), psh=_ints(g, -4, 4, Cout), res=_ints(g, -16, 16, Mo, Cout))
    else:
        d.update(wd=rnd(g, Ch, 9) / 3.0, wp=rnd(g, Cout, Ch) / Ch ** 0.5, pbias=rnd(g, Cout), res=rnd(g, Mo, Cout))
        d["dsc"], d["dsh"] = affine(g, Ch, c.dact)
        d["psc"], d["psh"] = affine(g, Cout, c.pact)
    if not c.pbias:
        d["pbias"] = None
    if not c.res:
        d["res"] = None
    return d


TAIL_ARGS = ("wd", "dsc", "dsh", "dact", "wp", "pbias", "psc", "psh", "pact", "res", "stride")
HEAD_ARGS = {"kd_dw_pw_infer": ("x", "isc", "ish", "iact"), "kd_block_infer": ("x", "we", "ebias", "esc", "esh", "eact")}


def _args(c, d):
    return [d[k] for k in HEAD_ARGS[INST[c.inst][0]] + TAIL_ARGS]


def reference(c, d, wrong=None, pre=None):
    """(value, err) of case c on the arguments d (any dtype)"""
    f = dw_pw_infer if INST[c.inst][0] == "kd_dw_pw_infer" else block_infer
    return f(*_args(c, d), wrong=wrong, pre=pre)


def emulate(c, d):
    f = emulate_dw_pw if INST[c.inst][0] == "kd_dw_pw_infer" else emulate_block
    return f(*_args(c, d))


def relu6_operands(c, d, pre):
    """every operand of case c that is activated with ReLU6 as (what, raw fp32, sc, sh), for relu6_shares; pre: filled by the
    float64 reference"""
    if c.inp == "relu6":
        yield "input", d["x"], d["isc"], d["ish"]
    if c.eact == 2:
        yield "expand", pre["e_raw"].float(), d["esc"], d["esh"]
    if c.dact == 2:
        yield "depthwise", pre["d_raw"].float(), d["dsc"], d["dsh"]


def wrongs_of(c):
    """the wrong readings that change case c"""
    w = ["tap", "chunk"]
    if c.res:
        w.append("no_res")
    if c.inp != "asis":
        w.append("border")
    if INST[c.inst][1] == 2:
        w.append("s2_taps")
    if c.pbias:
        w.append("bias_after_bn")
    if c.inp is None:
        w.append("esh_neighbour")
    return w


def to_double(d):
    return {k: v.double() if torch.is_tensor(v) else v for k, v in d.items()}


def exact_headroom(pre):
    """largest project partial sum the exact recipe can meet, in units of 2^-7 (pre: filled by the float64 reference): below 2^24
    every partial sum of the recipe is exact in fp32"""
    return pre["p_terms"].max().item() * 128.0
