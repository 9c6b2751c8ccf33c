"""Float64 references, acceptance rule and launch-layout mirrors for the bf16-storage inference kernels (csrc/kd_bf16.hip and the
NP = 1 instance of csrc/kd_lidar_infer.hip).

Arithmetic model of these kernels: operands are rounded to bf16 once (round to nearest even), a product of two bf16 values is
exact in fp32, accumulation is fp32, the result is rounded to bf16 once.  Every reference evaluates the operation in float64 on
the operands as the kernel sees them (activations / GEMM weights rounded with torch's .bfloat16(); coefficients, biases and the
depthwise / stem / classifier weights in fp32) and returns (value, err): `value` the quantity BEFORE the activation and the final
rounding, `err` the project's bound C_BOUND * n_seq * U * sum|t_i| on its fp32 evaluation (n_seq: products + epilogue operations).

A bf16 output `got` passes iff  rne_bf16(act(value - err) + res) <= got <= rne_bf16(act(value + err) + res)  (interval()):
rounding and the clamp are monotone, so no further constant is needed.  fp32 outputs use |got - value| <= err.  On the exact
inputs of exact_*() (small integers times powers of two: every partial sum is representable, so every evaluation order gives the
same fp32 value) err is irrelevant: the kernel must return rne_bf16(exact) bit for bit -- callers pass err = 0.

The layout mirrors at the end are plain Python copies of the host-side launch arithmetic; the GPU tests assert each ladder case
against them (on_ladder)."""
import math

import torch

from _fp64_tail_ref import C_BOUND, U, act, bilinear_matrix

NONE, RELU, RELU6 = 0, 1, 2
LOOSE_CAP = 0.25        # largest admitted share of outputs whose acceptance interval holds more than one bf16 value


def _bound(n_seq, terms):
    return C_BOUND * n_seq * U * terms


# ---- rounding and acceptance --------------------------------------------------------------------------------------------

def rne_bf16(x):
    """round to nearest even to bf16, returned as float64.  A float64 input is rounded ONCE: going through fp32 first would
    round twice, which differs exactly where the fp32 value lands on a bf16 tie that the float64 value was not on."""
    if x.dtype != torch.float64:
        return x.float().bfloat16().double()
    f = x.float()
    tie = (f.view(torch.int32) & 0xFFFF) == 0x8000
    d = f.double()
    inf = torch.full_like(f, float("inf"))
    f = torch.where(tie & (x > d), torch.nextafter(f, inf), f)
    f = torch.where(tie & (x < d), torch.nextafter(f, -inf), f)
    return f.bfloat16().double()


def trunc_bf16(x):
    """the WRONG rounding (toward zero), for the host test's rejected evaluations"""
    return (x.float().view(torch.int32) & -65536).view(torch.float32).double()


def interval(value, err, act_id=NONE, res=None):
    """(lo, hi): the bf16 values (as float64) a correctly rounded fp32 evaluation may return"""
    r = 0 if res is None else res.double()
    return rne_bf16(act(value - err, act_id) + r), rne_bf16(act(value + err, act_id) + r)


def loose_share(lo, hi):
    return (lo != hi).double().mean().item()


def accept(got, value, err, act_id=NONE, res=None):
    """-> (ok mask, lo, hi) for a bf16 output"""
    lo, hi = interval(value, err, act_id, res)
    g = got.double().reshape(value.shape)
    return (g >= lo) & (g <= hi), lo, hi


def sig_bits_over_8(v):
    """share of values that do not fit 8 significant bits (their rounding to bf16 is a real rounding), and the count of exact ties"""
    r = rne_bf16(v)
    inexact = r != v
    other = 2 * v - r                             # v half way between two neighbours: the mirror image of r is the other neighbour
    ties = inexact & (rne_bf16(other) == other)
    return inexact.double().mean().item(), int(ties.sum())


# ---- exact inputs: every admissible evaluation order gives the same fp32 value -----------------------------------------

def _ints(g, shape, lo, hi, device):
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).double()


def exact_acts(g, shape, amax=8, signed=True, device="cpu"):
    """small integers, exact in bf16 (|a| <= 256)"""
    assert amax <= 256
    return _ints(g, shape, -amax if signed else 0, amax, device).bfloat16()


def exact_weights(g, rows, cols, wmax=4, emin=-3, device="cpu"):
    """[rows, cols] fp32: integers in [-wmax, wmax] times one power of two per row (2^emin .. 2^0), exact in bf16"""
    e = torch.randint(emin, 1, (rows, 1), generator=g, device=device).double()
    return (_ints(g, (rows, cols), -wmax, wmax, device) * torch.pow(2.0, e)).float()


def exact_affine(g, n, smin=-5, smax=0, hmax=3, device="cpu"):
    """(scale, shift): powers of two and integers"""
    sc = torch.pow(2.0, torch.randint(smin, smax + 1, (n,), generator=g, device=device).double()).float()
    return sc, _ints(g, (n,), -hmax, hmax, device).float()


def exact_bias(g, n, bmax=8, device="cpu"):
    return _ints(g, (n,), -bmax, bmax, device).float()


def gemm_amax(K):
    """|a| <= 8, |w| <= 4 at K <= 768 keeps every partial sum far below 2^24 units; short sums take larger integers so that
    they too need more than 8 significant bits"""
    return 8 if K > 128 else 100


def assert_exact(tot, unit, what=""):
    """sum|t_i| in units of the smallest term stays below 2^24: any partial sum of any order is an fp32 number"""
    m = float((tot / unit).max())                                      # unit: a number, or a tensor that broadcasts (one unit per column)
    assert m < 2.0 ** 24, f"{what}: partial sums up to {m:.3g} units are not exactly representable in fp32"


# ---- references ---------------------------------------------------------------------------------------------------------

def _conv_nhwc(x, w, stride, groups):
    """x [B, H, W, Cin] float64, w [Cout, Cin / groups, 3, 3] float64 -> [B, Ho, Wo, Cout], pad 1, as explicit shifted products"""
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    out = 0
    for kh in range(3):
        for kw in range(3):
            v = xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride, :]
            out = out + (v * w[:, 0, kh, kw] if groups > 1 else v @ w[:, :, kh, kw].t())
    return out


def stem(x, w, sc, sh):
    """kd_bf16_stem: x fp32 NCHW, w fp32 [Cout, Cin, 3, 3], 3x3 / stride 2 / pad 1 -> z [B, Ho, Wo, Cout] before the activation.
    Nothing is rounded on the way in.  n_seq = 9 Cin products + the affine."""
    xd, wd, s, h = x.double().permute(0, 2, 3, 1), w.double(), sc.double(), sh.double()
    z, za = _conv_nhwc(xd, wd, 2, 1), _conv_nhwc(xd.abs(), wd.abs(), 2, 1)
    return z * s + h, _bound(9 * x.shape[1] + 1, za * s.abs() + h.abs())


def dwconv(x, w, sc, sh, stride):
    """kd_bf16_dwconv3x3: x bf16 NHWC, w fp32 [C, 1, 3, 3] (not rounded) -> z [B, Ho, Wo, C].  n_seq = 9 + the affine."""
    xd, wd, s, h = x.double(), w.double().reshape(-1, 1, 3, 3), sc.double(), sh.double()
    z, za = _conv_nhwc(xd, wd, stride, x.shape[3]), _conv_nhwc(xd.abs(), wd.abs(), stride, x.shape[3])
    return z * s + h, _bound(10, za * s.abs() + h.abs())


def pwconv(A, W, bias, esc, esh, res=None):
    """kd_bf16_pwconv, epi 0: A [M, K] bf16 (a_kind 0) or fp32 (a_kind 1: rounded on load), W fp32 [N, K] rounded to bf16 when it
    is parked in LDS; bias / esc / esh fp32.  -> z [M, N] before the activation (the residual enters in interval()).
    n_seq = K products + bias add + affine (+ residual add)."""
    a, wb = A.bfloat16().double(), W.bfloat16().double()
    s, h = esc.double(), esh.double()
    acc, tot = a @ wb.t(), a.abs() @ wb.abs().t()
    n = A.shape[1] + 1
    if bias is not None:
        acc, tot, n = acc + bias.double(), tot + bias.double().abs(), n + 1
    tot = tot * s.abs() + h.abs()
    if res is not None:
        tot, n = tot + res.double().abs(), n + 1
    return acc * s + h, _bound(n, tot)


def layer0(pts, l0w, l0b, sc0, sh0, act0):
    """a_kind 3: act0(bn0(layer0(point))) of the 16-byte point, rounded to bf16 -> [M, K] bf16.  The kernel evaluates it as a chain
    of fused multiply-adds; the inputs of these tests are dyadic with few bits, so that every step of that chain is exact and the
    float64 value IS the fp32 value (asserted): the one rounding to bf16 is then unambiguous."""
    z = act((pts.double() @ l0w.double().t() + l0b.double()) * sc0.double() + sh0.double(), act0)
    tot = (pts.double().abs() @ l0w.double().abs().t() + l0b.double().abs()) * sc0.double().abs() + sh0.double().abs()
    assert bool((z.float().double() == z).all()) and float(tot.max()) < 2.0 ** 9, "layer-0 inputs must keep the fma chain exact"
    assert bool(((tot * 2.0 ** 15) == (tot * 2.0 ** 15).round()).all()), "layer-0 inputs must be multiples of 2^-15"
    return z.float().bfloat16()


def scatter_max(v, e, cell, ncells):
    """per-cell maximum of the per-point values v [M, N] >= 0 (rows with cell < 0 skipped); bound: the largest per-point bound in
    the cell; a cell without a point: value 0, bound 0 (exactly 0 required)."""
    keep = cell >= 0
    idx = cell[keep].long()[:, None].expand(-1, v.shape[1])
    zero = torch.zeros(ncells, v.shape[1], dtype=torch.float64, device=v.device)
    val = zero.scatter_reduce(0, idx, v[keep], "amax")
    err = zero if e is None else zero.scatter_reduce(0, idx, e[keep], "amax")
    return val, err


def pwconv_scatter(A, W, bias, esc, esh, act_id, cell, ncells):
    """kd_bf16_pwconv, epi 4: act(z) per point (fp32, not rounded), then the per-cell maximum"""
    z, e = pwconv(A, W, bias, esc, esh)
    return scatter_max(act(z, act_id), e, cell, ncells)


def lidar_encoder(pts, cell, ncells, l0, l1, l2, exact=False):
    """kd_bf16_lidar_mlp_scatter: layer 0 (fp32 -> bf16) -> layer 1 (bf16 GEMM, ReLU, rounded to bf16 in registers) -> layer 2 ->
    scatter-max (fp32).  l0 = (w0 [64, 4], b0, sc0, sh0), l1 / l2 = (W, bias, sc, sh).  Where the acceptance interval of a layer-1
    activation holds two bf16 values, that one-step uncertainty enters the layer-2 bound linearly, weighted by |W2_bf16|."""
    a0 = layer0(pts, *l0, RELU)
    z1, e1 = pwconv(a0, *l1)
    if exact:
        e1 = torch.zeros_like(e1)
    lo1, hi1 = interval(z1, e1, RELU)
    a1 = rne_bf16(act(z1, RELU))
    d1 = torch.maximum(hi1 - a1, a1 - lo1)
    W2, b2, sc2, sh2 = l2
    z2, e2 = pwconv(a1.bfloat16(), W2, b2, sc2, sh2)
    e2 = torch.maximum(e2, pwconv(hi1.bfloat16(), W2, b2, sc2, sh2)[1])         # sum|t| with the larger admissible activations
    e2 = e2 + (d1 @ W2.bfloat16().double().abs().t()) * sc2.double().abs()
    if exact:
        assert float(d1.max()) == 0
        e2 = torch.zeros_like(e2)
    return scatter_max(act(z2, RELU), e2, cell, ncells)


def lidar_encoder_fp32(pts, cell, ncells, l0, l1, l2):
    """the same encoder on the fp32 operands, nothing rounded (kd_lidar_mlp_scatter_infer, split arithmetic): the float64 map"""
    a = act((pts.double() @ l0[0].double().t() + l0[1].double()) * l0[2].double() + l0[3].double(), RELU)
    for W, b, sc, sh in (l1, l2):
        a = act((a @ W.double().t() + b.double()) * sc.double() + sh.double(), RELU)
    return scatter_max(a, None, cell, ncells)[0]


def bilinear_sum(ins, Ho, Wo):
    """kd_bf16_bilinear_sum: ins = [x bf16 [B, Hi, Wi, C]]; the kernel's own fp32 interpolation coefficients (bilinear_matrix);
    n_seq = 6 per input (two lambda products, two adds, the row blend, the add into the sum)"""
    val = tot = 0
    for x in ins:
        xd = x.double()
        mh = bilinear_matrix(x.shape[1], Ho, device=x.device)
        mw = bilinear_matrix(x.shape[2], Wo, device=x.device)
        val = val + torch.einsum("pw,bowc->bopc", mw, torch.einsum("oh,bhwc->bowc", mh, xd))
        tot = tot + torch.einsum("pw,bowc->bopc", mw, torch.einsum("oh,bhwc->bowc", mh, xd.abs()))
    return val, _bound(6 * len(ins), tot)


def cls_conv(x, w, b, B):
    """kd_bf16_cls_conv: x bf16 [M, Cin], w fp32 [NC, Cin] (not rounded), b [NC] -> fp32 logits [B, NC, HW]; n_seq = Cin + 1"""
    xd, wd, bd = x.double(), w.double(), b.double()
    r, ra = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    nchw = lambda t: t.reshape(B, -1, t.shape[1]).permute(0, 2, 1).contiguous()
    return nchw(r), nchw(_bound(x.shape[1] + 1, ra))


def weighted_tail(h, cat, w2, b2):
    """kd_bf16_weighted_tail: h bf16 [M, C] (ReLU'd attention.0 output), cat bf16 [M, 2C] (the two projections), w2 fp32 [2, C],
    b2 [2] -> out [M, C] before its rounding.  The softmax treatment of _fp64_tail_ref.weighted_fuse_fwd: the logits' bound enters the
    weights through d w0 = w0 w1 (d a0 - d a1), the weights' bound enters the output linearly."""
    C = h.shape[1]
    hd, w2d, b2d = h.double(), w2.double(), b2.double()
    cp, lp = cat[:, :C].double(), cat[:, C:].double()
    a = hd @ w2d.t() + b2d
    sa = hd.abs() @ w2d.abs().t() + b2d.abs()
    e = torch.exp(a - a.max(1, keepdim=True).values)
    w = e / e.sum(1, keepdim=True)
    ea = _bound(C + 2, sa + a.abs().amax(1, keepdim=True))
    ew = w[:, :1] * w[:, 1:] * ea.sum(1, keepdim=True) + _bound(4, w)
    out = cp * w[:, :1] + lp * w[:, 1:]
    return out, cp.abs() * ew[:, :1] + lp.abs() * ew[:, 1:] + _bound(3, cp.abs() * w[:, :1] + lp.abs() * w[:, 1:])


# ---- the GEMM shapes of tests/test_gpu_bf16_kernels.py (the host test checks LOOSE_CAP for each) -----------------------------
# second form, (K, N, residual): every K instance; N chosen for many column tiles = a small grid cap = a short turn
V2_CASES = [(32, 736, False), (64, 736, False), (128, 768, False), (192, 768, False), (256, 768, False), (384, 768, False),
            (512, 768, False), (768, 768, False), (32, 384, True), (64, 768, True), (128, 768, True), (384, 768, True), (768, 768, True)]
# with a residual: NB = 1 (K = 32: four slabs per unit), 2 (K = 64; K = 768 on the LDS budget) and 4 (K = 128, 384: the full
# 32-register residual tile held across the prefetch of the next unit)
# first form (a device-side row count selects it): NB = 4, 2, 1
V1_CASES = [(64, 768, False), (64, 704, True), (64, 736, False), (96, 736, True)]
TAIL_KN = [(8, 8), (40, 16), (48, 24), (24, 40), (72, 48), (104, 72), (16, 104)]  # K past a multiple of 32 by 8 / 16 / 24, last tile of 8 / 16 / 24 columns
A1_CASES = [(128, 704), (40, 72)]                     # a_kind 1 (fp32 A rounded on load): NB = 2 and a TAIL shape


# second form, single-unit launches (M, K, N, residual): M = 1, one row more than a unit, small N
SMALL_CASES = [(1, 32, 32, False), (31, 128, 768, False), (130, 32, 32, True), (64, 64, 96, False), (777, 64, 64, True), (129, 192, 64, True),
               (257, 512, 128, True), (33, 256, 32, False), (300, 256, 128, True)]
LIDAR_KN = [(64, 128), (128, 128)]                   # the two launches of the LiDAR encoder (a_kind 3, epi 4)


def all_kn():
    """every (K, N) tests/test_gpu_bf16_kernels.py runs a GEMM with random inputs at"""
    return sorted({(k, n) for k, n, _ in V2_CASES + V1_CASES} | {(k, n) for _, k, n, _ in SMALL_CASES} | set(TAIL_KN) | set(A1_CASES) | set(LIDAR_KN))


# ---- random inputs that keep the intervals tight ------------------------------------------------------------------------

def random_gemm_inputs(g, M, K, N, device, lda=None, fp32_a=False):
    """non-negative activations (as after ReLU) and weights with a non-zero mean: sum|t| / |value| stays small, so few intervals hold
    a second bf16 value (LOOSE_CAP).  The epilogue keeps a good part of the outputs inside (0, 6)."""
    rnd = lambda *s: torch.randn(*s, generator=g, device=device)
    A = torch.full((M, lda or K), float("nan"), device=device)
    A[:, :K] = rnd(M, K).abs()
    W = rnd(N, K) * 0.1 + 0.25
    bias, esc, esh = rnd(N) * 0.5, (rnd(N).abs() + 0.5) * (8.0 / K), rnd(N) * 0.3 + 1.0
    return (A if fp32_a else A.bfloat16()), W, bias, esc, esh


def exact_gemm_inputs(g, M, K, N, device, lda=None, fp32_a=False, relu6=False):
    """relu6: scales small enough (still powers of two) to leave a good part of the outputs inside (0, 6), where they are rounded"""
    A = torch.full((M, lda or K), float("nan"), device=device, dtype=torch.bfloat16)
    A[:, :K] = exact_acts(g, (M, K), gemm_amax(K), device=device)
    W = exact_weights(g, N, K, device=device)
    esc, esh = exact_affine(g, N, *((-12, -9) if relu6 else (-5, 0)), device=device)
    return (A.float() if fp32_a else A), W, exact_bias(g, N, device=device), esc, esh


def lidar_params(g, P, exact, device="cpu"):
    """dyadic points and layer 0 (multiples of 2^-4: the fma chain is exact); random or exact layers 1 and 2"""
    q = 1.0 if exact else 16.0
    pts = _ints(g, (P, 4), -3 * int(q), 3 * int(q), device).float() / q
    l0 = ((_ints(g, (64, 4), -2 * int(q), 2 * int(q), device) / q).float(), (_ints(g, (64,), -2, 2, device)).float(),
          torch.ones(64, device=device), _ints(g, (64,), 0, 2, device).float())
    if exact:
        l1 = (_ints(g, (128, 64), -1, 4, device).float(), exact_bias(g, 128, device=device), torch.ones(128, device=device),
              _ints(g, (128,), -3, 3, device).float())
        l2 = (_ints(g, (128, 128), -2, 2, device).float(), exact_bias(g, 128, device=device), *exact_affine(g, 128, -8, -4, device=device))
    else:
        rnd = lambda *s: torch.randn(*s, generator=g, device=device)
        l1 = (rnd(128, 64) * 0.1 + 0.05, rnd(128) * 0.2, rnd(128).abs() * 0.1 + 0.1, rnd(128) * 0.2 + 0.3)
        l2 = (rnd(128, 128) * 0.1 + 0.05, rnd(128) * 0.2, rnd(128).abs() * 0.05 + 0.05, rnd(128) * 0.2 + 0.3)
    return l0, l1, l2, pts


def cell_pattern(P, ncells, n_skip=0, device="cpu"):
    """cells as kd_lidar_sort_points leaves them: ascending, runs of equal cells of lengths 1, 2, 3, 5, 31, 33, 4, 70, ... (single
    points; runs that cross a quad, a half wave -- 4 rows of a lane's quad, 8 rows later -- and a 32-row slab), cells in between
    left empty, then `n_skip` rows with cell < 0.  Needs ncells >= 2 * number of runs."""
    runs = [1, 1, 2, 3, 5, 1, 31, 33, 4, 70, 1, 7, 9, 64, 2, 6]
    out, c, i, n = [], 0, 0, P - n_skip
    while n > 0:
        r = min(runs[i % len(runs)], n)
        out.append(torch.full((r,), c, dtype=torch.int32))
        n -= r; i += 1
        c += 1 if i % 3 else 2                                          # every third cell index is skipped: an empty cell
        if c >= ncells:
            c = ncells - 1
    out.append(torch.full((n_skip,), -1, dtype=torch.int32))
    return torch.cat(out).to(device)


# ---- layout mirrors (the host-side launch arithmetic of kd_bf16.hip / kd_lidar_infer.hip) ------------------------------------

BW = 8                       # waves per workgroup of both GEMM forms and of the LiDAR kernel
V2_K = (32, 64, 128, 192, 256, 384, 512, 768)


def _walk(kernel, rows, unit, grid, cap, **kw):
    """a walk over units of `unit` rows, one per wave and turn; `full`: the units of one turn of the capped grid"""
    units = -(-rows // unit)
    per_turn = grid * BW
    return dict(kernel=kernel, rows=rows, unit=unit, units=units, grid=grid, per_turn=per_turn, iters=-(-units // per_turn), full=cap * BW, **kw)


def gemm_v1_layout(M, K, N):
    """first form: pw_gemm_bf16_kernel<NB, ., ., TAIL>; one wave takes one 32-row slab per turn"""
    tail = K % 32 != 0 or N % 32 != 0
    if tail:
        NB = 1
    elif N % 128 == 0 and 128 * K * 2 <= 96 * 1024:
        NB = 4
    elif N % 64 == 0 and 64 * K * 2 <= 96 * 1024:
        NB = 2
    else:
        NB = 1
    ntiles = -(-N // (32 * NB))
    cap = max(1, 256 // ntiles)
    return _walk(f"pw_gemm_bf16_kernel<{NB}{', TAIL' if tail else ''}>", M, 32, min(-(-M // 256), cap), cap, NB=NB, ntiles=ntiles, tail=tail)


def gemm_v2_layout(M, K, N, res=False, a_kind=0, epi=0, m_dev=False, ldc=None):
    """second form: pw_gemm_bf16_v2_kernel<NB, K / 16, RES>, or None where the first form runs"""
    ldc = N if ldc is None else ldc
    if a_kind != 0 or epi != 0 or m_dev or K not in V2_K or N % 32 != 0 or ldc % 8 != 0:
        return None
    SL = max(1, 128 // K)
    for NB in (4, 2, 1):
        if N % (32 * NB) != 0:
            continue
        if 32 * NB * K * 2 + BW * 32 * (64 * min(NB, 2) + 16) > 160 * 1024:
            continue
        if res and SL * NB * 8 > 32:
            continue
        ntiles = N // (32 * NB)
        cap = max(1, 256 // ntiles)
        return _walk(f"pw_gemm_bf16_v2_kernel<{NB}, {K // 16}, {'RES' if res else 'no RES'}>", M, 32 * SL, min(-(-M // (32 * SL * BW)), cap), cap,
                     NB=NB, ntiles=ntiles, SL=SL)
    return None


def gemm_ladder(unit, cap):
    """row counts over units of `unit` rows, `cap` workgroups of 8 waves per turn"""
    full = cap * BW
    return {"few": 5, "partial": 3 * unit + unit // 2 + 1, "full-1": (full - 1) * unit, "full": full * unit, "full+1": full * unit + 1,
            "ragged": (2 * full + full // 3) * unit + 5}


def on_ladder(name, wk, what=""):
    """the walk is what the ladder name says (units of a GEMM / LiDAR walk, items of a cg8 / per-pixel walk): one turn up to `full`
    (the capped grid), a second turn of one unit, a ragged third turn"""
    u, full, it, slots = wk["units"], wk["full"], wk["iters"], wk.get("slots", 1)
    ok = {"few": it == 1 and u <= max(1, slots), "partial": it == 1 and u < full and wk["rows"] % wk["unit"] != 0,
          "partial_block": it == 1 and slots < u < full, "full-1": it == 1 and u == full - 1,
          "full": it == 1 and u == full and wk["per_turn"] == full, "full+1": it == 2 and u == full + 1 and wk["per_turn"] == full,
          "ragged": it == 3 and u % full != 0 and wk["per_turn"] == full}[name]
    assert ok, f"not a '{name}' walk: {wk} {what}"


def cg8_layout(items, C):
    """(groups, slots, grid): C / 8 lanes share an item, 256 / groups items per block, at most 2048 blocks"""
    groups = C // 8
    slots = max(1, 256 // groups)
    return groups, slots, max(1, min(-(-items // slots), 2048))


def _item_walk(kernel, items, slots, grid, cap):
    per_turn = grid * slots
    return dict(kernel=kernel, rows=items, unit=1, units=items, slots=slots, grid=grid, per_turn=per_turn, iters=-(-items // per_turn),
                full=cap * slots)


def dw_layout(B, H, W, C, stride):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if stride == 1 and Ho % 16 == 0:
        kernel, nseg = "dw_bf16_s1_pipe_kernel<16>", Ho // 16
    elif stride == 1 and Ho % 8 == 0:
        kernel, nseg = "dw_bf16_s1_pipe_kernel<8>", Ho // 8
    else:
        kernel, nseg = f"dw_bf16_kernel<{stride}>", -(-Ho // 16)
    items = B * nseg * Wo
    _, slots, grid = cg8_layout(items, C)
    return dict(_item_walk(kernel, items, slots, grid, 2048), nseg=nseg)


def bilinear_layout(B, Ho, Wo, C):
    _, slots, grid = cg8_layout(B * Ho * Wo, C)
    return _item_walk("bilinear_sum_bf16_kernel", B * Ho * Wo, slots, grid, 2048)


def pixel_layout(kernel, npix):
    """stem and classifier: one pixel per thread, 256 per block, at most 4096 blocks"""
    return _item_walk(kernel, npix, 256, max(1, min(-(-npix // 256), 4096)), 4096)


def stem_layout(B, Cin, H, W, Cout):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return pixel_layout(f"stem_bf16_v2_kernel<3, {Cout}>" if Cin == 3 else f"stem_bf16_kernel<{Cout}>", B * Ho * Wo)


def weighted_tail_layout(M, C):
    slots = 256 // (C // 8)
    return _item_walk("weighted_tail_bf16_kernel", M, slots, max(1, min(-(-M // slots), 4096)), 4096)


def lidar_layout(P, NP=1):
    """32 points per wave, 8 waves, at most 256 blocks: one turn is 65 536 points"""
    nslab = -(-P // 32)
    return _walk(f"lidar_mlp_scatter_infer_kernel<{NP}>", P, 32, min(-(-nslab // BW), 256), 256)


def bhw(n):
    """n = B * H * W with a small B and a map as square as the count allows"""
    for B in (3, 5, 2, 7, 1):
        if n % B == 0:
            m = n // B
            H = max(h for h in range(1, int(math.isqrt(m)) + 1) if m % h == 0)
            return B, H, m // H
    raise AssertionError
