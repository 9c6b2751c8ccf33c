"""Float64 references for the 1x1-convolution GEMM family -- pw_gemm_kernel / pw_wgrad_kernel (csrc/kd_gemm.hip), pw_stream_kernel
(csrc/kd_gemm_stream_kernel.h) and pw_wgrad_rs_kernel (csrc/kd_wgrad_rs.hip) -- with the rounding-error bound each kernel output
must meet, mirrors of the launch layouts that decide the length of the reduction chains, and an fp32 emulation of the split
(bf16 x 3) product.  Same conventions as tests/_fp64_conv_ref.py: every function takes the kernel's fp32 inputs (any device;
evaluated in the inputs' dtype -- float64 for the truth, float32 for the self-check of the bound) and returns
{name: (value, err)} with

    err = C_BOUND * n_seq * U * sum |t_i|

`sum |t_i|` evaluated alongside the value.  n_seq, counted from the kernel source, is written next to each output:

  operand transforms   pro 1 / a_mode 1: kd_affine is one fma (1; the clamp is exact).  pro 2 / d_mode 2: kd_bwd_operand is
                       fmaf(al, g, fmaf(be, x, ga)) with g = d * mask exact (2).  A transformed operand is a rounded
                       intermediate multiplied by a weight: its bound enters linearly, as its terms times |W| under the same n_seq.
  reduction            one accumulation per element of the reduction (K for the forward and the data gradient; the rows a
                       matrix wave walks for the weight gradient).  v_mfma_f32_32x32x2_f32 is an fma chain of 2, the split form
                       issues six v_mfma_f32_32x32x16_bf16 per 16 elements, each adding 16 exact piece products to the fp32
                       accumulator; how that instruction rounds inside is not documented -- one rounding per instruction would be
                       6K/16 accumulations, one per piece product 6K -- and the count used here is K for both arithmetics.
  split products       + SPLIT_TERMS = 4: the six leading piece products represent x*y to 3.97 U |x||y| (include/kd_hip.h, rounded
                       up; the probe of tests/test_gpu_gemm_fp64.py measures it on single products).  Counted in both arithmetics:
                       one bound.
  epilogue             + 1 for the addend, + 1 for the bias, + 1 for the eval BatchNorm fma of epi 5 (its residual: the addend's
                       + 1, after the activation); the epi 2 mask is an exact 0 / 1 factor.
  statistics           s1 = sum v: + n_part; s2 = sum v^2 (epi 1): 2 n + 1 + n_part (|v| <= terms, so the bound of v^2 is
                       (2 n + 1) U terms^2); s2 = sum v * xhat (epi 2): n + 2 + n_part (xhat = (x - mean) * invstd, two
                       roundings, the product and the add are one fma).  n_part = the accumulations of one thread + the
                       partial sums a workgroup adds up (tiled_layout / stream_layout); the slab rows are summed in float64 by
                       the test.
  weight gradient      operand roundings + SPLIT_TERMS + n_red, n_red = rows of a matrix wave's chain + the cross-wave adds + slab rows +
                       SLAB_SPLIT (kd_slab_reduce_launch sums the slab in fp32): wgrad_tiled_layout / wgrad_rs_layout.

Masks: every mask is taken from z rounded ONCE to fp32 (mask32 of _fp64_conv_ref), whatever dtype the rest is evaluated in, so
no element is left out of any comparison."""
import torch

from _fp64_conv_ref import (C_BOUND, SLAB_SPLIT, U, act_in, coeffs, dyeff, folded, mask32, relu6_shares, rnd,  # noqa: F401
                            z32)
from _fp64_tail_ref import _bound, act

NT_BYTES = 64 << 20     # kd_nt_store: an output of at least this many bytes is stored with the non-temporal hint
SW = 8                  # waves of a streaming workgroup
STREAM_TR = 32 * 36     # floats of a wave's transposition tile
LDS_MAX = 160 * 1024
SPLIT_TERMS = 4         # the documented per-product error of the split arithmetic in units of U |x||y|, rounded up


def _cdiv(a, b):
    return -(-a // b)


# ---- launch layouts (mirrors of kd_gemm.hip, kd_gemm_stream.hip, kd_wgrad_rs.hip; the GPU suite asserts them equal to the
# library's answers: kd_pwconv_stat_rows_for, kd_pwconv_wgrad_ws_bytes) --------------------------------------------------------

def tiled_layout(M, N, pro=0):
    """gemm_launch's tiled form: 256 x 64 tiles when the last column tile would be at most 64 wide, else 128 x 128; one slab row per
    128 matrix rows (a tall tile fills row 2 b and zeroes row 2 b + 1).  A thread adds 2 halves x 8 rows, then `rg` row groups
    are added through LDS."""
    tall = pro != 4 and (N - 1) % 128 < 64
    bm, bn = (256, 64) if tall else (128, 128)
    rg = 256 // (bn // 4)
    return dict(form="tiled", tall=tall, bm=bm, bn=bn, rows=_cdiv(M, 128), n_part=16 + rg)


def stream_lds_bytes(K, N, pro):
    nco = {1: 2, 3: 7, 2: 5, 4: 5}.get(pro, 0)
    return 3 * N * K * 2 + max(nco, 1) * K * 4 + 8 * STREAM_TR * 4


def stream_cfg(K, N, pro, epi, add):
    """stream_cfg of kd_gemm_stream.hip in mode 2 (every covered shape) for pro 0 / 1 / 2 and the table-form data gradient of the
    LiDAR branch (pro 4, epi 2: one instance, 128 -> 128) -> (kb, nb, ntiles) or None"""
    if K % 32 or N % 32:
        return None
    kb, nbt = K // 32, N // 32
    fwd = pro in (0, 1) and epi in (0, 1, 5)
    bwd = (pro == 2 and epi in (0, 2)) or (pro == 4 and epi == 2 and kb == 4 and nbt == 4)
    if not (fwd or bwd) or kb not in (1, 2, 4):
        return None
    nb = next((c for c in (4, 2, 1) if nbt % c == 0 and stream_lds_bytes(K, 32 * c, pro) <= LDS_MAX), 0)
    if nb == 0:
        return None
    if pro == 2 and epi == 2 and kb * 100 + nb * 10 + int(bool(add)) in (120, 141, 211, 220, 241, 411, 420, 441):
        return None
    if pro == 2 and epi == 0 and kb == 4 and nb == 2:
        return None
    ntiles = nbt // nb
    if (ntiles > 2 and ntiles * K > 2 * N) or ntiles > 8:
        return None
    return kb, nb, ntiles


def stream_grid(M, ntiles):
    return min(_cdiv(M, 32 * SW), max(1, 256 // ntiles))


def stream_layout(M, K, N, pro, epi, add):
    """the streaming launch, or None: one slab row per workgroup; wave w of the launch owns the 32-row slabs w, w + W, ...; a lane
    adds 16 rows per slab in registers across its slabs, then its other half wave (1), then the 8 waves are added through LDS"""
    cfg = stream_cfg(K, N, pro, epi, add)
    if cfg is None:
        return None
    kb, nb, ntiles = cfg
    grid = stream_grid(M, ntiles)
    per_wave = _cdiv(_cdiv(M, 32), grid * SW)
    return dict(form="stream", kb=kb, nb=nb, ntiles=ntiles, grid=grid, rows=grid, slabs_per_wave=per_wave,
                n_part=16 * per_wave + 1 + SW)


def gemm_layout(M, K, N, pro, epi, add, form):
    """the layout of the launch kd_pwconv_gemm makes under kd_set_gemm_stream(0) ("tiled") / (2) in split arithmetic ("stream")"""
    lay = stream_layout(M, K, N, pro, epi, add) if form == "stream" else None
    return lay if lay is not None else tiled_layout(M, N, pro)


def slab_row_of(M, lay, device="cpu"):
    """the statistics-slab row each matrix row is summed into"""
    m = torch.arange(M, device=device)
    if lay["form"] == "stream":
        return ((m // 32) % (lay["grid"] * SW)) // SW
    return (m // lay["bm"]) * (lay["bm"] // 128)


def wgrad_tiled_layout(M, N, K, split):
    """wgrad_launch / launch_wgrad<WN, WK, WM>: output tiles of 64 WN x 64 WK, WM waves share the rows of a chunk (each walks
    rows_per_split / WM of them), WM - 1 cross-wave adds, nsplit slab rows"""
    wn, wk = (2 if N > 64 else 1), (2 if K > 64 else 1)
    wm = 4 // (wn * wk)
    ch = 16 * wm * (2 if wm == 1 else 1) if split else 32 * wm
    ntiles = _cdiv(N, 64 * wn) * _cdiv(K, 64 * wk)
    nsplit0 = _cdiv(512, ntiles)
    chunks = _cdiv(M, ch)
    nsplit = max(1, min(nsplit0, chunks))
    rps = _cdiv(chunks, nsplit) * ch
    nsplit = _cdiv(M, rps)
    return dict(form="tiled", wn=wn, wk=wk, wm=wm, ch=ch, ntiles=ntiles, nsplit=nsplit, rows_per_split=rps,
                ws_bytes=nsplit0 * N * K * 4, n_red=_cdiv(rps, wm) + (wm - 1) + nsplit + SLAB_SPLIT)


_RS_TAB = {(6, 1): (3, 1, 2, 1, 2), (12, 2): (3, 2, 4, 1, 1), (8, 4): (2, 4, 4, 1, 1), (2, 6): (1, 3, 2, 2, 2),
           (4, 12): (1, 12, 4, 1, 1), (4, 4): (2, 2, 2, 2, 2), (4, 2): (2, 1, 2, 2, 2), (2, 4): (1, 2, 2, 2, 2),
           (4, 8): (2, 4, 2, 2, 1), (2, 8): (1, 4, 2, 2, 2)}


def rs_plan(N, K):
    """rs_plan of kd_wgrad_rs.hip with every instance enabled (kd_set_wgrad_rs(2)) -> dict or None"""
    if N % 32 or K % 32:
        return None
    nb, kb, ncs, split_n = N // 32, K // 32, 1, 0
    if nb == 24:
        nb, ncs, split_n = 8, 3, 1
    elif kb == 24 and nb == 4:
        kb, ncs = 12, 2
    elif kb == 24:
        kb, ncs = 6, 4
    elif kb == 12 and nb == 4:
        pass
    elif kb == 12 and nb <= 4:
        kb, ncs = 6, 2
    elif nb == 8 and kb == 8:
        nb, ncs, split_n = 4, 2, 1
    e = _RS_TAB.get((nb, kb))
    if e is None:
        return None
    return dict(tnw=e[0], tkw=e[1], wn=e[2], wk=e[3], chk=e[4], ncs=ncs, split_n=split_n)


def _rs_slices(M, p):
    return max(1, min(256 // p["ncs"], _cdiv(M, 16 * p["chk"]) // 8))


def wgrad_rs_layout(M, N, K):
    """the role-specialised launch, or None: a matrix wave keeps its accumulator tiles for the whole row slice (rows_per_slice
    accumulations), nrs slab rows"""
    p = rs_plan(N, K)
    if p is None:
        return None
    ch = 16 * p["chk"]
    nrs0 = _rs_slices(M, p)
    rps = _cdiv(_cdiv(M, ch), nrs0) * ch
    nrs = _cdiv(M, rps)
    return dict(form="rs", ch=ch, nrs=nrs, rows_per_slice=rps, ws_bytes=nrs0 * N * K * 4, n_red=rps + nrs + SLAB_SPLIT, **p)


def wgrad_ws_bytes(M, N, K):
    """kd_pwconv_wgrad_ws_bytes: the larger of the two forms, whatever the arithmetic and the switches"""
    rs = wgrad_rs_layout(M, N, K)
    return max(wgrad_tiled_layout(M, N, K, True)["ws_bytes"], rs["ws_bytes"] if rs else 0)


def wgrad_layout(M, N, K, form, split=True):
    lay = wgrad_rs_layout(M, N, K) if form == "rs" and split else None
    return lay if lay is not None else wgrad_tiled_layout(M, N, K, split)


# ---- input recipes (shared by the GPU suite and the CPU self-check of the bounds) ---------------------------------------------

def fwd_inputs(g, M, K, N):
    """A [M, K], W [N, K], bias, addend [M, N]; sc / sh [K] and esc / esh [N] per activation id"""
    d = dict(A=rnd(g, M, K), W=rnd(g, N, K) / K ** 0.5, bias=rnd(g, N), addend=rnd(g, M, N))
    d["pro"] = {a: coeffs(g, K, a)[:2] for a in (1, 2)}
    d["epi"] = {a: coeffs(g, N, a)[:2] for a in (0, 1, 2)}
    return d


def dgrad_inputs(g, M, Kred, Nout):
    """G, Y [M, Kred] (upstream gradient, raw conv output), Wt [Nout, Kred], X, addend [M, Nout]; (al, be, ga), the mask's
    (msc, msh) [Kred] and (esc, esh, mean, invstd) [Nout] per activation id"""
    d = dict(G=rnd(g, M, Kred), Y=rnd(g, M, Kred), Wt=rnd(g, Nout, Kred) / Kred ** 0.5, X=rnd(g, M, Nout),
             addend=rnd(g, M, Nout), fold=folded(g, Kred))
    d["pro"] = {a: coeffs(g, Kred, a)[:2] for a in (1, 2)}
    d["epi"] = {a: coeffs(g, Nout, a) for a in (0, 1, 2)}
    return d


def wgrad_inputs(g, M, N, K):
    """D, X [M, N], A [M, K]; (al, be, ga), (msc, msh) [N] and (asc, ash) [K] per activation id"""
    d = dict(D=rnd(g, M, N), X=rnd(g, M, N), A=rnd(g, M, K), fold=folded(g, N))
    d["d"] = {a: coeffs(g, N, a)[:2] for a in (0, 1, 2)}
    d["a"] = {a: coeffs(g, K, a)[:2] for a in (0, 1, 2)}
    return d


def fwd_cases(inp):
    """(name, gemm_fwd keywords): pro {0, 1} x pro_act {1, 2} x bias x addend x epi {0, 1, 5 with epi_act 0 / 1 / 2}"""
    for pro, pa in ((0, 0), (1, 1), (1, 2)):
        sc, sh = inp["pro"].get(pa, (None, None))
        for bias in (None, inp["bias"]):
            for add in (None, inp["addend"]):
                for epi, ea in ((0, 0), (1, 0), (5, 0), (5, 1), (5, 2)):
                    esc, esh = inp["epi"][ea]
                    yield (f"pro={pro} pro_act={pa} bias={bias is not None} addend={add is not None} epi={epi} epi_act={ea}",
                           dict(pro=pro, pro_act=pa, sc=sc, sh=sh, bias=bias, addend=add, epi=epi, esc=esc, esh=esh, epi_act=ea))


def dgrad_cases(inp):
    """(name, gemm_dgrad keywords): mask ReLU / ReLU6 / off x addend x epi {0, 2 with epi_act 0 / 1 / 2}"""
    al, be, ga = inp["fold"]
    for pa in (1, 2, 0):
        msc, msh = inp["pro"].get(pa, (None, None))
        for add in (None, inp["addend"]):
            for epi, ea in ((0, 0), (2, 0), (2, 1), (2, 2)):
                esc, esh, mean, inv = inp["epi"][ea]
                yield (f"mask={pa} addend={add is not None} epi={epi} epi_act={ea}",
                       dict(al=al, be=be, ga=ga, msc=msc, msh=msh, pro_act=pa, addend=add, epi=epi, X=inp["X"], esc=esc, esh=esh,
                            mean=mean, invstd=inv, epi_act=ea))


def wgrad_cases(inp):
    """(name, gemm_wgrad arguments after D, X and before n_red): d_mode {0, 2} x d_act {0, 1, 2} x a_mode {0, 1} x a_act {0, 1, 2}
    (mode 0 must ignore its activation id)"""
    al, be, ga = inp["fold"]
    for dm, da in ((m, a) for m in (0, 2) for a in (0, 1, 2)):
        for am, aa in ((m, a) for m in (0, 1) for a in (0, 1, 2)):
            msc, msh = inp["d"][da]
            asc, ash = inp["a"][aa]
            yield f"d_mode={dm} d_act={da} a_mode={am} a_act={aa}", (al, be, ga, msc, msh, dm, da, inp["A"], asc, ash, am, aa)


def probe_values(g, *shape):
    """fp32 values with full 24-bit random mantissas, exponents -8 .. 8 and random signs"""
    m = torch.randint(1 << 23, 1 << 24, shape, generator=g, device=g.device).double()
    e = torch.randint(-8, 9, shape, generator=g, device=g.device).double()
    s = 1.0 - 2.0 * torch.randint(0, 2, shape, generator=g, device=g.device).double()
    return (s * m * 2.0 ** (e - 23)).float()


# ---- references ------------------------------------------------------------------------------------------------------------

def _stats(v, vt, w, n1, n2, rowsel):
    """(s1, s2) = (sum v, sum v * w) over the rows `rowsel` covers; w's terms are |w|"""
    if rowsel is not None:
        r = rowsel.to(v.dtype)[:, None]
        v, vt = v * r, vt * r
    return {"s1": (v.sum(0), _bound(n1, vt.sum(0))), "s2": ((v * w).sum(0), _bound(n2, (vt * w.abs()).sum(0)))}


def gemm_fwd(A, W, pro=0, pro_act=0, sc=None, sh=None, bias=None, addend=None, epi=0, esc=None, esh=None, epi_act=0, n_part=0,
             rowsel=None):
    """C = Aeff . W^T, Aeff = A (pro 0) or act(A*sc + sh) (pro 1).
    epi 0 / 1: c = (raw + addend) + bias                       n_seq: pro + K + 4 (+ 1 addend) (+ 1 bias)
    epi 1:     s1 = sum c, s2 = sum c^2 per column              n_seq: n + n_part, 2 n + 1 + n_part
    epi 5:     c = act((raw + bias)*esc + esh) + addend        n_seq: pro + K + 4 (+ 1 bias) + 1 (+ 1 addend); raw is itself
               rounded, so nothing is masked out of the terms (the clamp is 1-Lipschitz)"""
    a, at = act_in(A, sc if pro == 1 else None, sh, pro_act)
    v, vt = a @ W.t(), at @ W.abs().t()
    n = (pro == 1) + A.shape[1] + SPLIT_TERMS
    if addend is not None and epi != 5:
        v, vt, n = v + addend, vt + addend.abs(), n + 1
    if bias is not None:
        v, vt, n = v + bias, vt + bias.abs(), n + 1
    if epi == 5:
        v, vt, n = act(v * esc + esh, epi_act), vt * esc.abs() + esh.abs(), n + 1
        if addend is not None:
            v, vt, n = v + addend, vt + addend.abs(), n + 1
    out = {"c": (v, _bound(n, vt))}
    if epi == 1:
        if rowsel is not None:
            r = rowsel.to(v.dtype)[:, None]
            v, vt = v * r, vt * r
        out["s1"] = (v.sum(0), _bound(n + n_part, vt.sum(0)))
        out["s2"] = ((v * v).sum(0), _bound(2 * n + 1 + n_part, (vt * vt).sum(0)))
    return out


def gemm_dgrad(G, Y, Wt, al, be, ga, msc=None, msh=None, pro_act=0, addend=None, epi=0, X=None, esc=None, esh=None, mean=None,
               invstd=None, epi_act=0, n_part=0, rowsel=None):
    """data gradient: the pro 2 operand e = al*(G*mask(Y*msc+msh)) + be*Y + ga (msc None: no mask), Wt [Nout, Kred]
    epi 0: c = e . Wt^T + addend                                n_seq: 2 + Kred + 4 (+ 1 addend)
    epi 2: c = (e . Wt^T + addend) * act'(X*esc+esh)            the same (the mask is exact)
           s1 = sum c, s2 = sum c * (X - mean) * invstd          n_seq: n + n_part, n + 2 + n_part"""
    e, et, n_e = dyeff(G, Y, al, be, ga, msc, msh, pro_act)
    v, vt = e @ Wt.t(), et @ Wt.abs().t()
    n = n_e + G.shape[1] + SPLIT_TERMS
    if addend is not None:
        v, vt, n = v + addend, vt + addend.abs(), n + 1
    out = {}
    if epi == 2:
        m = mask32(X, esc, esh, epi_act)
        v, vt = v * m, vt * m
        out.update(_stats(v, vt, (X - mean) * invstd, n + n_part, n + 2 + n_part, rowsel))
    out["c"] = (v, _bound(n, vt))
    return out


def gemm_wgrad(D, X, al, be, ga, msc, msh, d_mode, d_act, A, asc, ash, a_mode, a_act, n_red):
    """dW [N, K] = Deff^T . Aeff; Deff = D (d_mode 0) or al*(D*mask(X*msc+msh)) + be*X + ga (d_mode 2), Aeff = A (a_mode 0) or
    act(A*asc + ash) (a_mode 1)                                  n_seq: (2) + (1) + 4 + n_red"""
    if d_mode == 2:
        e, et, n_e = dyeff(D, X, al, be, ga, msc, msh, d_act)
    else:
        e, et, n_e = D, D.abs(), 0
    a, at = act_in(A, asc if a_mode == 1 else None, ash, a_act)
    return {"dw": (e.t() @ a, _bound(n_e + (a_mode == 1) + SPLIT_TERMS + n_red, et.t() @ at))}


# ---- emulation of the split product ------------------------------------------------------------------------------------------

SMALLEST_FIRST = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))    # PA / PB of the kernels: (piece of x, piece of y)
LARGEST_FIRST = SMALLEST_FIRST[::-1]
LEADING_THREE = ((0, 1), (1, 0), (0, 0))


def split3(x):
    """the three bf16 pieces (as fp32) of an fp32 tensor, each rounded to nearest even (kd_split_pair): x - hi and x - hi - mid
    are exact in fp32"""
    assert x.dtype == torch.float32
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return hi, mid, lo


def six_products(x, y, order=SMALLEST_FIRST):
    """the piece products of x * y added to an fp32 accumulator one after the other in `order`, every add rounded to nearest
    (a bf16 x bf16 product has 16 significant bits: exact in fp32)"""
    px, py = split3(x), split3(y)
    acc = torch.zeros_like(x)
    for i, j in order:
        acc = acc + px[i] * py[j]
    return acc
