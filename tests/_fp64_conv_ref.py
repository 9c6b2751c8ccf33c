"""Float64 references for the camera body: the 3x3 / stride-2 stem, its im2col, the depthwise 3x3 forward and backward
(csrc/kd_conv.hip) and the row-wise BatchNorm kernels (kd_bn_act_apply, kd_bn_act_apply_res, kd_bn_bwd_reduce of
csrc/kd_bn.hip), with the rounding-error bound each kernel output must meet.  Same conventions as tests/_fp64_tail_ref.py:
every function takes the kernel's fp32 inputs (any device; evaluated in the inputs' dtype -- float64 for the truth, float32
for the self-check of the bound) and returns {name: (value, err)} with

    err = C_BOUND * n_seq * U * sum |t_i|

`sum |t_i|` evaluated alongside the value.  The convolutions are nine explicit shifted multiply-adds over a zero-padded NHWC
tensor; nothing here calls F.conv2d.  n_seq, counted from the kernel source, is written next to each output.  A reduction
gets the sequential part of its chain from the caller, who mirrors the launch layout (dw_layout / dw_bwd_forms below):
n_part = accumulations per thread + the threads a block adds up (the slab rows are summed in float64 by the test),
n_red = the same for the weight gradient + slab rows + SLAB_SPLIT, where kd_slab_reduce_launch sums the rows in fp32.

Masks.  The kernels form z = fmaf(x, sc, sh) once and test z > 0 && z < 6.  An exact value just below 6 rounds to 6.0f and
the kernel's mask is 0 where a mask taken from the float64 z would be 1.  Every mask here is therefore taken from z rounded
ONCE to fp32, (x.double() * sc.double() + sh.double()).float() -- the fma's result up to a double rounding (53 -> 24 bits)
nobody will meet -- whatever dtype the rest is evaluated in.  With that no element is left out of any comparison.

Activated operands.  act(z) itself is compared in the evaluation dtype (the clamp is 1-Lipschitz and rounding is monotonic,
so |fl(z) - z| <= U (|x sc| + |sh|) carries over); its term is |x sc| + |sh| where the value passes, 6 where ReLU6 saturates
(exact, but it takes part in later sums) and 0 below zero."""
import torch

from _fp64_tail_ref import C_BOUND, SLAB_SPLIT, U, _bound, _pad_hw, act    # noqa: F401  (C_BOUND, U, SLAB_SPLIT re-exported)

DW_SEG = 16             # rows of a column segment (DW_SEG in kd_conv.hip)
DT_COLS = 16            # columns of a strip of dw_bwd_tile_s1_kernel


def z32(x, sc, sh):
    """fmaf(x, sc, sh): the exact product and sum rounded once to fp32"""
    return (x.double() * sc.double() + sh.double()).float()


def mask32(x, sc, sh, act_id):
    """kd_act_mask(kd_affine(x, sc, sh), act) in the dtype of x"""
    if act_id == 0:
        return torch.ones_like(x)
    z = z32(x, sc, sh)
    m = z > 0
    if act_id == 2:
        m = m & (z < 6)
    return m.to(x.dtype)


def act_in(x, sc, sh, act_id):
    """(value, terms) of a deferred operand act(x * sc + sh); sc None: x as it is (no activation either)"""
    if sc is None:
        return x, x.abs()
    z = x * sc + sh
    t = (x * sc).abs() + sh.abs()
    if act_id == 0:
        return z, t
    t = torch.where(z <= 0, torch.zeros_like(t), t)
    if act_id == 2:
        t = torch.where(z >= 6, torch.full_like(t, 6.0), t)
    return act(z, act_id), t


def _out_size(n, stride):
    return (n - 1) // stride + 1


def _taps(vp, Ho, Wo, s):
    """the nine shifted views of the zero-padded vp [B, H+2, W+2, C]: tap k = kh*3 + kw of output (ho, wo) is input
    (s*ho - 1 + kh, s*wo - 1 + kw), padded index (s*ho + kh, s*wo + kw)"""
    for kh in range(3):
        for kw in range(3):
            yield kh * 3 + kw, vp[:, kh:kh + s * (Ho - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s, :]


# ---- input recipes (shared by the GPU suite and the CPU self-check of the bounds) ---------------------------------------------

def rnd(g, *s):
    return torch.randn(*s, generator=g, device=g.device)


def coeffs(g, C, act_id=1):
    """(sc, sh, mean, invstd) as a training BatchNorm hands them on: positive scale, small shift; for ReLU6 the shift is
    3 -+ (2.5 + |randn|), the sign alternating over the channels, so that even with 8 channels a visible share of
    z = x*sc+sh lies below 0, inside (0, 6) and above 6 (relu6_shares)"""
    sc, sh, mean, inv = rnd(g, C).abs() + 0.5, rnd(g, C) * 0.2, rnd(g, C) * 0.1, rnd(g, C).abs() + 0.5
    if act_id == 2:
        sign = 1.0 - 2.0 * (torch.arange(C, device=sh.device) % 2)
        sh = 3.0 + sign * (2.5 + 5.0 * sh.abs())
    return sc, sh, mean, inv


def folded(g, C):
    """(al, be, ga) of a BatchNorm backward folded into the load of (D, Y)"""
    return rnd(g, C), rnd(g, C) * 0.1, rnd(g, C) * 0.1


def relu6_shares(x, sc, sh):
    """shares of z = fmaf(x, sc, sh) at or below 0, inside (0, 6) and at or above 6"""
    z = z32(x, sc, sh)
    n = z.numel()
    return (z <= 0).sum().item() / n, ((z > 0) & (z < 6)).sum().item() / n, (z >= 6).sum().item() / n


# ---- launch layouts (mirrors of kd_conv.hip; the suites assert them equal to the library's answers) ---------------------------

def dw_layout(npix, C):
    """dw_layout: (groups, slots, nchunk, rows)"""
    quads = C // 4
    nchunk = quads // 32 if quads > 64 and quads % 32 == 0 else 1
    groups = quads // nchunk
    slots = max(1, 256 // groups)
    rows = max(1, min(-(-npix // slots), 2048 // nchunk))
    return groups, slots, nchunk, rows


def dw_fwd_form(B, H, W, C, stride):
    """the launch kd_dwconv3x3_fwd selects and its segment height"""
    Ho = _out_size(H, stride)
    small = B * H * W * C < 2 ** 31
    if stride == 1 and small and Ho % 16 == 0:
        return "dw_fwd_pipe_kernel<1,16>", 16
    if small and Ho % 8 == 0:
        return f"dw_fwd_pipe_kernel<{stride},8>", 8
    return f"dw_fwd_sw_kernel<{stride}>", DW_SEG


def dw_fused_form(mode, C, W, stride):
    if mode == 3:
        return 2 if stride == 1 and C >= 64 and C % 64 == 0 and W >= 16 else 1
    return mode


def _walk(items, rows, slots, per_item):
    """sequential accumulations of one thread of a column walk + the `slots` threads a block adds up"""
    return -(-items // (rows * slots)) * per_item + slots


def dw_fwd_chain(B, H, W, C, stride):
    """n_part of the forward statistics"""
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    _, slots, _, rows = dw_layout(B * Ho * Wo, C)
    seg = dw_fwd_form(B, H, W, C, stride)[1]
    return _walk(B * -(-Ho // seg) * Wo, rows, slots, min(seg, Ho))


def dw_bwd_forms(mode, B, H, W, C, stride, want_gx, want_dw):
    """the kernels dw_bwd_impl launches -> (names, n_part of (s1, s2), n_red of dw)"""
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    form = dw_fused_form(mode, C, W, stride)
    _, slots, _, rows = dw_layout(B * H * W, C)
    nseg = -(-H // DW_SEG)
    if stride == 1:
        col = wcol = _walk(B * nseg * W, rows, slots, min(DW_SEG, H))
    else:                           # 2x2 quads, 8 quad rows a segment: four pixels added per quad row, one product per tap
        QH, QW = (H + 1) // 2, (W + 1) // 2
        col = _walk(B * -(-QH // 8) * QW, rows, slots, min(8, QH) * 4)
        wcol = _walk(B * -(-QH // 8) * QW, rows, slots, min(8, QH))
    if want_gx and want_dw and form != 0:
        if stride == 2:
            return ["dw_bwd_fused_s2_kernel"], col, wcol + rows + SLAB_SPLIT
        if form == 2:               # one strip item per workgroup and turn, 16 columns added per workgroup
            tile = -(-(B * nseg * -(-W // DT_COLS)) // rows) * min(DW_SEG, H) + DT_COLS
            return ["dw_bwd_tile_s1_kernel"], tile, tile + rows + SLAB_SPLIT
        return ["dw_bwd_fused_s1_kernel"], col, wcol + rows + SLAB_SPLIT
    names, n_red = [], 0
    if want_gx:
        names.append("dw_bwd_data_sw_kernel" if stride == 1 else "dw_bwd_data_s2_kernel")
    if want_dw:
        _, wslots, _, wrows = dw_layout(B * Ho * Wo, C)
        names.append(f"dw_bwd_weight_sw_kernel<{stride}>")
        n_red = _walk(B * -(-Ho // DW_SEG) * Wo, wrows, wslots, min(DW_SEG, Ho)) + wrows + SLAB_SPLIT
    return names, col, n_red


def stem_chain(npix, cin):
    """n_part of the stem statistics: Cin 3 (stem_fwd2_kernel) keeps per-thread sums over its pixels, then 32 threads, then 8
    segments; the LDS form adds 256 pixels per batch, then the batches"""
    grid = min(-(-npix // 256), 1024)
    iters = -(-npix // (grid * 256))
    return iters + 32 + 8 if cin == 3 else iters + 256


KERNEL_WALK = {"dw_bwd_data_sw_kernel": "bwd_col", "dw_bwd_fused_s1_kernel": "bwd_col", "dw_bwd_tile_s1_kernel": "bwd_tile",
               "dw_bwd_data_s2_kernel": "bwd_quad", "dw_bwd_fused_s2_kernel": "bwd_quad",
               "dw_bwd_weight_sw_kernel<1>": "bwd_weight", "dw_bwd_weight_sw_kernel<2>": "bwd_weight"}


def dw_walk(kind, B, H, W, C, stride):
    """The grid-stride walk of one depthwise kernel over its work items.  An item is a column segment: `seg` rows x `colw`
    columns of the map the kernel walks (the output map for "fwd" and "bwd_weight", the input map for "bwd_col", "bwd_tile"
    -- 16-column strips, one item per workgroup and turn -- and "bwd_quad" -- 2 x 2 quads, 8 quad rows a segment), items
    ordered (frame, segment, column).  -> dict(Hm, Wm, seg, colw, slots, rows, per_turn, items, iters)"""
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    on_out = kind in ("fwd", "bwd_weight")
    Hm, Wm = (Ho, Wo) if on_out else (H, W)
    _, slots, _, rows = dw_layout(B * Hm * Wm, C)
    seg = dw_fwd_form(B, H, W, C, stride)[1] if kind == "fwd" else DW_SEG
    colw = {"bwd_tile": DT_COLS, "bwd_quad": 2}.get(kind, 1)
    if kind == "bwd_tile":
        slots = 1
    items = B * -(-Hm // seg) * -(-Wm // colw)
    return dict(Hm=Hm, Wm=Wm, seg=seg, colw=colw, slots=slots, rows=rows, per_turn=rows * slots, items=items,
                iters=-(-items // (rows * slots)))


def dw_item_ladder(C, tile=False):
    """work-item counts around one full turn of the grid (cap * slots items; the tile form: cap workgroups)"""
    _, slots, nchunk, _ = dw_layout(1, C)
    slots = 1 if tile else slots
    full = (2048 // nchunk) * slots
    return {"few": max(1, slots // 3), "partial_block": 3 * slots + slots // 2 + 1, "full-1": full - 1, "full": full,
            "full+1": full + 1, "ragged": 2 * full + full // 3 + 5}


def dw_tail_mask(B, walk, device="cpu"):
    """[B, Hm, Wm] bool over the map a kernel walks (dw_walk): the pixels of the items it handles last or at its edges -- the
    last (ragged) turn of the grid-stride loop when there is more than one, the last block of every turn, the last segment
    (when there are several) and the last 16 columns of the last frame, and the first / last row and column of the first and
    last frame"""
    Hm, Wm, seg, colw, slots, rows = (walk[k] for k in ("Hm", "Wm", "seg", "colw", "slots", "rows"))
    nseg, ncol = -(-Hm // seg), -(-Wm // colw)
    b = torch.arange(B, device=device)[:, None, None]
    h = torch.arange(Hm, device=device)[None, :, None]
    w = torch.arange(Wm, device=device)[None, None, :]
    it = (b * nseg + h // seg) * ncol + w // colw
    sel = (it // slots) % rows == rows - 1
    if walk["iters"] > 1:
        sel = sel | (it >= (walk["iters"] - 1) * walk["per_turn"])
    last = w // DT_COLS == (Wm - 1) // DT_COLS
    if nseg > 1:
        last = last | (h // seg == nseg - 1)
    edge = (h == 0) | (h == Hm - 1) | (w == 0) | (w == Wm - 1)
    return sel | last & (b == B - 1) | edge & ((b == 0) | (b == B - 1))


def dw_bwd_tail_mask(names, B, H, W, C, stride, device="cpu"):
    """[B, Ho, Wo] bool for the upstream gradient: the union of dw_tail_mask over the kernels `names` of one backward call, a
    mask over the input map taken at the top-left pixel of each stride x stride cell"""
    m = None
    for n in names:
        wk = dw_walk(KERNEL_WALK[n], B, H, W, C, stride)
        t = dw_tail_mask(B, wk, device)
        if (wk["Hm"], wk["Wm"]) != (_out_size(H, stride), _out_size(W, stride)):
            t = t[:, ::stride, ::stride]
        m = t if m is None else m | t
    return m


def dw_fwd_tail_mask(B, H, W, C, stride, device="cpu"):
    """[B, H, W] bool for the forward's input: the input pixels of the output pixels dw_tail_mask selects on the (Ho, Wo) walk"""
    t = dw_tail_mask(B, dw_walk("fwd", B, H, W, C, stride), device)
    return t.repeat_interleave(stride, 1).repeat_interleave(stride, 2)[:, :H, :W]


def row_tail_mask(rows, slots, grid, device="cpu"):
    """the rows a grid-stride walk over rows handles last or at its edges: the last (ragged) turn, the last block, row 0,
    row M-1"""
    iters = -(-rows // (grid * slots))
    m = torch.arange(rows, device=device)
    sel = (m >= (iters - 1) * grid * slots) | ((m // slots) % grid == grid - 1)
    sel[0] = sel[-1] = True
    return sel


# ---- stem --------------------------------------------------------------------------------------------------------------

def _stem_raw(x, w):
    Ho, Wo = _out_size(x.shape[2], 2), _out_size(x.shape[3], 2)
    xp = _pad_hw(x.permute(0, 2, 3, 1))                               # [B, H+2, W+2, Cin]
    y, ya = 0, 0
    for k, v in _taps(xp, Ho, Wo, 2):
        wk = w[:, :, k // 3, k % 3].t()                                # [Cin, Cout]
        y, ya = y + v @ wk, ya + v.abs() @ wk.abs()
    return y, ya


def stem_fwd(x, w, n_part=0):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3], stride 2, pad 1 -> raw [B, Ho, Wo, Cout] (one fma chain of 9 Cin products),
    s1 = sum raw, s2 = sum raw^2 per channel"""
    y, ya = _stem_raw(x, w)
    n = 9 * x.shape[1]
    return {"y": (y, _bound(n, ya)),
            "s1": (y.sum((0, 1, 2)), _bound(n + n_part, ya.sum((0, 1, 2)))),
            "s2": ((y * y).sum((0, 1, 2)), _bound(2 * n + 1 + n_part, (ya * ya).sum((0, 1, 2))))}


def stem_infer(x, w, sc, sh, act_id):
    """act(fma(raw, sc, sh)): raw is itself rounded, so nothing is masked out of the terms (the clamp is 1-Lipschitz)"""
    y, ya = _stem_raw(x, w)
    return {"y": (act(y * sc + sh, act_id), _bound(9 * x.shape[1] + 1, ya * sc.abs() + sh.abs()))}


def stem_im2col(x, Kp):
    """col [B*Ho*Wo, Kp], column ci*9 + kh*3 + kw, zeros from Cin*9 to Kp: a copy, compared bit for bit"""
    B, Cin, H, W = x.shape
    Ho, Wo = _out_size(H, 2), _out_size(W, 2)
    xp = _pad_hw(x.permute(0, 2, 3, 1))
    col = torch.zeros(B, Ho, Wo, Kp, dtype=x.dtype, device=x.device)
    for k, v in _taps(xp, Ho, Wo, 2):
        col[..., k:Cin * 9:9] = v
    return col.reshape(B * Ho * Wo, Kp)


# ---- depthwise 3x3 -----------------------------------------------------------------------------------------------------

def dw_fwd(x, sc, sh, act_id, w, stride, n_part=0):
    """x [B, H, W, C] deferred, w [C, 9] -> y [B, Ho, Wo, C] (n_seq: the affine + 9 fmas), s1 = sum y, s2 = sum y^2"""
    B, H, W, C = x.shape
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    a, t = act_in(x, sc, sh, act_id)
    y, ya = 0, 0
    for (k, v), (_, vt) in zip(_taps(_pad_hw(a), Ho, Wo, stride), _taps(_pad_hw(t), Ho, Wo, stride)):
        y, ya = y + v * w[:, k], ya + vt * w[:, k].abs()
    n = 9 + (sc is not None)
    return {"y": (y, _bound(n, ya)),
            "s1": (y.sum((0, 1, 2)), _bound(n + n_part, ya.sum((0, 1, 2)))),
            "s2": ((y * y).sum((0, 1, 2)), _bound(2 * n + 1 + n_part, (ya * ya).sum((0, 1, 2))))}


def dyeff(D, Y, al, be, ga, dsc, dsh, d_act):
    """kd_bwd_operand: al * (D * mask(Y*dsc+dsh)) + be*Y + ga as fmaf(al, g, fmaf(be, Y, ga)) -> (value, terms, roundings);
    al None: D itself"""
    if al is None:
        return D, D.abs(), 0
    g = D * mask32(Y, dsc, dsh, d_act) if dsc is not None else D
    return al * g + be * Y + ga, (al * g).abs() + (be * Y).abs() + ga.abs(), 2


def dw_bwd(D, Y, al, be, ga, dsc, dsh, d_act, x, sc, sh, act_id, mean, invstd, w, stride, addend=None, n_part=0, n_red=0):
    """backward of y = dwconv3x3(act(x*sc+sh)):
    gx = (conv^T dyeff + addend) * act'(x*sc+sh)                       n_seq: dyeff's 2 roundings + 9 fmas (+ 1 for the addend)
    s1 = sum gx, s2 = sum gx * (x - mean) * invstd  (with sc and mean)  n_seq: + n_part (+ 2 for xhat)
    dw[c][kh*3+kw] = sum dyeff(ho, wo) * act(x*sc+sh)(s*ho-1+kh, s*wo-1+kw)      n_seq: dyeff's 2 + the affine + n_red
    dyeff is a rounded intermediate multiplied by a weight or an input: its bound enters linearly, as its terms times that
    factor under the same n_seq."""
    B, H, W, C = x.shape
    Ho, Wo = _out_size(H, stride), _out_size(W, stride)
    e, et, n_e = dyeff(D, Y, al, be, ga, dsc, dsh, d_act)
    a, at = act_in(x, sc, sh, act_id)
    gp = torch.zeros(B, H + 2, W + 2, C, dtype=x.dtype, device=x.device)
    gtp = torch.zeros_like(gp)
    dw, dwt = [], []
    for (k, gv), (_, gtv), (_, av), (_, atv) in zip(_taps(gp, Ho, Wo, stride), _taps(gtp, Ho, Wo, stride),
                                                    _taps(_pad_hw(a), Ho, Wo, stride), _taps(_pad_hw(at), Ho, Wo, stride)):
        gv += e * w[:, k]
        gtv += et * w[:, k].abs()
        dw.append((e * av).sum((0, 1, 2)))
        dwt.append((et * atv).sum((0, 1, 2)))
    g, gt = gp[:, 1:H + 1, 1:W + 1, :], gtp[:, 1:H + 1, 1:W + 1, :]
    n_g = 9 + n_e
    if addend is not None:
        g, gt, n_g = g + addend, gt + addend.abs(), n_g + 1
    out = {"dw": (torch.stack(dw, 1), _bound(n_e + (sc is not None) + n_red, torch.stack(dwt, 1)))}
    if sc is not None:
        m = mask32(x, sc, sh, act_id)
        g, gt = g * m, gt * m
        if mean is not None:
            xh = (x - mean) * invstd
            out["s1"] = (g.sum((0, 1, 2)), _bound(n_g + n_part, gt.sum((0, 1, 2))))
            out["s2"] = ((g * xh).sum((0, 1, 2)), _bound(n_g + 2 + n_part, (gt * xh.abs()).sum((0, 1, 2))))
    out["gx"] = (g, _bound(n_g, gt))
    return out


# ---- row-wise BatchNorm kernels ----------------------------------------------------------------------------------------

def bn_act_apply(x, sc, sh, act_id, res=None, rsc=None, rsh=None, ract=0):
    """out = act(x*sc+sh) (+ res | + ract(res*rsc+rsh)); sc None: the identity affine, the activation still applies.
    n_seq: one per affine + the add"""
    if sc is None:
        v = act(x, act_id)
        t, n = v.abs(), 0
    else:
        (v, t), n = act_in(x, sc, sh, act_id), 1
    if res is not None:
        r, rt = act_in(res, rsc, rsh, ract)
        v, t, n = v + r, t + rt, n + 1 + (rsc is not None)
    return {"out": (v, _bound(n, t))}


def bn_bwd_reduce(D, X, sc, sh, act_id, mean, invstd, n_part=0):
    """s1 = sum G, s2 = sum G * xhat over rows, G = D * act'(X*sc+sh) (exact), xhat = (X - mean) * invstd (2 roundings)"""
    g = D * mask32(X, sc, sh, act_id) if act_id else D
    xh = (X - mean) * invstd
    return {"s1": (g.sum(0), _bound(n_part, g.abs().sum(0))),
            "s2": ((g * xh).sum(0), _bound(2 + n_part, (g * xh).abs().sum(0)))}
