"""Float64 references for the kernels between the fusion output and the logits, plus the FPN / LiDAR-map resize
(csrc/kd_fuse.hip, csrc/kd_head.hip), with the rounding-error bound each kernel output must meet.

Every function takes the kernel's fp32 inputs (any device; evaluated in the inputs' dtype -- float64 for the references,
float32 for the self-check that a plain fp32 evaluation meets the same bound) and returns {name: (value, err)}:
`value` is the operation written as explicit gathers and matmuls, `err` the allowed |got - value| per element,

    err = C_BOUND * n_seq * U * sum |t_i|

over the n terms t_i an output is built from, `sum |t_i|` evaluated in the same precision alongside the value and n_seq the
longest sequential fp32 chain: the number of terms for an element-wise output; iterations per slot + slots + slab rows (+ the
slab reduction's split) for a grid-stride reduction.  Where a kernel feeds one rounded intermediate into another (softmax
weights, the gradient of the attention logits), that intermediate's bound enters linearly, weighted by the factor it is
multiplied with.  Reductions take their n_seq from the caller, which knows the launch layout."""
import torch

U = 2.0 ** -24          # unit roundoff of fp32
C_BOUND = 2.0           # the one constant of every bound in tests/test_gpu_tail_kernels.py
RELU = 1
SLAB_SPLIT = 64         # kd_slab_reduce_launch sums the slab rows in at most 64 lanes, then adds the lanes


def act(z, act_id):
    if act_id == 0:
        return z
    z = z.clamp_min(0)
    return z.clamp_max(6) if act_id == 2 else z


def act_mask(z, act_id):
    if act_id == 0:
        return torch.ones_like(z)
    m = z > 0
    if act_id == 2:
        m = m & (z < 6)
    return m.to(z.dtype)


def deferred(x, sc, sh, act_id):
    """act(x * sc + sh) per channel (last dim); sc None: x as is."""
    return x if sc is None else act(x * sc + sh, act_id)


def deferred_abs(x, sc, sh, act_id):
    """the terms of deferred(): |x*sc| + |sh| where the activation passes the value (the affine is a two-term sum)"""
    if sc is None:
        return x.abs()
    z = x * sc + sh
    return act_mask(z, act_id) * ((x * sc).abs() + sh.abs())


def _bound(n_seq, terms):
    return C_BOUND * n_seq * U * terms


# ---- bilinear resize, align_corners=False -------------------------------------------------------------------------------

def bilinear_matrix(in_size, out_size, coord=torch.float32, dtype=torch.float64, device="cpu"):
    """[out_size, in_size] interpolation weights.  coord=float32: the source coordinate exactly as the kernel forms it
    (fp32 scale in / out, one fused multiply-add, fp32 lambdas) -- the float64 reference then uses the kernel's own
    coefficients; coord=float64: aten's float64 path (F.interpolate on a float64 tensor)."""
    o = torch.arange(out_size, dtype=torch.float64)
    if coord == torch.float32:
        scale = torch.tensor(in_size, dtype=torch.float32) / torch.tensor(out_size, dtype=torch.float32)
        src = (scale.double() * (o + 0.5) - 0.5).float()          # exact product and difference, one rounding: the fma
    else:
        src = (in_size / out_size) * (o + 0.5) - 0.5
    src = src.clamp_min(0)
    i0 = src.floor().long().clamp_max(in_size - 1)
    i1 = torch.where(i0 < in_size - 1, i0 + 1, i0)
    l1 = src - i0.to(src.dtype)
    l0 = 1 - l1
    m = torch.zeros(out_size, in_size, dtype=torch.float64)
    rows = torch.arange(out_size)
    m.index_put_((rows, i0), l0.double(), accumulate=True)
    m.index_put_((rows, i1), l1.double(), accumulate=True)
    return m.to(dtype=dtype, device=device)


def _resize(v, mh, mw):
    """v [B, Hi, Wi, C] -> [B, Ho, Wo, C] = mh . v . mw^T per (batch, channel)."""
    t = torch.einsum("oh,bhwc->bowc", mh, v)
    return torch.einsum("pw,bowc->bopc", mw, t)


def bilinear_sum_fwd(laterals, Ho, Wo, out0=None):
    """laterals: [(x [B,Hi,Wi,C], sc, sh, act)], summed in order; out0 (accumulate): the buffer added to.
    out: n_seq = 6 per lateral (affine, two lambda products, two adds, the add into the sum) + 1 for out0."""
    val = None
    for x, sc, sh, a in laterals:
        mh = bilinear_matrix(x.shape[1], Ho, dtype=x.dtype, device=x.device)
        mw = bilinear_matrix(x.shape[2], Wo, dtype=x.dtype, device=x.device)
        r, ra = _resize(deferred(x, sc, sh, a), mh, mw), _resize(deferred_abs(x, sc, sh, a), mh, mw)
        val, tot = (r, ra) if val is None else (val + r, tot + ra)
    n = 6 * len(laterals)
    if out0 is not None:
        val, tot, n = val + out0, tot + out0.abs(), n + 1
    return {"out": (val, _bound(n, tot))}


def _window(m):
    """longest chain of nonzero weights a gather form meets along one axis: max over inputs of #outputs reading it"""
    return int((m != 0).sum(0).max().item())


def bilinear_bwd(dout, Hi, Wi, x=None, sc=None, sh=None, act_id=RELU, mean=None, invstd=None, n_part=0):
    """adjoint of the resize: gin = act'(x*sc+sh) * (mh^T . dout . mw), and (sum gin, sum gin*xhat) per channel over all
    rows when masked (n_part: iterations per slot + slots of the partial rows)."""
    B, Ho, Wo, C = dout.shape
    mh = bilinear_matrix(Hi, Ho, dtype=dout.dtype, device=dout.device)
    mw = bilinear_matrix(Wi, Wo, dtype=dout.dtype, device=dout.device)
    g, ga = _resize(dout, mh.t(), mw.t()), _resize(dout.abs(), mh.t(), mw.t())
    n_g = _window(mh) * _window(mw) + 3                      # the fma chain + weight product + lambda roundings
    out = {}
    if sc is not None:
        msk = act_mask(x * sc + sh, act_id)
        g, ga = g * msk, ga * msk
        if mean is not None:
            xh = (x - mean) * invstd
            out["s1"] = (g.sum((0, 1, 2)), _bound(n_g + n_part, ga.sum((0, 1, 2))))
            out["s2"] = ((g * xh).sum((0, 1, 2)), _bound(n_g + 2 + n_part, (ga * xh.abs()).sum((0, 1, 2))))
    out["gin"] = (g, _bound(n_g, ga))
    return out


# ---- weighted fusion tail ------------------------------------------------------------------------------------------------

def weighted_fuse_fwd(cat, sc, sh, hraw, w2, b2):
    """ReLU(hraw) -> 1x1 conv to 2 logits (+b2) -> softmax -> out = cam * w0 + lidar * w1, cam|lidar = ReLU(cat*sc+sh)."""
    C = hraw.shape[1]
    h = act(hraw, RELU)
    cp = deferred(cat[:, :C], sc[:C], sh[:C], RELU)
    lp = deferred(cat[:, C:], sc[C:], sh[C:], RELU)
    cpa, lpa = deferred_abs(cat[:, :C], sc[:C], sh[:C], RELU), deferred_abs(cat[:, C:], sc[C:], sh[C:], RELU)
    a = h @ w2.t() + b2
    sa = h.abs() @ w2.abs().t() + b2.abs()
    e = torch.exp(a - a.max(1, keepdim=True).values)
    w = e / e.sum(1, keepdim=True)
    ea = _bound(C + 2, sa + a.abs().amax(1, keepdim=True))   # the logits: C products, bias, minus the larger one
    ew = w[:, :1] * w[:, 1:] * ea.sum(1, keepdim=True) + _bound(4, w)        # softmax: d w0 = w0 w1 (d a0 - d a1); exp, sum, div
    out = cp * w[:, :1] + lp * w[:, 1:]
    eo = cp.abs() * ew[:, :1] + lp.abs() * ew[:, 1:] + _bound(3, cpa * w[:, :1] + lpa * w[:, 1:])
    return {"out": (out, eo), "wts": (w, ew)}


def weighted_fuse_bwd(dout, cat, sc, sh, hraw, w2, wts, n_red):
    """backward of weighted_fuse_fwd for given softmax weights `wts`: dcat = [dout*w0 | dout*w1], gh = dL/dhraw,
    dparams = dW2 (2C) | db1 (C) | db2 (2).  n_red: the sequential chain of a parameter-gradient sum over rows."""
    C = hraw.shape[1]
    h = act(hraw, RELU)
    cp = deferred(cat[:, :C], sc[:C], sh[:C], RELU)
    lp = deferred(cat[:, C:], sc[C:], sh[C:], RELU)
    cpa, lpa = deferred_abs(cat[:, :C], sc[:C], sh[:C], RELU), deferred_abs(cat[:, C:], sc[C:], sh[C:], RELU)
    w0, w1 = wts[:, :1], wts[:, 1:]
    g0, g1 = (dout * cp).sum(1, keepdim=True), (dout * lp).sum(1, keepdim=True)
    GL = (dout.abs() * cpa).sum(1, keepdim=True) + (dout.abs() * lpa).sum(1, keepdim=True)
    dot = w0 * g0 + w1 * g1
    da = torch.cat([w0 * (g0 - dot), w1 * (g1 - dot)], 1)                  # softmax backward [M, 2]
    eda = _bound(C + 5, wts * GL)                                           # C products (+ affine), dot, difference, product
    hm = (h > 0).to(h.dtype)
    gh = hm * (da @ w2)
    gha = hm * (da.abs() @ w2.abs())
    egh = hm * (eda @ w2.abs()) + _bound(2, gha)
    out = {
        "dcat": (torch.cat([dout * w0, dout * w1], 1), _bound(1, torch.cat([(dout * w0).abs(), (dout * w1).abs()], 1))),
        "gh": (gh, egh),
        "dw2": (da.t() @ h, eda.t() @ h.abs() + _bound(n_red + 1, da.abs().t() @ h.abs())),
        "db1": (gh.sum(0), egh.sum(0) + _bound(n_red, gha.sum(0))),
        "db2": (da.sum(0), eda.sum(0) + _bound(n_red, da.abs().sum(0))),
    }
    return out


# ---- classifier 1x1 ----------------------------------------------------------------------------------------------------

def rows_from_nchw(t):
    """[B, NC, H, W] (or [B, NC, HW]) -> [B*HW, NC]"""
    return t.reshape(t.shape[0], t.shape[1], -1).permute(0, 2, 1).reshape(-1, t.shape[1])


def nchw_from_rows(t, B):
    return t.reshape(B, -1, t.shape[1]).permute(0, 2, 1).contiguous()


def cls_conv_fwd(x, sc, sh, act_id, w, b, B):
    """logits [B, NC, HW] of the 1x1 classifier over deferred rows x [M, Cin]"""
    xa = deferred(x, sc, sh, act_id)
    r = xa @ w.t() + (0 if b is None else b)
    ra = deferred_abs(x, sc, sh, act_id) @ w.abs().t() + (0 if b is None else b.abs())
    return {"logits": (nchw_from_rows(r, B), nchw_from_rows(_bound(w.shape[1] + 2, ra), B))}


def _bn_partial(g, ga, x, mean, invstd, n_g, n_part, dims):
    xh = (x - mean) * invstd
    return {"s1": (g.sum(dims), _bound(n_g + n_part, ga.sum(dims))),
            "s2": ((g * xh).sum(dims), _bound(n_g + 2 + n_part, (ga * xh.abs()).sum(dims)))}


def cls_conv_bwd(dlog, x, sc, sh, act_id, mean, invstd, w, n_red, n_part):
    """dlog [B, NC, HW] -> gx [M, Cin], dw [NC, Cin], db [NC] and, with sc, the BN-backward sums s1, s2 [Cin]"""
    dl = rows_from_nchw(dlog)
    xa = deferred(x, sc, sh, act_id)
    g, ga = dl @ w, dl.abs() @ w.abs()
    n_g = w.shape[0]
    out = {"dw": (dl.t() @ xa, _bound(n_red + 1, dl.abs().t() @ deferred_abs(x, sc, sh, act_id))),
           "db": (dl.sum(0), _bound(n_red, dl.abs().sum(0)))}
    if sc is not None:
        m = act_mask(x * sc + sh, act_id)
        g, ga = g * m, ga * m
        if mean is not None:
            out.update(_bn_partial(g, ga, x, mean, invstd, n_g, n_part, 0))
    out["gx"] = (g, _bound(n_g, ga))
    return out


# ---- 3x3 classifier (pad 1) ----------------------------------------------------------------------------------------------

def _pad_hw(v):
    """[B, H, W, C] -> [B, H+2, W+2, C] with a zero border"""
    return torch.nn.functional.pad(v, (0, 0, 1, 1, 1, 1))


def cls3x3_fwd(x, sc, sh, act_id, w, b):
    """x [B, H, W, Cin] deferred, w [NC, Cin, 3, 3] -> logits [B, NC, H, W]"""
    B, H, W, _ = x.shape
    xp, xpa = _pad_hw(deferred(x, sc, sh, act_id)), _pad_hw(deferred_abs(x, sc, sh, act_id))
    r, ra = 0, 0
    for kh in range(3):
        for kw in range(3):
            r = r + xp[:, kh:kh + H, kw:kw + W, :] @ w[:, :, kh, kw].t()
            ra = ra + xpa[:, kh:kh + H, kw:kw + W, :] @ w[:, :, kh, kw].abs().t()
    if b is not None:
        r, ra = r + b, ra + b.abs()
    return {"logits": (r.permute(0, 3, 1, 2), _bound(9 * w.shape[1] + 2, ra).permute(0, 3, 1, 2))}


def cls3x3_bwd(dlog, x, sc, sh, act_id, mean, invstd, w, n_red, n_part):
    """dlog [B, NC, H, W] -> gx [B, H, W, Cin], dw [NC, Cin, 3, 3], db [NC], and with sc the sums s1, s2 [Cin]"""
    B, H, W, Cin = x.shape
    NC = w.shape[0]
    d = dlog.permute(0, 2, 3, 1)                                    # [B, H, W, NC]
    dp = _pad_hw(d)
    xa = deferred(x, sc, sh, act_id)
    xp, xpa = _pad_hw(xa), _pad_hw(deferred_abs(x, sc, sh, act_id))
    g, ga = 0, 0
    dw = torch.zeros(NC, Cin, 3, 3, dtype=x.dtype, device=x.device)
    dwa = torch.zeros_like(dw)
    for kh in range(3):
        for kw in range(3):
            # input pixel (h, w) met tap (kh, kw) of output pixel (h + 1 - kh, w + 1 - kw)
            dv = dp[:, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W, :]
            g = g + dv @ w[:, :, kh, kw]
            ga = ga + dv.abs() @ w[:, :, kh, kw].abs()
            dw[:, :, kh, kw] = d.reshape(-1, NC).t() @ xp[:, kh:kh + H, kw:kw + W, :].reshape(-1, Cin)
            dwa[:, :, kh, kw] = d.reshape(-1, NC).abs().t() @ xpa[:, kh:kh + H, kw:kw + W, :].reshape(-1, Cin)
    out = {"dw": (dw, _bound(n_red + 1, dwa)),
           "db": (d.sum((0, 1, 2)), _bound(n_red, d.abs().sum((0, 1, 2))))}
    n_g = 9 * NC
    if sc is not None:
        m = act_mask(x * sc + sh, act_id)
        g, ga = g * m, ga * m
        if mean is not None:
            out.update(_bn_partial(g, ga, x, mean, invstd, n_g, n_part, (0, 1, 2)))
    out["gx"] = (g, _bound(n_g, ga))
    return out


# ---- ConvTranspose2d(k4, s2, p1): col2im / im2col ------------------------------------------------------------------------

def col2im_fwd(col, B, H, W, Cout, n_part):
    """col [B*H*W, Cout*16] (column co*16 + kh*4 + kw) -> out [B, 2H, 2W, Cout]:
    out[b, 2ih-1+kh, 2iw-1+kw, co] += col[(b,ih,iw), co, kh, kw]; plus (sum y, sum y^2) per channel."""
    c = col.reshape(B, H, W, Cout, 4, 4)
    o = torch.zeros(B, 2 * H + 2, 2 * W + 2, Cout, dtype=col.dtype, device=col.device)
    oa = torch.zeros_like(o)
    for kh in range(4):
        for kw in range(4):
            # padded row index 2ih - 1 + kh + 1
            o[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2, :] += c[..., kh, kw]
            oa[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2, :] += c[..., kh, kw].abs()
    y, ya = o[:, 1:2 * H + 1, 1:2 * W + 1, :], oa[:, 1:2 * H + 1, 1:2 * W + 1, :]
    return {"out": (y, _bound(4, ya)),
            "s1": (y.sum((0, 1, 2)), _bound(4 + n_part, ya.sum((0, 1, 2)))),
            "s2": ((y * y).sum((0, 1, 2)), _bound(9 + n_part, (ya * ya).sum((0, 1, 2))))}


def im2col_bwd(D, Y, al, be, ga, msc, msh, act_id, H, W):
    """D, Y [B, 2H, 2W, Cout] -> dcol [B*H*W, Cout*16] = dy_eff at tap (kh, kw), 0 outside the image, with
    dy_eff = al * (D * act'(Y*msc+msh)) + be * Y + ga."""
    B, Ho, Wo, Cout = D.shape
    g = D * (act_mask(Y * msc + msh, act_id) if act_id else 1)
    e = al * g + be * Y + ga
    ea = (al * g).abs() + (be * Y).abs() + ga.abs()
    ep, eap = _pad_hw(e), _pad_hw(ea)
    dcol = torch.zeros(B, H, W, Cout, 4, 4, dtype=D.dtype, device=D.device)
    dcola = torch.zeros_like(dcol)
    for kh in range(4):
        for kw in range(4):
            dcol[..., kh, kw] = ep[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2, :]
            dcola[..., kh, kw] = eap[:, kh:kh + 2 * H:2, kw:kw + 2 * W:2, :]
    return {"dcol": (dcol.reshape(B * H * W, Cout * 16), _bound(3, dcola.reshape(B * H * W, Cout * 16)))}
