"""Float64 reference for csrc/kd_loss_lovasz.hip (kd_seg_lovasz_fwd_bwd): the Lovasz-Softmax hard-label term of DESIGN.md section 3
(classes = "present", per image), written from the definition with the CUMULATIVE form of the Jaccard increments
(g_k = J_k - J_{k-1}, J_k = 1 - I_k / U_k), its value, dL/dlogits and the rounding-error bound each kernel output must meet, in
the conventions of tests/_fp64_loss_ref.py:

    err = C_BOUND * n_seq * U * sum |t_i|

Two entries:
  lovasz(zs, y, ign, weight, gs)                    sorts by its own float64 errors, equal errors in ascending pixel order
  lovasz_given_order(zs, y, ign, weight, gs, order) evaluates value and gradient for a supplied per-(image, class) order
The second exists because the gradient is piecewise constant in the order: fp32 and float64 may order a few pixels whose errors
differ by less than the fp32 softmax's deviation differently, the value is continuous across such a swap, the gradient is not.

Every function evaluates in the inputs' dtype; scalars enter as the fp32 values the C ABI receives (`f32`).  The softmax and its
relative bound `rel_p` are _fp64_loss_ref._softmax's.  Operation counts of the kernel, per step:
  * e: p_c off the class (rel_p); on it the sum of the other NC - 1 probabilities, NC - 2 additions on top (rel_p + (NC - 2));
    TINY for a probability that left the normal range;
  * g_k: integers below 2^24 convert exactly; 1 / U is one operation, I / (U' * U) two: a relative bound of 2 operations;
  * L_{b,c} = sum e_k g_k: the bounds of e and g weighted by the other factor, plus the reduction: a thread's chunk of
    NPAD / threads positions by fused multiply-add, 6 wave steps, the waves in order (`n_seq`), and the fp32 store;
  * everything after L_{b,c} (the per-image means, the batch mean, the class means, hard + weight * L) is formed in double and
    stored once: one operation each;
  * dL/dp = +-g / (B |P_b|): one more division (3 operations); the float64 cumulative g itself is a difference of two numbers
    near 1, wrong by up to 4 * 2^-53 in ABSOLUTE terms, which enters the coefficient's bound so that a tiny g is not held to
    a relative bound the reference cannot meet;
  * dzs_j = (weight * gs * p_j) * (q_j - sum_c p_c q_c): the form and the bound of the Tversky part of _fp64_region_loss_ref
    (NC fused multiply-adds, the difference, the products), two more products for weight * gscale * gscale_dev; the dot product
    carries sum_c e_p_c |q_c| with the absolute TINY part of each probability's bound, since logits of +-80 make a probability
    0 in fp32 and 1e-70 in float64 beside a coefficient of ordinary size."""
import torch

from _fp64_loss_ref import TINY, _bound, _softmax, f32  # noqa: F401  (re-exported for the tests)

MAX_HW = 16384
G_ABS = 4 * 2.0 ** -53


def layout(HW):
    """(NPAD, threads, positions per thread) of the sort kernel: keys padded to a power of two >= 64, NPAD / 8 threads in 64 .. 1024"""
    npad = 64
    while npad < HW:
        npad *= 2
    T = min(1024, max(64, npad // 8))
    return npad, T, npad // T


def n_seq(HW):
    _, T, E = layout(HW)
    return E + 6 + T // 64


def ws_bytes(B, NC, HW):
    return 4 * (2 * B * NC + B * NC * HW)


def errors(zs, y, ign):
    """zs [B, NC, HW], y int64 [B, HW] -> dict: keep [B, HW], fg [B, NC, HW] (kept pixels of the class), e and its bound e_e
    [B, NC, HW] (0 at dropped pixels), p, rel_p"""
    B, NC, HW = zs.shape
    keep = (y != ign) & (y >= 0) & (y < NC)
    p, _, _, rel_p = _softmax(zs, 1.0)
    cls = torch.arange(NC, device=zs.device).view(1, NC, 1)
    fg = (y.view(B, 1, HW) == cls) & keep.view(B, 1, HW)
    others = torch.stack([(p * (cls != c)).sum(1) for c in range(NC)], 1)      # sum_{j != c} p_j, never 1 - p_c
    e = torch.where(fg, others, p) * keep.view(B, 1, HW)
    rel_e = rel_p + fg * _bound(max(NC - 2, 0), 1.0)
    e_e = (rel_e * e + TINY) * keep.view(B, 1, HW)
    return dict(keep=keep, fg=fg, e=e, e_e=e_e, p=p, rel_p=rel_p)


def own_order(zs, y, ign):
    """[B, NC, HW] int64: the kept pixels of (b, c) by e descending, equal e in ascending pixel order, -1 past the kept count and
    for classes without a pixel in the image"""
    B, NC, HW = zs.shape
    r = errors(zs, y, ign)
    order = torch.full((B, NC, HW), -1, dtype=torch.int64, device=zs.device)
    for b in range(B):
        idx = torch.nonzero(r["keep"][b]).flatten()                           # ascending
        for c in range(NC):
            if not bool(r["fg"][b, c].any()):
                continue
            perm = torch.sort(-r["e"][b, c, idx], stable=True)[1]            # stable: ties keep the ascending pixel order
            order[b, c, :idx.numel()] = idx[perm]
    return order


def lovasz_given_order(zs, y, ign, weight, gs, order, hard0=0.0):
    """-> dict of (value, bound) pairs:
      "vals" [1 + NC]: L, then per class the mean of L_{b,c} over the images where it is present (0 if never)
      "hard": hard0 + weight * L       "dzs" [B, NC, HW]: weight * gs * dL/dzs       "lbc" [B, NC]: L_{b,c}
    and the plain tensors "e", "e_e", "dLde" (g at each pixel's rank, 0 elsewhere), "present" [B, NC], "order"."""
    B, NC, HW = zs.shape
    dt, dev = zs.dtype, zs.device
    r = errors(zs, y, ign)
    e, e_e, fg, keep, p, rel_p = (r[k] for k in ("e", "e_e", "fg", "keep", "p", "rel_p"))
    present = fg.any(2)                                                       # [B, NC]
    npres = present.sum(1)                                                    # |P_b|
    lbc, e_lbc = torch.zeros(B, NC, dtype=dt, device=dev), torch.zeros(B, NC, dtype=dt, device=dev)
    dLde = torch.zeros_like(zs)
    ns = n_seq(HW)
    for b in range(B):
        for c in range(NC):
            if not bool(present[b, c]):
                continue
            idx = order[b, c]
            idx = idx[idx >= 0].long()
            n = idx.numel()
            es, f = e[b, c, idx], fg[b, c, idx].to(dt)
            F = torch.cumsum(f, 0)
            G = F[-1]
            I = G - F
            Un = G + torch.arange(1, n + 1, dtype=dt, device=dev) - F
            J = 1.0 - I / Un
            g = J - torch.cat([torch.zeros(1, dtype=dt, device=dev), J[:-1]])
            t = es * g
            lbc[b, c] = t.sum()
            e_lbc[b, c] = (e_e[b, c, idx] * g.abs() + _bound(2, t.abs())).sum() + _bound(ns + 1, t.abs().sum())
            dLde[b, c, idx] = g
    wb = torch.where(npres > 0, 1.0 / (B * npres.clamp_min(1).to(dt)), torch.zeros(B, dtype=dt, device=dev))    # 1 / (B |P_b|)
    L = (lbc * wb.view(B, 1)).sum()
    e_L = (e_lbc * wb.view(B, 1)).sum() + _bound(1, L.abs())
    cnt = present.sum(0).to(dt)
    cm = torch.where(cnt > 0, lbc.sum(0) / cnt.clamp_min(1), torch.zeros_like(cnt))
    e_cm = torch.where(cnt > 0, e_lbc.sum(0) / cnt.clamp_min(1), torch.zeros_like(cnt)) + _bound(1, cm.abs())
    hard = hard0 + weight * L
    e_hard = weight * e_L + _bound(1, abs(hard))
    out = {"vals": (torch.cat([L.view(1), cm]), torch.cat([e_L.view(1), e_cm])), "hard": (hard, e_hard), "lbc": (lbc, e_lbc),
           "e": e, "e_e": e_e, "dLde": dLde, "present": present, "order": order}
    # gradient: q = dL/dp_{i,c} = (fg ? -1 : +1) g / (B |P_b|), then the softmax Jacobian
    kf = keep.view(B, 1, HW).to(dt)
    sign = torch.where(fg, -torch.ones_like(zs), torch.ones_like(zs))
    q = sign * dLde * wb.view(B, 1, 1)
    e_q = _bound(3, q.abs()) + G_ABS * wb.view(B, 1, 1) * present.view(B, NC, 1) * kf
    sc = weight * gs
    dot, adot = (p * q).sum(1, keepdim=True), (p * q.abs()).sum(1, keepdim=True)
    e_dot = (p * e_q).sum(1, keepdim=True)
    gt = sc * p * (q - dot) * kf
    gta = abs(sc) * p * (q.abs() + adot) * kf
    e_p = rel_p * p + TINY
    # the dot product inherits every probability's bound weighted by its coefficient: sum_c e_p_c |q_c| (TINY included: a
    # probability that underflowed to 0 in fp32 still multiplies a coefficient of ordinary size)
    e_dot = e_dot + (e_p * q.abs()).sum(1, keepdim=True)
    e_t = abs(sc) * kf * (p * (e_q + e_dot) + e_p * (q.abs() + adot)) + _bound(NC + 6, gta)
    out["dzs"] = (gt, e_t)
    out["coef"] = q
    return out


def lovasz(zs, y, ign, weight, gs, hard0=0.0):
    """lovasz_given_order with the reference's own order"""
    return lovasz_given_order(zs, y, ign, weight, gs, own_order(zs, y, ign), hard0)


# ---- inputs and cases shared by the host self-check and tests/test_gpu_lovasz_loss.py -----------------------------------------

SCENES = ("random", "absent", "ignored", "one_class", "const", "dups", "sat")
SIZES = (1, 63, 64, 65, 1000, 4096, 16384)      # smallest; the wave edge; padding to 1024; the benchmarked map; the cap


def lovasz_inputs(B, NC, HW, seed, device, scene="random", ignore_index=-1):
    """logits N(0, 3^2); about 10 % of the labels ignore_index, 2 % each NC + 1 and -7.  In every image (HW >= 16) the pixels
    i % 7 == 3 carry the bits of pixel 3's logits (identical rows scattered among distinct ones) and the pixels i % 11 == 5
    logits of +-80 (probabilities exactly 0 and 1 in fp32).  The scene shapes the LAST image: "absent": no pixel of class
    NC - 1; "ignored": every label ignored; "one_class": every pixel kept and of class 1 (G = n); "const": one logit per class
    over the whole image (every error ties: the order is the pixel order within fg); "dups": three quarters of the pixels copy
    one of five rows; "sat": every pixel at +-80."""
    g = torch.Generator(device=device).manual_seed(seed)
    zs = torch.randn(B, NC, HW, generator=g, device=device) * 3.0
    y = torch.randint(0, NC, (B, HW), generator=g, device=device)
    r = torch.rand(B, HW, generator=g, device=device)
    for lo, hi, bad in ((0.0, 0.1, ignore_index), (0.1, 0.12, NC + 1), (0.12, 0.14, -7)):
        y = torch.where((r >= lo) & (r < hi), torch.full_like(y, bad), y)
    i = torch.arange(HW, device=device)
    hot = torch.zeros(NC, HW, device=device).scatter_(0, (i % NC).view(1, HW), 1.0)
    sat = (hot * 2 - 1) * 80.0                                                  # +80 at class i % NC, -80 elsewhere
    if HW >= 16:
        zs = torch.where((i % 7 == 3).view(1, 1, HW), zs[:, :, 3:4], zs)
        zs = torch.where((i % 11 == 5).view(1, 1, HW), sat.view(1, NC, HW), zs)
    s = B - 1
    if scene == "absent":
        y[s] = torch.where(y[s] == NC - 1, torch.zeros_like(y[s]), y[s])
    elif scene == "ignored":
        y[s] = ignore_index
    elif scene == "one_class":
        y[s] = 1
    elif scene == "const":
        zs[s] = torch.linspace(-1.0, 0.5, NC, device=device).view(NC, 1).expand(NC, HW)
    elif scene == "dups":
        src = zs[s][:, i % 5]
        zs[s] = torch.where((i % 4 != 0).view(1, HW), src, zs[s])
    elif scene == "sat":
        zs[s] = sat
    else:
        assert scene == "random", scene
    return zs.contiguous(), y.contiguous()


def cases():
    """(HW, B, NC, scene): every size with B in {1, 3} and NC in {2, 3, 4}, the scene rotating so that every scene meets every size"""
    out = []
    for si, HW in enumerate(SIZES):
        for bi, B in enumerate((1, 3)):
            for NC in (2, 3, 4):
                out.append((HW, B, NC, SCENES[(len(out) + 2 * si) % len(SCENES)]))
    # one more pass of the scenes over the benchmarked map and the cap, so each of the seven is run there
    for HW in (4096, 16384):
        have = {c[3] for c in out if c[0] == HW}
        out += [(HW, 3, 2 + k % 3, sc) for k, sc in enumerate(SCENES) if sc not in have]
    # between the two: 8192 padded keys, the first size whose keys (64 KiB) need the raised dynamic LDS limit, 1024 threads
    out.append((5000, 3, 3, "random"))
    return out


CASES = cases()


def case_id(c):
    return "HW%d-B%d-NC%d-%s" % c
