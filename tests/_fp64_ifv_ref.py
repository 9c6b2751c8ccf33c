"""Float64 reference of the intra-class feature variation distillation feature term (kdrt.losses.IntraClassKD,
csrc/kd_loss_ifv.hip), written from the definition and independently of kdrt.

  value(S, T, y, NC)   the term as a differentiable torch expression in the dtype of its inputs (float64 in the tests)
  direct(S, T, y, NC)  the value, the per-image values, the closed-form gradient and the magnitudes that cancel in them
  ifv32(S, T, y, NC)   the same formulas in numpy float32, every sum taken in pixel order: the yardstick of what fp32 costs

S [B, n, Cs] and T [B, n, Ct] are the NHWC matrices of the two maps, y [B, n] the int64 labels.  Pixel i of image b is kept when
y != ignore_index and 0 <= y < NC; K_b kept pixels, N_bc of class c.  For X in {S, T}, per image:
  r_i = sqrt(sum_k x_ik^2), xh_i = x_i / r_i if r_i > 1e-12 else 0,  m_c = 1/N_bc sum_{i in c} x_i,  mh_c = m_c / |m_c| if |m_c| > 1e-12
  else 0,  s_i = xh_i . mh_{y_i};  L_b = 1/K_b sum_kept (sS_i - sT_i)^2 (0 if K_b = 0),  IFV = 1/B sum_b L_b;
  g_i = 2 (sS_i - sT_i) / (B K_b),  D_c = sum_{i in c} g_i (xh_i - s_i mh_c) / |m_c|,
  dIFV/dS_j = g_j (mh_c - s_j xh_j) / r_j [0 if r_j <= 1e-12] + D_c / N_bc for kept j (c = y_j), 0 otherwise."""
import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-12


def f32(x):
    return float(np.float32(x))


def kept_mask(y, NC, ignore_index=-1):
    return (y != ignore_index) & (y >= 0) & (y < NC)


def _sims(X, yb, kb, NC):
    """one image of one map -> (s [n] (0 where not kept), xh [n, C], r [n, 1], mh [NC, C], mnorm [NC], N [NC]); differentiable"""
    ss = X.pow(2).sum(-1, keepdim=True)
    r = ss.detach().sqrt()
    live = r > EPS
    xh = torch.where(live, X / torch.where(live, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(X))     # no sqrt'(0) for autograd
    s = torch.zeros(X.shape[0], dtype=X.dtype, device=X.device)
    mh, mn, N = [], [], []
    for c in range(NC):
        sel = kb & (yb == c)
        n_c = int(sel.sum())
        N.append(n_c)
        if n_c == 0:
            mh.append(torch.zeros_like(X[0])); mn.append(torch.zeros((), dtype=X.dtype, device=X.device))
            continue
        m = X[sel].sum(0) / n_c
        nrm = m.pow(2).sum().sqrt()
        mhc = m / nrm if nrm.item() > EPS else torch.zeros_like(m)
        mh.append(mhc); mn.append(nrm)
        s = torch.where(sel, xh @ mhc, s)
    return s, xh, r, torch.stack(mh), torch.stack(mn), N


def value(S, T, y, NC, ignore_index=-1):
    """IFV as a torch expression: autograd gives its gradient"""
    B = S.shape[0]
    k = kept_mask(y, NC, ignore_index)
    tot = 0.0
    for b in range(B):
        K = int(k[b].sum())
        if K == 0:
            continue
        sS = _sims(S[b], y[b], k[b], NC)[0]
        sT = _sims(T[b], y[b], k[b], NC)[0]
        tot = tot + (sS - sT).pow(2).sum() / K
    return tot / B if torch.is_tensor(tot) else torch.zeros((), dtype=S.dtype, device=S.device)


def direct(S, T, y, NC, ignore_index=-1):
    """-> dict(val, img [B], grad [B, n, Cs], M [B, n, Cs], Sv, Sv_img [B]).  M is the gradient formula with every term replaced by
    its absolute value and |sS_i - sT_i| by |sS_i| + |sT_i|: the magnitude that cancels in a gradient element; Sv_img =
    1/K_b sum (|sS_i| + |sT_i|)^2 the one that cancels in a per-image value, Sv their mean."""
    B, n, Cs = S.shape
    k = kept_mask(y, NC, ignore_index)
    img, Sv, grads, Ms = [], [], [], []
    with torch.no_grad():
        for b in range(B):
            K = int(k[b].sum())
            g_out, M_out = torch.zeros_like(S[b]), torch.zeros_like(S[b])
            if K == 0:
                img.append(torch.zeros((), dtype=S.dtype, device=S.device)); Sv.append(torch.zeros((), dtype=S.dtype, device=S.device))
                grads.append(g_out); Ms.append(M_out)
                continue
            sS, xh, r, mh, mn, N = _sims(S[b], y[b], k[b], NC)
            sT = _sims(T[b], y[b], k[b], NC)[0]
            d, a = sS - sT, sS.abs() + sT.abs()
            img.append(d.pow(2).sum() / K)
            Sv.append(a.pow(2).sum() / K)
            g, ga = 2.0 * d / (B * K), 2.0 * a / (B * K)
            rinv = torch.where(r > EPS, 1.0 / torch.where(r > EPS, r, torch.ones_like(r)), torch.zeros_like(r))
            for c in range(NC):
                if N[c] == 0:
                    continue
                sel = k[b] & (y[b] == c)
                gc, gac, sc, xc = g[sel, None], ga[sel, None], sS[sel, None], xh[sel]
                live = mn[c].item() > EPS
                D = (gc * (xc - sc * mh[c])).sum(0) / mn[c] if live else torch.zeros_like(mh[c])
                Da = (gac * (xc.abs() + sc.abs() * mh[c].abs())).sum(0) / mn[c] if live else torch.zeros_like(mh[c])
                g_out[sel] = gc * (mh[c] - sc * xc) * rinv[sel] + D / N[c]
                M_out[sel] = gac * (mh[c].abs() + sc.abs() * xc.abs()) * rinv[sel] + Da / N[c]
            grads.append(g_out); Ms.append(M_out)
    img, Sv = torch.stack(img), torch.stack(Sv)
    return {"val": img.sum() / B, "img": img, "grad": torch.stack(grads), "M": torch.stack(Ms), "Sv": Sv.sum() / B, "Sv_img": Sv}


def _seq(x, axis=0):
    """the float32 sum along `axis` in index order (np.cumsum adds one element after the other, without pairwise blocking)"""
    x = np.asarray(x, np.float32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), np.float32)
    return np.take(np.cumsum(x, axis=axis, dtype=np.float32), -1, axis=axis)


def ifv32(S, T, y, NC, ignore_index=-1):
    """the formulas above evaluated plainly in float32 (numpy), every sum in pixel / channel order -> dict(val, img, grad) as float64
    torch tensors on the CPU"""
    S32, T32 = S.detach().cpu().numpy().astype(np.float32), T.detach().cpu().numpy().astype(np.float32)
    yn = y.detach().cpu().numpy()
    B, n, Cs = S32.shape
    one = np.float32(1)
    kept = (yn != ignore_index) & (yn >= 0) & (yn < NC)

    def sims(X, yb, kb):
        r = np.sqrt(_seq(X * X, 1))[:, None]
        live = r > np.float32(EPS)
        xh = np.where(live, X / np.where(live, r, one), np.float32(0)).astype(np.float32)
        s = np.zeros(X.shape[0], np.float32)
        mh, mn = np.zeros((NC, X.shape[1]), np.float32), np.zeros(NC, np.float32)
        for c in range(NC):
            sel = kb & (yb == c)
            if not sel.any():
                continue
            m = _seq(X[sel], 0) / np.float32(sel.sum())
            mn[c] = np.sqrt(_seq(m * m, 0))
            if mn[c] > np.float32(EPS):
                mh[c] = m / mn[c]
            s[sel] = _seq(xh[sel] * mh[c], 1)
        return s, xh, r, mh, mn

    img, grads = np.zeros(B, np.float32), np.zeros((B, n, Cs), np.float32)
    for b in range(B):
        K = int(kept[b].sum())
        if K == 0:
            continue
        sS, xh, r, mh, mn = sims(S32[b], yn[b], kept[b])
        sT = sims(T32[b], yn[b], kept[b])[0]
        d = (sS - sT).astype(np.float32)
        img[b] = _seq((d * d)[kept[b]], 0) / np.float32(K)
        g = (np.float32(2) * d / np.float32(B * K)).astype(np.float32)
        live = r > np.float32(EPS)
        rinv = np.where(live, one / np.where(live, r, one), np.float32(0)).astype(np.float32)
        for c in range(NC):
            sel = kept[b] & (yn[b] == c)
            if not sel.any():
                continue
            gc, sc, xc = g[sel, None], sS[sel, None], xh[sel]
            D = _seq(gc * (xc - sc * mh[c]), 0) / mn[c] if mn[c] > np.float32(EPS) else np.zeros(Cs, np.float32)
            grads[b][sel] = gc * (mh[c] - sc * xc) * rinv[sel] + D / np.float32(sel.sum())
    val = _seq(img, 0) / np.float32(B)
    return {"val": torch.tensor(float(val), dtype=torch.float64), "img": torch.from_numpy(img.astype(np.float64)),
            "grad": torch.from_numpy(grads.astype(np.float64))}


# ---- input builders -------------------------------------------------------------------------------------------------------------

def slice_rows(B, HW):
    """mirror of the kernel's row slices: up to ceil(1024 / B) slices of at least 64 rows, cut at multiples of 32 rows"""
    want = 1 if B >= 1024 else -(-1024 // B)
    s = min(want, -(-HW // 64))
    return -(-(-(-HW // s)) // 32) * 32


def slices(B, HW):
    return -(-HW // slice_rows(B, HW))


def relu_maps(B, n, Cs, Ct, seed, device="cpu"):
    """ReLU'd normal maps as fp32 [B, n, C], one all-zero row in each (row n // 3 of S, row 2 n // 3 of T: the same row when n = 1)"""
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, n, Cs, generator=g).clamp_min(0)
    T = torch.randn(B, n, Ct, generator=g).clamp_min(0)
    S[:, n // 3] = 0
    T[:, (2 * n) // 3] = 0
    return S.to(device), T.to(device)


ZERO_ROWS = (7, 8, 9)       # image 0: the pixels of the class whose student rows are all zero
SINGLE = 5                  # image 0: the one pixel of the single-pixel class


def planted(B, n, Cs, Ct, NC, seed, device="cpu"):
    """relu_maps plus labels uniform in [-1, NC] (ignored and out-of-range pixels both occur) -> (S, T, y, plants).  From n >= 64,
    image 0 carries: class NC - 1 on exactly the pixels ZERO_ROWS, whose student rows are zeroed (m = 0); class NC - 2 on exactly the
    pixel SINGLE (s = 1 on both sides); with NC >= 4, class 1 absent; with more than one row slice, class 0 on both sides of the first
    slice boundary.  From B >= 2 (and n >= 64) image 1 has no kept pixel, so every class is absent from it."""
    S, T = relu_maps(B, n, Cs, Ct, seed)
    g = torch.Generator().manual_seed(seed + 7)
    y = torch.randint(-1, NC + 1, (B, n), generator=g)
    plants = {}
    if n >= 64:
        y0 = y[0]
        y0[(y0 == NC - 1) | (y0 == NC - 2)] = 0
        if NC >= 4:
            y0[y0 == 1] = 0
            plants["absent"] = 1
        y0[list(ZERO_ROWS)] = NC - 1
        S[0, list(ZERO_ROWS)] = 0
        y0[SINGLE] = NC - 2
        plants.update(zero=NC - 1, single=NC - 2)
        if slices(B, n) > 1:
            rows = slice_rows(B, n)
            y0[rows - 1] = y0[rows] = 0
            plants["straddle"] = (rows - 1, rows)
        if B >= 2:
            y[1] = torch.where(torch.arange(n) % 2 == 0, torch.full((n,), -1), torch.full((n,), NC))
            plants["empty"] = 1
    return S.to(device), T.to(device), y.to(device), plants


def exact_inputs(B, NC, N, extra, Cs, Ct, seed, device="cpu"):
    """Inputs on which every intermediate of the term is exactly representable.  Each image has NC classes of N pixels (N a multiple
    of 8) at shuffled positions plus `extra` pixels that are not kept; for class c with pixels p[0 .. N): the student's rows
    p[0 .. N/2) are 2 e_k, the rows p[N/2 + i] and p[3N/4 + i] are +a e_j and -a e_j (a in {1, 2, 4}, j != k), so m = e_k = mh and
    s is 1 on the first half and 0 on the second.  The teacher has the same construction on the pixels rotated by N/4 (with its own
    k, j, a), so sS - sT is 1, 0, -1, 0 on the four quarters.  With B, K_b = NC N and N powers of two every quotient is exact."""
    assert N % 8 == 0
    r = np.random.RandomState(seed)
    n = NC * N + extra
    S, T = np.zeros((B, n, Cs), np.float32), np.zeros((B, n, Ct), np.float32)
    y = np.zeros((B, n), np.int64)

    def fill(X, p, C):
        k = r.randint(C)
        X[p[:N // 2], k] = 2.0
        for i in range(N // 4):
            j = (k + 1 + r.randint(C - 1)) % C
            a = r.choice([1.0, 2.0, 4.0])
            X[p[N // 2 + i], j], X[p[3 * N // 4 + i], j] = a, -a
    for b in range(B):
        perm = r.permutation(n)
        for c in range(NC):
            p = perm[c * N:(c + 1) * N]
            y[b, p] = c
            fill(S[b], p, Cs)
            fill(T[b], np.roll(p, -(N // 4)), Ct)
        rest = perm[NC * N:]
        y[b, rest] = np.where(np.arange(len(rest)) % 2 == 0, -1, NC)
        S[b, rest] = r.randn(len(rest), Cs)
        T[b, rest] = r.randn(len(rest), Ct)
    return torch.from_numpy(S).to(device), torch.from_numpy(T).to(device), torch.from_numpy(y).to(device)
