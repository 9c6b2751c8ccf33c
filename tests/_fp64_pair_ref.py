"""Float64 reference of the pair-wise distillation feature term (kdrt.losses.PairKD, csrc/kd_loss_pair.hip).

  direct(S, T)  the definition with the explicit n x n affinity matrices, in the dtype of its inputs (float64 in the tests)
  gram(S, T)    the Gram formulation in the dtype of its inputs: the identity tr(A A^T B B^T) = |A^T B|_F^2 the kernels rest on
  gram32(S, T)  the Gram formulation in float32 numpy matmuls, the final sums in double: what fp32 costs in this formulation

S [B, n, Cs] and T [B, n, Ct] are the NHWC matrices of the two maps.  For image b:
  r_i = sqrt(sum_c x_ic^2), xh_i = x_i / r_i if r_i > 1e-12 else 0 (such a row receives no gradient), a_ij = xh_i . xh_j,
  L_b = 1/n^2 sum_ij (a^S_ij - a^T_ij)^2,  PAIR = 1/B sum_b L_b,
  dPAIR/dSh_b = 4/(B n^2) (Sh_b Gss - Th_b Gts) =: gh,  dPAIR/dS_i = (gh_i - xh_i (xh_i . gh_i)) / r_i."""
import numpy as np
import torch

U = 2.0 ** -24
EPS = 1e-12


def f32(x):
    return float(np.float32(x))


def normalise(X):
    """-> (Xh, r, live): unit rows, the norms, and the mask of the rows whose norm is above 1e-12"""
    r = X.pow(2).sum(-1, keepdim=True).sqrt()
    live = r > EPS
    return torch.where(live, X / torch.where(live, r, torch.ones_like(r)), torch.zeros_like(X)), r, live


def _backward_norm(gh, Xh, r, live):
    g = (gh - Xh * (Xh * gh).sum(-1, keepdim=True)) / torch.where(live, r, torch.ones_like(r))
    return torch.where(live, g, torch.zeros_like(g))


def direct(S, T):
    """the definition, n x n affinities and all -> dict(val, img [B], grad [B, n, Cs], M [B, n, Cs], Sv, Sv_img [B]).
    M = 4/(B n^2) (|Sh| |Gss| + |Th| |Gts|) / r is the magnitude that cancels in a gradient element, Sv = (|Gss|^2 + 2 |Gts|^2 +
    |Gtt|^2) / (B n^2) the one that cancels in the value (Sv_img: per image, / n^2)."""
    B, n, _ = S.shape
    Sh, rs, ls = normalise(S)
    Th, _, _ = normalise(T)
    img, grads, Ms, Svs = [], [], [], []
    for b in range(B):
        D = Sh[b] @ Sh[b].T - Th[b] @ Th[b].T                       # a^S - a^T, [n, n]
        img.append(D.pow(2).sum() / (n * n))
        gh = (4.0 / (B * n * n)) * (D @ Sh[b])                       # dPAIR/dSh: D is symmetric
        grads.append(_backward_norm(gh, Sh[b], rs[b], ls[b]))
        Gss, Gts, Gtt = Sh[b].T @ Sh[b], Th[b].T @ Sh[b], Th[b].T @ Th[b]
        M = (4.0 / (B * n * n)) * (Sh[b].abs() @ Gss.abs() + Th[b].abs() @ Gts.abs()) / torch.where(ls[b], rs[b], torch.ones_like(rs[b]))
        Ms.append(torch.where(ls[b], M, torch.zeros_like(M)))
        Svs.append((Gss.pow(2).sum() + 2 * Gts.pow(2).sum() + Gtt.pow(2).sum()) / (n * n))
    img, Sv_img = torch.stack(img), torch.stack(Svs)
    return {"val": img.sum() / B, "img": img, "grad": torch.stack(grads), "M": torch.stack(Ms), "Sv": Sv_img.sum() / B, "Sv_img": Sv_img}


def gram(S, T):
    """the Gram formulation in the inputs' dtype -> dict(val, img, grad)"""
    B, n, _ = S.shape
    Sh, rs, ls = normalise(S)
    Th, _, _ = normalise(T)
    Gss, Gts, Gtt = Sh.transpose(1, 2) @ Sh, Th.transpose(1, 2) @ Sh, Th.transpose(1, 2) @ Th
    img = (Gss.pow(2).sum((1, 2)) - 2 * Gts.pow(2).sum((1, 2)) + Gtt.pow(2).sum((1, 2))) / (n * n)
    gh = (4.0 / (B * n * n)) * (Sh @ Gss - Th @ Gts)
    return {"val": img.sum() / B, "img": img, "grad": _backward_norm(gh, Sh, rs, ls)}


def gram32(S, T):
    """the Gram formulation with float32 numpy matmuls and float32 normalisation; the value's sums and the coefficient 4/(B n^2) in
    double -> dict(val, img, grad) as float64 torch tensors on the CPU"""
    S32, T32 = S.detach().cpu().numpy().astype(np.float32), T.detach().cpu().numpy().astype(np.float32)
    B, n, _ = S32.shape

    def norm32(X):
        r = np.sqrt((X * X).sum(-1, keepdims=True, dtype=np.float32))
        live = r > np.float32(EPS)
        return np.where(live, X / np.where(live, r, np.float32(1)), np.float32(0)).astype(np.float32), r, live
    img, grads = [], []
    for b in range(B):
        Sh, r, live = norm32(S32[b])
        Th, _, _ = norm32(T32[b])
        Gss, Gts, Gtt = Sh.T @ Sh, Th.T @ Sh, Th.T @ Th
        d = lambda G: (G.astype(np.float64) ** 2).sum()
        img.append((d(Gss) - 2 * d(Gts) + d(Gtt)) / (float(n) * n))
        gh = Sh @ Gss - Th @ Gts
        g = (gh - Sh * (Sh * gh).sum(-1, keepdims=True, dtype=np.float32)) / np.where(live, r, np.float32(1))
        grads.append(np.where(live, g, np.float32(0)).astype(np.float64) * (4.0 / (B * float(n) * n)))
    img = np.array(img)
    return {"val": torch.tensor(img.sum() / B, dtype=torch.float64), "img": torch.from_numpy(img),
            "grad": torch.from_numpy(np.stack(grads))}


def relu_maps(B, n, Cs, Ct, seed, device="cpu"):
    """ReLU'd normal maps as fp32 [B, n, C], one all-zero row in each (row n // 3 of S, row 2 n // 3 of T: the same row when n = 1)"""
    g = torch.Generator().manual_seed(seed)
    S = torch.randn(B, n, Cs, generator=g).clamp_min(0)
    T = torch.randn(B, n, Ct, generator=g).clamp_min(0)
    S[:, n // 3] = 0
    T[:, (2 * n) // 3] = 0
    return S.to(device), T.to(device)


def exact_maps(B, n, C, seed, device="cpu"):
    """[B, n, C] fp32 whose rows have one nonzero entry of magnitude 1, 2 or 4, or four of one magnitude 0.5, 1 or 2, signs mixed:
    every row norm is a power of two, every normalised entry +-1 or +-0.5, and every sum of the term is exact in fp32"""
    r = np.random.RandomState(seed)
    X = np.zeros((B, n, C), np.float32)
    for b in range(B):
        for i in range(n):
            if r.rand() < 0.5:
                X[b, i, r.randint(C)] = r.choice([1.0, 2.0, 4.0]) * r.choice([-1.0, 1.0])
            else:
                X[b, i, r.choice(C, 4, replace=False)] = r.choice([0.5, 1.0, 2.0]) * r.choice([-1.0, 1.0], 4)
    return torch.from_numpy(X).to(device)


def slices(B, HW):
    """mirror of kd_feat_pair_slices: 1 once B alone fills 256 CUs, else up to ceil(256 / B) slices of at least 64 rows, cut at
    multiples of 32 rows"""
    want = 1 if B >= 256 else -(-256 // B)
    s = min(want, -(-HW // 64))
    rows = -(-(-(-HW // s)) // 32) * 32
    return -(-HW // rows)
