"""One plain-torch KD objective for every hard-label term x feature term kdrt.losses.kd_objective accepts, written from the
definitions in the kdrt/losses.py docstrings and DESIGN.md section 3, differentiable by torch.autograd and evaluated in the dtype
of its inputs (float64: the reference; float32: the self-check of tests/test_fp64_objective_ref_host.py):

    total = hard + alpha * T^2 * KL + beta * (feature(camera_feat) + feature(lidar_feat))

    hard:    None (weighted CE) | RegionLoss | LovaszLoss(base = None or a RegionLoss) | OhemCE
    feature: None (MSE) | ChannelKD | PairKD | IntraClassKD

It calls none of the per-term references for a value: tests/test_fp64_objective_ref_host.py pins every term of it, value and
gradient, against them.  The two discrete choices are taken the way the per-term files take them and then held constant:

  * OhemCE: the mined set is tests/_ohem_ref.select on the float32 bits of l = -log p_y evaluated in float32 (`ohem_keep`);
  * LovaszLoss: the order is tests/_fp64_lovasz_ref.own_order of the float64 errors.

`stability` is the condition under which those choices are the device's as well: the gap between theta and the nearest l, and
between neighbouring Lovasz errors, exceeds the float32 error bound of those quantities.  The inputs of every case (`CASES`,
`case_setup`) are chosen so that it holds; the host test asserts it for every case the GPU test uses.

The spec classes below mirror the fields of the kdrt.losses classes of the same name (`to_kdrt` converts), so this module does
not import kdrt.  Scalars (T, alpha, beta, the specs' parameters) enter as the fp32 values the C ABI receives."""
import collections
import math

import numpy as np
import torch

import _fp64_loss_ref as L
import _fp64_lovasz_ref as LV
import _ohem_ref as OH

EPS = 1e-12
f32 = L.f32

RegionLoss = collections.namedtuple("RegionLoss", "gamma wf wt a b s", defaults=(2.0, 1.0, 1.0, 0.7, 0.3, 1.0))
LovaszLoss = collections.namedtuple("LovaszLoss", "weight base", defaults=(1.0, None))
OhemCE = collections.namedtuple("OhemCE", "thresh min_divisor min_kept", defaults=(0.7, 16, 1))
ChannelKD = collections.namedtuple("ChannelKD", "tau", defaults=(4.0,))
PairKD = collections.namedtuple("PairKD", "")
IntraClassKD = collections.namedtuple("IntraClassKD", "")

FEATURE_NAMES = {None: "mse", ChannelKD: "cwd", PairKD: "pair", IntraClassKD: "ifv"}


def to_kdrt(spec):
    """the kdrt.losses object of a spec of this module"""
    from kdrt import losses
    if spec is None:
        return None
    kw = spec._asdict()
    if isinstance(spec, LovaszLoss):
        kw["base"] = to_kdrt(spec.base)
    return getattr(losses, type(spec).__name__)(**kw)


def feature_prefix(feature):
    return FEATURE_NAMES[None if feature is None else type(feature)]


def part_names(hard, feature, autograd_form=False):
    """the keys kd_objective documents for a combination ("class_lovasz" comes from the autograd form only)"""
    p = feature_prefix(feature)
    names = {"ce", "kl", p + "_cam", p + "_lidar"}
    if isinstance(hard, RegionLoss):
        names |= {"focal", "tversky"}
    elif isinstance(hard, LovaszLoss):
        names |= {"lovasz"} | ({"class_lovasz"} if autograd_form else set()) | ({"focal", "tversky"} if hard.base is not None else set())
    elif isinstance(hard, OhemCE):
        names |= {"ce_all", "ohem_theta", "ohem_kept"}
    return names


# ---- the hard-label terms ---------------------------------------------------------------------------------------------------------

def kept(target, NC, ignore_index):
    return (target != ignore_index) & (target >= 0) & (target < NC)


def _pixels(zs, target, cw, ignore_index):
    """zs [B, NC, HW], target [B, HW] -> keep [B, HW], ys (0 where dropped), log p, p [B, NC, HW], w [B, HW] (0 where dropped)"""
    NC = zs.shape[1]
    keep = kept(target, NC, ignore_index)
    ys = torch.where(keep, target, torch.zeros_like(target))
    lp = torch.log_softmax(zs, 1)
    w = (torch.ones(NC, dtype=zs.dtype) if cw is None else cw.to(zs.dtype))[ys] * keep
    return keep, ys, lp, lp.exp(), w


def weighted_ce(zs, target, cw, ignore_index, subset=None):
    """sum_K w[y] (-log p_y) / sum_K w[y]; subset: a mask that narrows K (the mined set)"""
    keep, ys, lp, _, w = _pixels(zs, target, cw, ignore_index)
    if subset is not None:
        w = w * subset
    nll = -lp.gather(1, ys.unsqueeze(1)).squeeze(1)
    return (w * nll).sum() / w.sum()


def kl_term(zs, zt, T):
    """per-pixel mean of KL(softmax(zt / T) || softmax(zs / T)) over all B * HW pixels, labelled or not"""
    invT = float(np.float32(1.0) / np.float32(T))
    lps, lpt = torch.log_softmax(zs * invT, 1), torch.log_softmax(zt * invT, 1)
    return (lpt.exp() * (lpt - lps)).sum() / (zs.shape[0] * zs.shape[2])


def region_term(zs, target, cw, ignore_index, spec):
    """-> (wf * Focal + wt * Tversky, Focal, Tversky); a term whose weight is 0 reads 0"""
    gamma, wf, wt, a, b, s = (f32(v) for v in spec)
    NC = zs.shape[1]
    keep, ys, lp, p, w = _pixels(zs, target, cw, ignore_index)
    kf = keep.to(zs.dtype).unsqueeze(1)
    oh = torch.zeros_like(zs).scatter_(1, ys.unsqueeze(1), 1.0) * kf
    zero = torch.zeros((), dtype=zs.dtype)
    focal = tv = zero
    if wf > 0:
        om = (p * (kf - oh)).sum(1)                                  # 1 - p_y as the sum of the other classes' probabilities
        fac = torch.ones_like(om) if gamma == 0 else om ** gamma
        focal = (w * fac * -(lp * oh).sum(1)).sum() / w.sum()
    if wt > 0:
        TP, A, N = (p * oh).sum((0, 2)), (p * kf).sum((0, 2)), oh.sum((0, 2))
        tv = 1.0 - ((TP + s) / (TP + a * (A - TP) + b * (N - TP) + s)).sum() / NC
    return wf * focal + wt * tv, focal, tv


def lovasz_term(zs, target, ignore_index, order):
    """Lovasz-Softmax, classes "present", per image, along the given order [B, NC, HW] (-1 past the kept count)
    -> (L, per class the mean of L_{b,c} over the images where the class is present)"""
    B, NC, HW = zs.shape
    dt = zs.dtype
    keep = kept(target, NC, ignore_index)
    p = torch.softmax(zs, 1)
    lbc = [[None] * NC for _ in range(B)]
    img = []
    for b in range(B):
        here = []
        for c in range(NC):
            fg = (target[b] == c) & keep[b]
            if not bool(fg.any()):
                continue
            idx = order[b, c]
            idx = idx[idx >= 0]
            others = torch.stack([p[b, j] for j in range(NC) if j != c]).sum(0)      # the OTHER probabilities, never 1 - p_c
            e = torch.where(fg, others, p[b, c])[idx]
            f = fg[idx].to(dt)
            G = f.sum()
            inter = G - torch.cumsum(f, 0)
            union = G + torch.cumsum(1.0 - f, 0)
            J = 1.0 - inter / union
            g = J - torch.cat([torch.zeros(1, dtype=dt), J[:-1]])
            lbc[b][c] = (e * g).sum()
            here.append(lbc[b][c])
        img.append(torch.stack(here).mean() if here else torch.zeros((), dtype=dt))
    cm = []
    for c in range(NC):
        v = [lbc[b][c] for b in range(B) if lbc[b][c] is not None]
        cm.append(torch.stack(v).mean() if v else torch.zeros((), dtype=dt))
    return torch.stack(img).sum() / B, torch.stack(cm)


def ohem_nll32(zs, target, ignore_index):
    """l = -log p_y evaluated in float32 from the float32 logits: what the selection reads -> (valid [B, HW], l float32 [B, HW])"""
    z = zs.detach().float()
    valid = kept(target, z.shape[1], ignore_index)
    ys = torch.where(valid, target, torch.zeros_like(target))
    l = -torch.log_softmax(z, 1).gather(1, ys.unsqueeze(1)).squeeze(1)
    return valid, torch.where(valid, l.clamp_min(0.0), torch.zeros_like(l))


def ohem_keep(zs, target, ignore_index, spec):
    """-> (keep bool [B, HW], m, whether the rank decides) by _ohem_ref.select on the float32 bits of l"""
    valid, l = ohem_nll32(zs, target, ignore_index)
    lam = OH.lam_of(spec.thresh)
    m, tau, theta, keep = OH.select(l, valid, lam, spec.min_kept, spec.min_divisor)
    return torch.from_numpy(keep.reshape(tuple(target.shape))), m, tau is not None and float(tau) < lam


def ohem_term(zs, target, cw, ignore_index, spec, keep):
    """-> (the weighted CE over the mined set, over all of K, theta, |S| / n); the set is a constant of the gradient"""
    valid = kept(target, zs.shape[1], ignore_index)
    _, ys, lp, _, _ = _pixels(zs, target, cw, ignore_index)
    l = -lp.detach().gather(1, ys.unsqueeze(1)).squeeze(1)[valid]
    n = int(valid.sum())
    m = OH.count_to_keep(n, spec.min_kept, spec.min_divisor)
    tau = torch.sort(l, descending=True)[0][m - 1]
    theta = torch.minimum(tau, torch.tensor(OH.lam_of(spec.thresh), dtype=zs.dtype))
    share = torch.tensor(int(keep.sum()) / n, dtype=zs.dtype)
    return weighted_ce(zs, target, cw, ignore_index, keep), weighted_ce(zs, target, cw, ignore_index).detach(), theta, share


# ---- the feature terms: S [B, Cs, H, W], T [B, Ct, H, W] --------------------------------------------------------------------------

def _rows(X):
    """[B, C, H, W] -> the NHWC matrix [B, H * W, C]"""
    return X.permute(0, 2, 3, 1).reshape(X.shape[0], -1, X.shape[1])


def _unit_rows(X):
    """rows of [..., C] scaled to unit length, all-zero where the norm is at most 1e-12 (and no gradient through such a row)"""
    ss = X.pow(2).sum(-1, keepdim=True)
    live = ss.detach().sqrt() > EPS
    return torch.where(live, X / torch.where(live, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(X))


def mse_term(S, T):
    return (S - T).pow(2).mean()


def cwd_term(S, T, tau):
    """tau^2 / (B * C) * sum_{b,c} KL(phi(T) || phi(S)), phi: the temperature softmax down the H * W positions of a channel"""
    B, C = S.shape[:2]
    ls, lt = torch.log_softmax(S.reshape(B, C, -1) / tau, 2), torch.log_softmax(T.reshape(B, C, -1) / tau, 2)
    return tau * tau / (B * C) * (lt.exp() * (lt - ls)).sum()


def pair_term(S, T):
    """1 / B * sum_b 1 / n^2 * sum_ij (a^S_ij - a^T_ij)^2, a: the cosine similarity of two positions"""
    Sh, Th = _unit_rows(_rows(S)), _unit_rows(_rows(T))
    n = Sh.shape[1]
    D = Sh @ Sh.transpose(1, 2) - Th @ Th.transpose(1, 2)
    return (D.pow(2).sum((1, 2)) / (n * n)).mean()


def _own_class_similarity(X, y, keep, NC):
    """one image [n, C] -> s [n]: the cosine of every kept pixel to the unit prototype of its own class (0 elsewhere)"""
    xh = _unit_rows(X)
    s = torch.zeros(X.shape[0], dtype=X.dtype)
    for c in range(NC):
        sel = keep & (y == c)
        if not bool(sel.any()):
            continue
        m = X[sel].mean(0)
        nrm = m.pow(2).sum().sqrt()
        mh = m / nrm if nrm.item() > EPS else torch.zeros_like(m)
        s = torch.where(sel, xh @ mh, s)
    return s


def ifv_term(S, T, target, NC, ignore_index):
    """1 / B * sum_b 1 / K_b * sum_kept (sS_i - sT_i)^2 (an image without a kept pixel adds 0 and counts in B)"""
    Sm, Tm = _rows(S), _rows(T)
    B = Sm.shape[0]
    y = target.reshape(B, -1)
    keep = kept(y, NC, ignore_index)
    tot = torch.zeros((), dtype=S.dtype)
    for b in range(B):
        K = int(keep[b].sum())
        if K:
            d = _own_class_similarity(Sm[b], y[b], keep[b], NC) - _own_class_similarity(Tm[b], y[b], keep[b], NC)
            tot = tot + d.pow(2).sum() / K
    return tot / B


# ---- the objective ----------------------------------------------------------------------------------------------------------------

def objective(zs, ms, zt, mt, target, cw, T, alpha, beta, ignore_index, hard, feature, keep=None, order=None):
    """zs, zt [B, NC, H, W]; ms, mt: {"camera_feat", "lidar_feat"} of [B, C, H, W]; target int64 [B, H, W] on the logits' grid (and,
    for IntraClassKD, the feature maps').  -> (total, parts): the keys of kd_objective's parts, "class_lovasz" included.
    keep / order: the discrete choices, taken here as the module docstring says when not given."""
    B, NC = zs.shape[:2]
    z3, zt3, y2 = zs.reshape(B, NC, -1), zt.reshape(B, NC, -1), target.reshape(B, -1)
    parts = {}
    kl = kl_term(z3, zt3.detach(), T)
    if hard is None:
        ce = weighted_ce(z3, y2, cw, ignore_index)
    elif isinstance(hard, OhemCE):
        if keep is None:
            keep = ohem_keep(z3, y2, ignore_index, hard)[0]
        ce, parts["ce_all"], parts["ohem_theta"], parts["ohem_kept"] = ohem_term(z3, y2, cw, ignore_index, hard, keep.reshape(B, -1))
    else:
        base = hard.base if isinstance(hard, LovaszLoss) else hard
        if base is None:
            ce = weighted_ce(z3, y2, cw, ignore_index)
        else:
            ce, parts["focal"], parts["tversky"] = region_term(z3, y2, cw, ignore_index, base)
        if isinstance(hard, LovaszLoss):
            if order is None:
                order = LV.own_order(z3.detach(), y2, ignore_index)
            parts["lovasz"], parts["class_lovasz"] = lovasz_term(z3, y2, ignore_index, order)
            ce = ce + f32(hard.weight) * parts["lovasz"]
    pre = feature_prefix(feature)
    for key, name in (("camera_feat", pre + "_cam"), ("lidar_feat", pre + "_lidar")):
        S, Tm = ms[key], mt[key].detach()
        if feature is None:
            parts[name] = mse_term(S, Tm)
        elif isinstance(feature, ChannelKD):
            parts[name] = cwd_term(S, Tm, f32(feature.tau))
        elif isinstance(feature, PairKD):
            parts[name] = pair_term(S, Tm)
        else:
            parts[name] = ifv_term(S, Tm, target, NC, ignore_index)
    total = ce + (alpha * T * T) * kl + beta * (parts[pre + "_cam"] + parts[pre + "_lidar"])
    parts.update(ce=ce, kl=kl)
    return total, {k: v.detach() for k, v in parts.items()}


# ---- when the discrete choices are the device's too -------------------------------------------------------------------------------

def lovasz_gap_ratio(zs, target, ignore_index):
    """zs [B, NC, HW] float64 -> the smallest (e_k - e_{k+1}) / (bound_k + bound_{k+1}) between neighbours of the float64 order over
    every (image, class); above 1 the float32 errors sort the same way (inf when no list has two pixels)"""
    r = LV.errors(zs, target, ignore_index)
    order = LV.own_order(zs, target, ignore_index)
    worst = math.inf
    for b in range(zs.shape[0]):
        for c in range(zs.shape[1]):
            idx = order[b, c]
            idx = idx[idx >= 0]
            if idx.numel() > 1:
                es, ee = r["e"][b, c, idx], r["e_e"][b, c, idx]
                worst = min(worst, ((es[:-1] - es[1:]) / (ee[:-1] + ee[1:])).min().item())
    return worst


def ohem_gap(zs, target, ignore_index, spec):
    """zs [B, NC, HW] float64 -> dict: `same` (the float32 selection is the float64 one), `loose` (pixels within their float32 bound
    of theta other than the one that attains it when the rank decides), `rank` (whether the rank decides), `gap` (the distance
    from theta to the nearest other l), `e_theta`"""
    valid, l, e_l = OH.per_pixel(zs, target, ignore_index)
    lam = OH.lam_of(spec.thresh)
    s = OH.select64(l, e_l, valid, lam, spec.min_kept, spec.min_divisor)
    keep32, m, rank = ohem_keep(zs, target, ignore_index, spec)
    d = (l.reshape(-1) - s["theta"]).abs()[valid.reshape(-1)]
    d = torch.sort(d)[0]
    gap = (d[1] if rank else d[0]).item()
    return {"same": bool((keep32.reshape(-1) == s["keep"]).all()) and m == s["m"], "loose": int(s["margin"].sum()) - (1 if rank else 0),
            "rank": rank, "gap": gap, "e_theta": s["e_theta"] if rank else 0.0, "theta": s["theta"], "share": int(s["keep"].sum()) / int(valid.sum())}


def stability(zs, target, ignore_index, hard):
    """-> (ok, text) for the discrete choices `hard` makes on these inputs"""
    if isinstance(hard, LovaszLoss):
        r = lovasz_gap_ratio(zs, target, ignore_index)
        return r > 1.0, f"smallest Lovasz error gap / float32 bound {r:.3g}"
    if isinstance(hard, OhemCE):
        g = ohem_gap(zs, target, ignore_index, hard)
        return g["same"] and g["loose"] == 0, (f"theta {g['theta']:.6g} ({'rank' if g['rank'] else 'threshold'} decides), nearest l at {g['gap']:.3g}, "
                                               f"{g['loose']} pixels inside the float32 margin, float32 set equal {g['same']}")
    return True, "no discrete choice"


# ---- the cases of tests/test_gpu_objective_matrix.py (a) and of the host test -------------------------------------------------------

REGION = RegionLoss(gamma=2.0, wf=1.0, wt=0.8, a=0.7, b=0.3, s=1.0)
HARDS = {"ce": None, "region": REGION, "lovasz": LovaszLoss(0.7, None), "ohem": OhemCE(0.7, 4, 8)}
LOVASZ_REGION = LovaszLoss(1.5, REGION)
OHEM_RANK = OhemCE(1e-30, 3, 1)                   # lambda = 69 above every l: the rank decides
FEATURES = {"mse": None, "cwd": ChannelKD(4.0), "pair": PairKD(), "ifv": IntraClassKD()}
COMBOS = [(h, f) for h in HARDS for f in FEATURES]
# B, H, W and per feature term the (student, teacher) widths of (camera_feat, lidar_feat): 16 x 16 with every term at its smallest
# width; 12 x 20 (240 pixels, no multiple of 256 in an image or in the batch) at widths that are no power of two, student and teacher
# differing where the term allows it.  The two maps always differ in data, in the second shape in width as well.
SHAPES = {"b2_16x16": (2, 16, 16, {"mse": ((4, 4), (4, 4)), "cwd": ((4, 4), (4, 4)), "pair": ((4, 4), (4, 4)), "ifv": ((4, 4), (4, 4))}),
          "b3_12x20": (3, 12, 20, {"mse": ((12, 12), (20, 20)), "cwd": ((12, 12), (20, 20)), "pair": ((8, 12), (12, 20)), "ifv": ((8, 12), (12, 20))})}
T_KD, ALPHA, BETA = 4.0, f32(0.7), f32(0.7)
Case = collections.namedtuple("Case", "hard feature NC shape ign")


def class_counts(hard):
    """2 and 4 for every combination, 3 where the Lovasz / region kernels run, 8 and 16 where only the CE family does"""
    return (2, 3, 4) if hard in ("region", "lovasz") else (2, 4, 8, 16)


def _cases():
    out = []
    for h, f in COMBOS:
        for i, NC in enumerate(class_counts(h)):
            out.append(Case(h, f, NC, ("b2_16x16", "b3_12x20")[(i + COMBOS.index((h, f))) % 2], -1))
    # ignore_index = 0: class 0 is the one that is dropped, once per hard-label row and once per feature term
    out += [Case("ce", "ifv", 4, "b3_12x20", 0), Case("region", "pair", 3, "b2_16x16", 0), Case("lovasz", "cwd", 4, "b2_16x16", 0),
            Case("ohem", "mse", 8, "b3_12x20", 0)]
    return out


CASES = _cases()


def case_id(c):
    return f"{c.hard}+{c.feature}-nc{c.NC}-{c.shape}" + ("" if c.ign == -1 else f"-ign{c.ign}")


def case_specs(c):
    """-> (hard, feature) specs of a case: the Lovasz row runs over the CE at 2 and 4 classes and over a RegionLoss at 3 (and at 4
    with ignore_index = 0); the OhemCE row lets the threshold decide at 2 and 8 classes and the rank at 4 and 16"""
    hard = HARDS[c.hard]
    if c.hard == "lovasz" and (c.NC == 3 or c.ign != -1):
        hard = LOVASZ_REGION
    if c.hard == "ohem" and c.NC in (4, 16):
        hard = OHEM_RANK
    return hard, FEATURES[c.feature]


def make_inputs(c, seed):
    """float32 CPU tensors of a case -> dict(zs, zt, target, cw, ms, mt).  Logits N(0, 2^2); labels uniform over the classes with
    about 10 % ignore_index and 2 % each NC + 1 and -7; class NC - 1 is absent from the last image.  Feature maps: ReLU'd normal maps,
    one all-zero position in the student's camera map."""
    B, H, W, widths = SHAPES[c.shape]
    NC = c.NC
    g = torch.Generator().manual_seed(seed)
    zs = torch.randn(B, NC, H, W, generator=g) * 2.0
    zt = torch.randn(B, NC, H, W, generator=g) * 2.0
    y = torch.randint(0, NC, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    for lo, hi, bad in ((0.0, 0.1, c.ign), (0.1, 0.12, NC + 1), (0.12, 0.14, -7)):
        y = torch.where((r >= lo) & (r < hi), torch.full_like(y, bad), y)
    y[B - 1] = torch.where(y[B - 1] == NC - 1, torch.full_like(y[B - 1], 1 if c.ign == 0 else 0), y[B - 1])
    cw = torch.rand(NC, generator=g) * 3 + 0.2
    ms, mt = {}, {}
    for key, (cs, ct) in zip(("camera_feat", "lidar_feat"), widths[c.feature]):
        ms[key] = torch.randn(B, cs, H, W, generator=g).clamp_min(0)
        mt[key] = torch.randn(B, ct, H, W, generator=g).clamp_min(0)
        if cs == ct:                                                 # a trained pair: the teacher near the student
            mt[key] = (0.7 * ms[key] + 0.6 * mt[key]).contiguous()
    ms["camera_feat"][:, :, H // 3, W // 3] = 0
    return dict(zs=zs, zt=zt, target=y, cw=cw, ms=ms, mt=mt)


# The input seed of a case.  Cases with a discrete choice take the first seed from 1000 + 100 * index on for which `stability` holds
# on the float64 reference alone (scanned on the CPU; tests/test_fp64_objective_ref_host.py asserts the condition for every case).
SEED_OFFSETS = {"lovasz+mse-nc2-b2_16x16": 7, "lovasz+mse-nc3-b3_12x20": 11, "lovasz+mse-nc4-b2_16x16": 24, "lovasz+cwd-nc3-b2_16x16": 11,
                "lovasz+cwd-nc4-b3_12x20": 13, "lovasz+pair-nc2-b2_16x16": 1, "lovasz+pair-nc3-b3_12x20": 8, "lovasz+pair-nc4-b2_16x16": 10,
                "lovasz+ifv-nc2-b3_12x20": 5, "lovasz+ifv-nc3-b2_16x16": 17, "lovasz+ifv-nc4-b3_12x20": 70,
                "lovasz+cwd-nc4-b2_16x16-ign0": 9}


def case_seed(c):
    i = CASES.index(c)
    return 1000 + 100 * i + SEED_OFFSETS.get(case_id(c), 0)


def case_setup(c, dtype=torch.float64, seed=None):
    """-> (inputs cast to dtype with the differentiable leaves requiring grad, hard, feature)"""
    t = make_inputs(c, case_seed(c) if seed is None else seed)
    cv = lambda x, grad=False: x.to(dtype).clone().requires_grad_(grad)
    hard, feature = case_specs(c)
    return dict(zs=cv(t["zs"], True), zt=cv(t["zt"]), target=t["target"], cw=cv(t["cw"]),
                ms={k: cv(v, True) for k, v in t["ms"].items()}, mt={k: cv(v) for k, v in t["mt"].items()}), hard, feature


def case_objective(c, inp, hard, feature, **kw):
    return objective(inp["zs"], inp["ms"], inp["zt"], inp["mt"], inp["target"], inp["cw"], T_KD, ALPHA, BETA, c.ign, hard, feature, **kw)


def flat3(inp):
    """the [B, NC, HW] / [B, HW] views the per-term references take"""
    zs = inp["zs"].detach()
    B, NC = zs.shape[:2]
    return zs.reshape(B, NC, -1), inp["zt"].detach().reshape(B, NC, -1), inp["target"].reshape(B, -1)


# ---- one KD step through the model against the float64 oracle: the cases of tests/test_gpu_objective_matrix.py (c) ---------------------
# name: (hard, feature, classes, BEV grid, keep one label in ...).  Every term appears once; the last case puts an 8 x 8 BEV grid under
# the 16 x 16 camera map, so the LiDAR term's gradient is deposited for the RESIZED map.  The Lovasz case labels one pixel in 16 (the
# rest ignore_index, as sparse BEV labels are): among the ~250 labelled pixels of a dense image no batch keeps every pair of
# neighbouring errors 10 * LOGIT_TOL apart (the gaps of n values in [0, 1] average 1 / n), among ~16 some do.
STEP_CASES = {"region+cwd": (REGION, ChannelKD(4.0), 2, 16, 1), "lovasz_region+pair": (LOVASZ_REGION, PairKD(), 2, 16, 16),
              "ohem+ifv-nc8": (HARDS["ohem"], IntraClassKD(), 8, 16, 1), "ce+ifv-grid8": (None, IntraClassKD(), 2, 8, 1)}
STEP_CW8 = (0.4, 3.5, 1.0, 2.0, 0.7, 1.5, 3.0, 0.9)          # tests/test_gpu_multiclass_step.py
STEP_GAP = 1e-3                                              # 10 * _fp64_step_ref.LOGIT_TOL


def step_batch(name, seed):
    """(images, points, labels) of a step case on the CPU: the images and points of _fp64_step_ref's shapes for the case's BEV grid,
    labels on the 16 x 16 grid of the logits and of both feature maps"""
    import kd_oracle as O
    import _fp64_step_ref as R
    _, _, nc, grid, every = STEP_CASES[name]
    images, pts, _ = O.make_inputs(R.B, R.HW, R.N, grid, seed, pad_tail=R.PAD_TAIL)
    labels = O.make_inputs(R.B, R.HW, R.N, R.HW // 4, seed, pad_tail=R.PAD_TAIL, num_classes=nc)[2]
    if every > 1:
        r = torch.rand(labels.shape, generator=torch.Generator().manual_seed(77 + seed))
        labels = torch.where(r < 1.0 / every, labels, torch.full_like(labels, -1))
    return images, pts, labels


def step_objective(name):
    """the case's objective with kd_oracle.kd_loss's signature, its parts the scalars a KDStep reports"""
    hard, feature = STEP_CASES[name][:2]

    def run(zs, ms, zt, mt, labels, cw, T, alpha, beta):
        total, parts = objective(zs, ms, zt, mt, labels, cw, T, alpha, beta, -1, hard, feature)
        return total, {k: v for k, v in parts.items() if k != "class_lovasz"}
    return run


def step_gaps(name, logits, labels):
    """float64 logits [B, NC, H, W] of the student's forward pass -> (ok, text): theta at least STEP_GAP from every other l, every
    pair of neighbouring Lovasz errors at least STEP_GAP apart, and the float32 selection equal to the float64 one"""
    hard = STEP_CASES[name][0]
    B, NC = logits.shape[:2]
    zs, y = logits.detach().double().reshape(B, NC, -1), labels.reshape(B, -1)
    if isinstance(hard, OhemCE):
        g = ohem_gap(zs, y, -1, hard)
        return g["same"] and g["loose"] == 0 and g["gap"] > STEP_GAP, f"theta {g['theta']:.6g}, nearest other l at {g['gap']:.3g}, float32 set equal {g['same']}"
    if isinstance(hard, LovaszLoss):
        r, order, worst, n = LV.errors(zs, y, -1), LV.own_order(zs, y, -1), math.inf, 0
        for b in range(B):
            for c in range(NC):
                idx = order[b, c]
                idx = idx[idx >= 0]
                n = max(n, idx.numel())
                if idx.numel() > 1:
                    es = r["e"][b, c, idx]
                    worst = min(worst, (es[:-1] - es[1:]).min().item())
        return worst > STEP_GAP and n > 1, f"smallest gap between neighbouring Lovasz errors {worst:.3g} ({n} labelled pixels in the fullest image)"
    return True, "no discrete choice"
