"""References for csrc/kd_loss_ohem.hip (kd_seg_ohem_fwd_bwd), the online-hard-example-mining cross-entropy of DESIGN.md section 3:

    K = the pixels the weighted CE keeps, n = |K|, l_i = -log p_{y_i},  m = min(n, max(min_kept, ceil(n / min_divisor))),
    theta = min(m-th largest l, lambda),  S = { i in K : l_i >= theta },  L = sum_S w[y] l / sum_S w[y],  S constant in the gradient.

Two parts, pure numpy / torch on any device:

  select(nll_f32, mask, lam, min_kept, min_divisor)   the selection on the fp32 BITS of whatever l it is given (np.partition on uint32
      views; l >= 0 with the sign bit clear, so the bits order as the values, a NaN above every number): exact, no tolerance.
  ohem(zs, zt, y, cw, ign, T, alpha, gs, keep, n_seq)  value and gradient over a GIVEN kept set: exactly _fp64_loss_ref.seg_loss on a
      target whose pixels outside S are set to ignore_index, so that function's bounds (C_BOUND * n_seq * U * sum |t|, n_seq =
      seg_n_seq(npix)) apply unchanged; evaluated in the inputs' dtype like everything in _fp64_loss_ref.

per_pixel gives l with the per-pixel bound e_lp of _fp64_loss_ref._softmax; select64 is the selection on float64 values together with
the margin inside which fp32 and float64 may legitimately disagree about a pixel:
    the device's l_i lies within e_i of the float64 l_i, so its m-th largest lies between the m-th largest of (l - e) and of (l + e);
    e_theta = the larger distance of those two from the float64 tau_m, and not less than e_lp of the pixel that attains tau_m.
    min(., lambda) moves by no more than its argument, so |theta_dev - theta_64| <= e_theta, and a pixel with
    |l_i - theta_64| > e_i + e_theta is on the same side of the cut-off in both."""
import math

import numpy as np
import torch

import _fp64_loss_ref as L
from _fp64_loss_ref import _bound, f32  # noqa: F401  (re-exported for the tests)

NVALS = 8
D_BINS = (2048, 1024, 1024)                       # the digit histograms of the radix select: 11 + 10 + 10 bits
STATE_WORDS = 16


def ws_bytes(npix):
    """mirror of kd_seg_ohem_ws_bytes: the slab (8 doubles per block), the histograms and the state (32-bit words), one key per pixel"""
    return L.seg_layout(npix)[0] * 8 * 8 + (sum(D_BINS) + STATE_WORDS) * 4 + npix * 4


def lam_of(thresh):
    """lambda = fl32(-log(thresh)) as the host forms it, +0 for thresh = 1"""
    return float(np.float32(-math.log(thresh))) + 0.0


def count_to_keep(n, min_kept, min_divisor):
    return min(n, max(min_kept, -(-n // min_divisor)))


def _bits(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    return a.view(np.uint32) & np.uint32(0x7FFFFFFF)


def select(nll_f32, n_valid_mask, lam, min_kept, min_divisor):
    """nll_f32: fp32 values [npix] (anything outside the mask), n_valid_mask: bool [npix], lam: the fp32 cut-off (>= 0).
    -> (m, tau_m, theta, keep): the count to keep, the m-th largest l over the mask and theta = min(tau_m, lam) as numpy.float32
    (compare their BITS), keep bool [npix].  No valid pixel: m = 0, tau_m = None, theta = lam, nothing kept."""
    bits = _bits(nll_f32)
    mask = (n_valid_mask.detach().cpu().numpy() if torch.is_tensor(n_valid_mask) else np.asarray(n_valid_mask)).reshape(-1).astype(bool)
    lam_bits = np.array([lam], dtype=np.float32).view(np.uint32)[0]
    valid = bits[mask]
    n = int(valid.size)
    m = count_to_keep(n, min_kept, min_divisor)
    if n == 0:
        return 0, None, np.float32(lam), np.zeros_like(mask)
    tau_bits = np.partition(valid, n - m)[n - m]
    theta_bits = min(tau_bits, lam_bits)
    as_f32 = lambda b: np.array([b], dtype=np.uint32).view(np.float32)[0]
    return m, as_f32(tau_bits), as_f32(theta_bits), mask & (bits >= theta_bits)


def per_pixel(zs, y, ign):
    """zs [B, NC, HW], y int64 [B, HW] -> (valid [B, HW], l [B, HW] (0 outside K), e_l [B, HW]) in zs' dtype"""
    B, NC, HW = zs.shape
    valid = (y != ign) & (y >= 0) & (y < NC)
    ys = torch.where(valid, y, torch.zeros_like(y)).reshape(B, 1, HW)
    _, lp, e_lp, _ = L._softmax(zs, 1.0)
    l = -lp.gather(1, ys).reshape(B, HW)
    return valid, torch.where(valid, l, torch.zeros_like(l)), e_lp.reshape(B, HW)


def select64(l, e_l, valid, lam, min_kept, min_divisor):
    """the selection on float64 values -> dict: m, tau, theta, keep [npix], e_theta, margin [npix] (valid pixels within
    e_l + e_theta of theta: the only ones fp32 and float64 may put on different sides), share = |margin| / n"""
    l, e_l, valid = l.reshape(-1), e_l.reshape(-1), valid.reshape(-1)
    lv, ev = l[valid], e_l[valid]
    n = int(lv.numel())
    m = count_to_keep(n, min_kept, min_divisor)
    if n == 0:
        z = torch.zeros_like(valid)
        return {"m": 0, "tau": None, "theta": lam, "keep": z, "e_theta": 0.0, "margin": z, "share": 0.0}
    kth = lambda v: torch.sort(v, descending=True)[0][m - 1].item()
    srt, idx = torch.sort(lv, descending=True)
    tau = srt[m - 1].item()
    e_theta = max(kth(lv + ev) - tau, tau - kth(lv - ev), ev[idx[m - 1]].item())
    theta = min(tau, lam)
    keep = valid & (l >= theta)
    margin = valid & ((l - theta).abs() <= e_l + e_theta)
    return {"m": m, "tau": tau, "theta": theta, "keep": keep, "e_theta": e_theta, "margin": margin, "share": int(margin.sum()) / n}


def ohem(zs, zt, y, cw, ign, T, alpha, gs, keep, n_seq, want_grad=True):
    """value and gradient over the kept set `keep` [B, HW] (a subset of K) -> dict of (value, bound):
    "vals" [4] = (L, KL, sum_S w, the weighted CE over all of K) and "dzs"."""
    y_s = torch.where(keep.reshape(y.shape), y, torch.full_like(y, ign))
    r = L.seg_loss(zs, zt, y_s, cw, ign, T, alpha, gs, n_seq, want_grad=want_grad)
    a = L.seg_loss(zs, None, y, cw, ign, T, alpha, gs, n_seq, want_grad=False)
    v, e = r["losses"]
    out = {"vals": (torch.cat([v, a["losses"][0][:1]]), torch.cat([e, a["losses"][1][:1]]))}
    if want_grad:
        out["dzs"] = r["dzs"]
    return out


# ---- inputs and cases shared by tests/test_ohem_ref_host.py and tests/test_gpu_ohem_loss.py -------------------------------------

SHAPES = {"few": (2, 3), "partial_block": (3, 61), "ragged": (17, 16384)}       # 17 * 16384 = 278 528 > 1024 * 256: a ragged second iteration
# (thresh, min_divisor, min_kept)
PARAMS = {
    "m1": (1e-30, 2 ** 40, 1),           # m = 1, lambda = 69 above every l: the hardest pixel (and its ties) alone
    "all_div": (0.7, 1, 1),              # min_divisor = 1: m = n, everything valid is kept
    "kept_cap": (1e-30, 16, 10 ** 9),    # min_kept > n: m is capped at n
    "thresh1": (1.0, 16, 1),             # lambda = 0: everything valid is kept
    "rank": (1e-30, 16, 1),              # lambda above every l: the rank decides
    "third": (1e-30, 3, 1),              # the same with a third of the pixels
    "mid": (0.7, 16, 1),                 # the defaults: far more than n / 16 pixels lie above the threshold, which decides
}
KEEP_ALL = ("all_div", "kept_cap", "thresh1")


def ohem_inputs(B, NC, HW, seed, device, scene, ign=-1, teacher=True, weights=True):
    """scene: "continuous" (random logits of scale 3, every label valid), "dropped" (the same with about 3 % each of NC, -7 and
    ignore_index among the labels), "narrow" (logits of scale 1e-6 around a constant: every l shares its high bits), "ties" (five
    distinct logit vectors: at most 5 * NC distinct l), "identical" (one vector, one label), "ignored" (every label ignore_index)"""
    g = torch.Generator(device=device).manual_seed(seed + 7919)          # a stream of its own beside seg_inputs'
    zs, zt, y, cw = L.seg_inputs(B, NC, HW, seed, device, ign, 3.0, weights, teacher)
    if scene != "dropped":
        y = torch.randint(0, NC, (B, HW), generator=g, device=device)
    if scene == "narrow":
        zs = 0.5 + 1e-6 * torch.randn(B, NC, HW, generator=g, device=device)
    elif scene == "ties":
        vecs = torch.randn(5, NC, generator=g, device=device) * 2
        pick = torch.randint(0, 5, (B, HW), generator=g, device=device)
        zs = vecs[pick].permute(0, 2, 1).contiguous()
    elif scene == "identical":
        zs = (torch.randn(1, NC, 1, generator=g, device=device) * 2).expand(B, NC, HW).contiguous()
        y = torch.full_like(y, NC - 1)
    elif scene == "ignored":
        y = torch.full_like(y, ign)
    return zs, zt, y, cw


# (shape, NC, scene, teacher, class weights, parameters): every NC of both ends of each class bucket, every shape, every scene,
# every parameter corner; the cross-product is thinned.  A (2, 3) case of the set-agreement scenes uses parameters under which the
# threshold decides: where the rank decides, the pixel that attains tau_m lies inside the margin by construction, one of six.
CASES = [
    ("few", 2, "continuous", True, True, "mid"),
    ("few", 5, "dropped", False, True, "mid"),
    ("few", 3, "identical", False, False, "rank"),
    ("partial_block", 3, "continuous", True, False, "rank"),
    ("partial_block", 4, "dropped", False, True, "mid"),
    ("partial_block", 9, "continuous", False, False, "m1"),
    ("partial_block", 8, "ties", True, True, "rank"),
    ("partial_block", 16, "narrow", False, True, "third"),
    ("partial_block", 2, "ignored", True, True, "mid"),
    ("partial_block", 5, "continuous", False, True, "kept_cap"),
    ("partial_block", 9, "continuous", True, True, "thresh1"),
    ("partial_block", 4, "continuous", False, False, "all_div"),
    ("ragged", 2, "continuous", True, True, "mid"),
    ("ragged", 16, "dropped", True, True, "rank"),
    ("ragged", 8, "narrow", False, False, "rank"),
    ("ragged", 5, "ties", False, True, "rank"),
    ("ragged", 9, "continuous", False, True, "rank"),
    ("ragged", 3, "identical", True, False, "mid"),
    ("ragged", 4, "ignored", False, False, "rank"),
]
SET_SCENES = ("continuous", "dropped")            # the scenes of the set-agreement check
MARGIN_CAP = 0.02                                 # the cap tests/test_gpu_multiclass_step.py puts on its exempt share


def case_id(case):
    shape, NC, scene, teacher, weights, par = case
    return f"{shape}-nc{NC}-{scene}-{'kl' if teacher else 'ce'}-{'w' if weights else 'u'}-{par}"


# The input seed of a case.  The seeds of the SET_SCENES cases were picked on the CPU from the float64 reference alone
# (tests/test_ohem_ref_host.py asserts the condition): with 100 + the case's index every such case has at most 2 % of its valid
# pixels inside the margin.
def case_seed(case):
    return 100 + CASES.index(case)


def case_setup(case, device):
    """-> (zs, zt, y, cw), dict of the call's scalars"""
    shape, NC, scene, teacher, weights, par = case
    B, HW = SHAPES[shape]
    i = CASES.index(case)
    ign = (-1, 255)[i % 2]
    tensors = ohem_inputs(B, NC, HW, case_seed(case), device, scene, ign, teacher, weights)
    thresh, min_divisor, min_kept = PARAMS[par]
    gscale, gdev = ((1.0, None), (2.5, 0.5))[(i // 2) % 2]
    a = {"B": B, "HW": HW, "npix": B * HW, "ign": ign, "T": 4.0, "alpha": f32(0.7) if teacher else 0.0, "gscale": gscale, "gdev": gdev,
         "gs": f32(gscale) * (1.0 if gdev is None else f32(gdev)), "lam": lam_of(thresh), "min_kept": min_kept, "min_divisor": min_divisor,
         "n_seq": L.seg_n_seq(B * HW)}
    return tensors, a
