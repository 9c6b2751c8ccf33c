"""Loss / metric Functions of the KD step (device-side values, no host sync).

  seg_loss      : weighted CE with ignore_index (trainer.py:55,88), optionally + alpha*T^2*KL to a
                  teacher's logits -- value and dL/dlogits produced by one fused HIP call; 2 to 16 classes (the opt-in
                  RegionLoss / LovaszLoss terms below: 2 to 4)
  region_seg_loss : the opt-in hard-label loss wf*Focal + wt*Tversky (RegionLoss) in place of the weighted CE, same fused
                  form (csrc/kd_loss_region.hip; definition in DESIGN.md section 3)
  lovasz_seg_loss : the opt-in Lovasz-Softmax term (LovaszLoss) added to the weighted CE or to a RegionLoss: the base call, then
                  csrc/kd_loss_lovasz.hip on the same stream, adding its value and its gradient to what the base call wrote
  ohem_seg_loss : the opt-in online-hard-example-mining cross-entropy (OhemCE) in place of the weighted CE, 2 to 16 classes: an exact
                  order-statistic selection on the device, then the CE over the kept pixels (csrc/kd_loss_ohem.hip)
  hard_seg_loss : whichever of the four above the type of its `spec` names (None: seg_loss); what Trainer trains with
  feature_mse   : F.mse_loss forward + gradient
  channel_kd    : the opt-in channel-wise distillation feature term (ChannelKD; Shu et al., ICCV 2021) in the feature MSE's place:
                  a temperature softmax down the H*W positions of every channel of every image, KL to the teacher's
                  (csrc/kd_loss_cwd.hip; definition in DESIGN.md section 3)
  pair_kd       : the opt-in pair-wise distillation feature term (PairKD; Liu et al., CVPR 2019) in the feature MSE's place: the cosine
                  similarities of all pairs of positions of a map against the teacher's, formed from C x C Gram matrices, never the
                  n x n affinities (csrc/kd_loss_pair.hip; definition in DESIGN.md section 3)
  intra_class_kd : the opt-in intra-class feature variation distillation feature term (IntraClassKD; Wang et al., ECCV 2020) in the
                  feature MSE's place: the cosine similarity of every labelled pixel to the prototype of its own class against the
                  teacher's (csrc/kd_loss_ifv.hip; definition in DESIGN.md section 3)
  kd_objective  : CE + alpha*T^2*KL + beta*(MSE(cam) + MSE(lidar))   (the
                  reference has no KD code -- this definition is the build's specification)
  kd_objective_backward : the same objective AND its backward pass for the training step: every loss kernel
                  produces its value and its gradient in one pass (the root's upstream gradient is 1), the
                  feature-MSE gradients ride into the fusion block's data-gradient GEMMs as addends
  confusion     : argmax + confusion matrix of SegmentationMetrics.update (trainer.py:18-26)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, Dict, Optional, Tuple

import torch

import numpy as np

from . import gradsink, ops
from .lib import KDError, lib
from .ops import P, stream


def _check_target(logits, target):
    """The loss kernels index the target as [B, H, W] of the logits: anything else would read past its end."""
    B, _, H, W = logits.shape
    if tuple(target.shape) != (B, H, W) or target.device != logits.device:
        raise KDError(f"segmentation target {tuple(target.shape)} on {target.device} does not match the logits' "
                      f"[B, H, W] = {(B, H, W)} on {logits.device}")


def _check_class_weights(logits, class_w):
    """The loss kernels read class_w[y] for every label 0 <= y < NC without a bounds check of their own."""
    if class_w is None:
        return
    NC = logits.shape[1]
    if (not torch.is_tensor(class_w) or class_w.dtype != torch.float32 or class_w.device != logits.device
            or class_w.dim() != 1 or class_w.numel() != NC or not class_w.is_contiguous()):
        what = (f"{tuple(class_w.shape)} {class_w.dtype} on {class_w.device}" if torch.is_tensor(class_w)
                else type(class_w).__name__)
        raise KDError(f"class weights must be a contiguous float32 tensor of {NC} entries (the logits' class count) on "
                      f"{logits.device}, got {what}")


def _ce_call(spec, zs, zt, target, class_w, ignore_index, T, alpha, gdev, losses, dzs):
    """the default hard-label term (spec None): the weighted CE, losses[0] = CE, [1] = KL, [2] = the sum of the kept weights"""
    B, NC, H, W = zs.shape
    nbytes = lib.kd_seg_loss_ws_bytes(B * H * W)
    ws = ops.workspace(nbytes, zs.device)
    lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(target), P(class_w), int(ignore_index), float(T), float(alpha),
             1.0, P(gdev), P(losses), P(dzs), B, NC, H * W, P(ws), nbytes, stream())


def _expect_spec(fn, spec, cls):
    if not isinstance(spec, cls):
        raise KDError(f"{fn}: spec must be a kdrt.losses.{cls.__name__}, got {type(spec).__name__}")


def seg_loss(logits, target, class_weights: Optional[torch.Tensor] = None, ignore_index: int = -1,
             teacher_logits: Optional[torch.Tensor] = None, T: float = 4.0, alpha: float = 1.0):
    """-> (ce, kl).  The gradient that flows back through `ce` is that of ce + alpha*T^2*kl
    (kl is returned for logging / for adding its VALUE to the total)."""
    return hard_seg_loss(logits, target, None, class_weights, ignore_index, teacher_logits, T, alpha)[:2]


@dataclass(frozen=True)
class RegionLoss:
    """Parameters of the region-based hard-label loss  L_hard = wf * Focal + wt * Tversky  (DESIGN.md section 3):

      Focal   = sum_K w[y] (1 - p_y)^gamma (-log p_y) / sum_K w[y]      K: the pixels the weighted CE keeps, p = softmax(logits)
      Tversky = 1 - (1/NC) sum_c (TP_c + s) / (TP_c + a*FP_c + b*FN_c + s)   soft counts over K, all NC classes, no class weights

    gamma = 0 makes Focal the weighted CE; a = b = 0.5 makes Tversky the Dice loss.  A term whose weight is 0 is not evaluated.
    With wf > 0 a batch without a kept pixel gives NaN, as the CE does (0/0); with wf == 0 it gives the Tversky value and a zero
    gradient.  The Tversky sums run over the batch of ONE call: under data parallelism each rank forms them over its own shard
    (like the BatchNorm statistics) and the reducer averages the per-rank gradients, so the optimised loss is the mean of the
    per-rank losses, which is not the Tversky loss of the global batch."""
    gamma: float = 2.0
    wf: float = 1.0
    wt: float = 1.0
    a: float = 0.7
    b: float = 0.3
    s: float = 1.0

    def __post_init__(self):
        for k in ("gamma", "wf", "wt", "a", "b", "s"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"RegionLoss: {k} must be a finite number, got {v!r}")
        if not (self.gamma == 0 or self.gamma >= 1):
            raise ValueError(f"RegionLoss: gamma must be 0 or >= 1 (the focal derivative is unbounded at p_y -> 1 in between), got {self.gamma}")
        if self.a < 0 or self.b < 0 or self.s <= 0:
            raise ValueError(f"RegionLoss: need a >= 0, b >= 0 and s > 0, got a={self.a} b={self.b} s={self.s}")
        if self.wf < 0 or self.wt < 0 or (self.wf == 0 and self.wt == 0):
            raise ValueError(f"RegionLoss: need wf >= 0 and wt >= 0, not both 0, got wf={self.wf} wt={self.wt}")

    def args(self):
        return tuple(float(getattr(self, k)) for k in ("gamma", "wf", "wt", "a", "b", "s"))


REGION_VALS = 17          # floats kd_seg_region_loss_fwd_bwd writes: L_hard, KL, sum w, Focal, Tversky, TI_c[4], gradient coefficients[8]
HARD_MAX_NC = 4           # RegionLoss and LovaszLoss: per-class slots of REGION_VALS / LOVASZ_VALS and of their kernels


def _region_call(spec, zs, zt, target, class_w, ignore_index, T, alpha, gdev, vals, dzs):
    B, NC, H, W = zs.shape
    nbytes = lib.kd_seg_region_loss_ws_bytes(B * H * W)
    ws = ops.workspace(nbytes, zs.device)
    lib.call("kd_seg_region_loss_fwd_bwd", P(zs), P(zt), P(target), P(class_w), int(ignore_index), float(T), float(alpha),
             1.0, P(gdev), *spec.args(), P(vals), P(dzs), B, NC, H * W, P(ws), nbytes, stream())


def region_seg_loss(logits, target, spec: RegionLoss, class_weights: Optional[torch.Tensor] = None, ignore_index: int = -1,
                    teacher_logits: Optional[torch.Tensor] = None, T: float = 4.0, alpha: float = 1.0):
    """-> (hard, kl, parts): seg_loss with hard = spec.wf * Focal + spec.wt * Tversky in place of the weighted CE (see RegionLoss;
    class weights enter the focal term only).  The gradient that flows back through `hard` is that of hard + alpha*T^2*kl.
    parts = {"focal", "tversky", "class_ti"}: device scalars and the [NC] vector of per-class Tversky indices (detached; a term
    whose weight is 0 reads 0)."""
    _expect_spec("region_seg_loss", spec, RegionLoss)
    return hard_seg_loss(logits, target, spec, class_weights, ignore_index, teacher_logits, T, alpha)


@dataclass(frozen=True)
class LovaszLoss:
    """The Lovasz-Softmax hard-label term (Berman et al., CVPR 2018) on top of a base term:

      L_hard = base + weight * Lovasz,    base: None (the weighted CE) or a RegionLoss
      Lovasz = (1/B) sum_b (1/|P_b|) sum_{c in P_b} L_{b,c}      classes = "present", per image

    L_{b,c} sorts the kept pixels of image b by the class's error (p_c off the class, the sum of the other probabilities on it)
    descending -- equal fp32 errors in ascending pixel order, so the gradient is a function of the input -- and weighs them with
    the increments of the Jaccard loss along that order.  P_b: the classes with a kept pixel in image b; an image without one
    adds 0 and still counts in B.  Class weights do not enter.  One workgroup sorts an image's keys in LDS: H * W <= 16384
    (128 x 128), KDError above.
    The term is a mean over images: with equal shards under data parallelism the mean of the per-rank losses IS the loss of the
    global batch and the reducer's averaged gradient its gradient (the batch-wide Tversky sums of RegionLoss lack this)."""
    weight: float = 1.0
    base: Optional[RegionLoss] = None

    def __post_init__(self):
        w = self.weight
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w <= 0:
            raise ValueError(f"LovaszLoss: weight must be a finite number > 0, got {w!r}")
        if self.base is not None and not isinstance(self.base, RegionLoss):
            raise ValueError(f"LovaszLoss: base must be a RegionLoss or None (the weighted CE), got {type(self.base).__name__}")


LOVASZ_VALS = 5           # floats kd_seg_lovasz_fwd_bwd writes: L, then per class the mean of L_{b,c} over the images where it is present
LOVASZ_MAX_HW = 16384     # 8-byte keys of one image in the LDS of one CU


def _lovasz_call(spec, zs, target, ignore_index, gdev, vals, hard, dzs):
    """the Lovasz call that follows the base call on the same stream: hard[0] += weight * L, dzs += weight * gdev[0] * dL/dzs"""
    B, NC, H, W = zs.shape
    if H * W > LOVASZ_MAX_HW:
        raise KDError(f"LovaszLoss: a {H} x {W} map has {H * W} pixels per image, the per-image sort holds at most {LOVASZ_MAX_HW} (128 x 128)")
    nbytes = lib.kd_seg_lovasz_ws_bytes(B, NC, H * W)
    ws = ops.workspace(nbytes, zs.device)
    lib.call("kd_seg_lovasz_fwd_bwd", P(zs), P(target), int(ignore_index), float(spec.weight), 1.0, P(gdev), P(vals), P(hard), P(dzs),
             1, None, B, NC, H * W, P(ws), nbytes, stream())


def _hard_call(spec, zs, zt, target, class_w, ignore_index, T, alpha, gdev, hard, lov, dzs):
    """base call (weighted CE or region loss) into hard / dzs, then the Lovasz call adding to both.  hard: REGION_VALS floats
    ([0] the hard-label term, [1] KL in either layout), lov: LOVASZ_VALS floats."""
    base = _ce_call if spec.base is None else _region_call
    base(spec.base, zs, zt, target, class_w, ignore_index, T, alpha, gdev, hard, dzs)
    _lovasz_call(spec, zs, target, ignore_index, gdev, lov, hard, dzs)     # looked up here, at call time: tests replace it


def lovasz_seg_loss(logits, target, spec: LovaszLoss, class_weights: Optional[torch.Tensor] = None, ignore_index: int = -1,
                    teacher_logits: Optional[torch.Tensor] = None, T: float = 4.0, alpha: float = 1.0):
    """-> (hard, kl, parts): seg_loss / region_seg_loss with hard = base + spec.weight * Lovasz (see LovaszLoss; the class weights
    enter the base term only).  The gradient that flows back through `hard` is that of hard + alpha*T^2*kl.
    parts = {"lovasz", "class_lovasz"}: the unweighted Lovasz value and the [NC] vector of per-class means of L_{b,c} over the
    images where the class is present (0 if never), detached; with a RegionLoss base also its "focal" and "tversky".
    Data parallel: the Lovasz term is a mean over images, so with equal shards the mean of the per-rank values is the global one."""
    _expect_spec("lovasz_seg_loss", spec, LovaszLoss)
    return hard_seg_loss(logits, target, spec, class_weights, ignore_index, teacher_logits, T, alpha)


@dataclass(frozen=True)
class OhemCE:
    """Online hard example mining for the weighted cross-entropy, 2 to 16 classes:

      l_i = -log p_{y_i} over the n pixels K the weighted CE keeps,   m = min(n, max(min_kept, ceil(n / min_divisor)))
      theta = min(m-th largest l, -log(thresh)),   S = { i in K : l_i >= theta },   L_hard = sum_S w[y] l / sum_S w[y]

    Every pixel whose probability of its label is at most `thresh` is kept when there are at least m of them; otherwise the m
    hardest, with every tie at the m-th.  S is held constant in the gradient.  thresh = 1 or min_divisor = 1 keeps all of K: the
    weighted CE.  min_divisor = 16 is BiSeNet's n/16.  Mining is a training device: Trainer validates with the plain weighted CE.
    Mining is per call: under data parallelism each rank mines its own shard (as the Tversky sums of RegionLoss cover one shard)
    and the reducer averages the per-rank gradients; there is no collective."""
    thresh: float = 0.7
    min_divisor: int = 16
    min_kept: int = 1

    def __post_init__(self):
        t = self.thresh
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or not 0 < t <= 1:
            raise ValueError(f"OhemCE: thresh must be a finite number in (0, 1], got {t!r}")
        for k in ("min_divisor", "min_kept"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"OhemCE: {k} must be an integer >= 1, got {v!r}")

    def lam(self):
        """lambda = fl32(-log(thresh)), the cut-off on l the kernel receives (+0 for thresh = 1)"""
        return float(np.float32(-math.log(self.thresh))) + 0.0


OHEM_VALS = 8             # floats kd_seg_ohem_fwd_bwd writes: L, KL, sum_S w, the CE over all of K, theta, |S| / n, 2 spare
_I64_MAX = 2 ** 63 - 1


def _ohem_call(spec, zs, zt, target, class_w, ignore_index, T, alpha, gdev, vals, dzs):
    B, NC, H, W = zs.shape
    nbytes = lib.kd_seg_ohem_ws_bytes(B * H * W)
    ws = ops.workspace(nbytes, zs.device)
    lib.call("kd_seg_ohem_fwd_bwd", P(zs), P(zt), P(target), P(class_w), int(ignore_index), float(T), float(alpha), 1.0, P(gdev),
             spec.lam(), min(spec.min_kept, _I64_MAX), min(spec.min_divisor, _I64_MAX), P(vals), None, P(dzs), None, None,
             B, NC, H * W, P(ws), nbytes, stream())


def ohem_seg_loss(logits, target, spec: OhemCE, class_weights: Optional[torch.Tensor] = None, ignore_index: int = -1,
                  teacher_logits: Optional[torch.Tensor] = None, T: float = 4.0, alpha: float = 1.0):
    """-> (hard, kl, parts): seg_loss with the weighted CE averaged over the mined pixels only (see OhemCE), 2 to 16 classes.  The
    gradient that flows back through `hard` is that of hard + alpha*T^2*kl, the kept set held constant.
    parts = {"ce_all", "theta", "kept"}: the weighted CE over every kept-label pixel (for logging), the cut-off on -log p_y and the
    kept share |S| / n, device scalars, detached.  Data parallel: each rank mines its own shard."""
    _expect_spec("ohem_seg_loss", spec, OhemCE)
    hard, kl, parts = hard_seg_loss(logits, target, spec, class_weights, ignore_index, teacher_logits, T, alpha)
    return hard, kl, {k.removeprefix("ohem_"): v for k, v in parts.items()}      # the objective's "ohem_theta", "ohem_kept"


# ---------------------------------------------------------------------------------------------
# The hard-label terms, one row each.  The rows are all that seg_loss .. ohem_seg_loss, kd_objective and kd_objective_backward know of
# a term; a new term supplies a spec class, its call and a row.
_FUNCTION, _AUTOGRAD, _FUSED = _FORMS = ("function", "autograd", "fused")    # a term's own *_seg_loss function, kd_objective, kd_objective_backward


@dataclass(frozen=True)
class _Part:
    """where a named part lives in the value buffers of its term"""
    at: int
    buf: int = 0
    per_class: bool = False                       # the [NC] vector that starts at `at`, not the scalar there
    forms: Tuple[str, ...] = _FORMS               # the forms that report it


@dataclass(frozen=True, eq=False)
class _HardTerm:
    """one hard-label term: its launches, its value buffers, its class limit and where its named parts lie"""
    fn: str                                       # the term's public function, for messages
    call: Callable                                # (spec, zs, zt, target, class_w, ignore_index, T, alpha, gdev, *bufs, dzs): the launches
    sizes: Tuple[int, ...]                        # floats per value buffer; bufs[0][0] is the term's value, bufs[0][1] the KL
    zeroed: bool = False                          # whether bufs[0] must start zeroed
    max_nc: Optional[int] = None                  # class limit, checked before the first launch; None: the kernel's own 2..16
    parts: Dict[str, _Part] = field(default_factory=dict)
    absent: Callable = lambda spec: ()            # the parts that this spec does not report

    def check_classes(self, spec, NC):
        if self.max_nc is not None and NC > self.max_nc:
            raise KDError(f"{type(spec).__name__}: at most {self.max_nc} classes, got {NC}; 5 to 16 classes train with the weighted CE "
                          "(hard_loss=None) or an OhemCE")

    def alloc(self, dev, scratch=False):
        """the value buffers; scratch: for a call whose values nobody reads (the autograd backward), never zeroed"""
        first = torch.zeros if self.zeroed and not scratch else torch.empty
        return tuple((torch.empty if i else first)(n, device=dev, dtype=torch.float32) for i, n in enumerate(self.sizes))

    def names(self, spec, form):
        skip = self.absent(spec)
        return [k for k, p in self.parts.items() if form in p.forms and k not in skip]

    def read(self, spec, form, bufs, NC):
        """-> {name: view of its buffer} of the parts that `form` reports"""
        at = ((k, self.parts[k]) for k in self.names(spec, form))
        return {k: bufs[p.buf][p.at:p.at + NC] if p.per_class else bufs[p.buf][p.at] for k, p in at}


_HARD_TERMS = {
    type(None): _HardTerm("seg_loss", _ce_call, (4,)),
    RegionLoss: _HardTerm("region_seg_loss", _region_call, (REGION_VALS,), max_nc=HARD_MAX_NC, parts={
        "focal": _Part(3), "tversky": _Part(4), "class_ti": _Part(5, per_class=True, forms=(_FUNCTION,))}),
    LovaszLoss: _HardTerm("lovasz_seg_loss", _hard_call, (REGION_VALS, LOVASZ_VALS), zeroed=True, max_nc=HARD_MAX_NC, parts={
        "lovasz": _Part(0, buf=1), "class_lovasz": _Part(1, buf=1, per_class=True, forms=(_FUNCTION, _AUTOGRAD)),
        "focal": _Part(3), "tversky": _Part(4)}, absent=lambda spec: ("focal", "tversky") if spec.base is None else ()),
    OhemCE: _HardTerm("ohem_seg_loss", _ohem_call, (OHEM_VALS,), parts={
        "ce_all": _Part(3), "ohem_theta": _Part(4), "ohem_kept": _Part(5)}),
}
HARD_LOSSES = tuple(c for c in _HARD_TERMS if c is not type(None))


def _term(table, what, spec, error=ValueError):
    """the row of `spec` in a table of terms; `error` naming every accepted class when it has none (the constructors that take the
    option raise ValueError, the objective KDError, as they always have)"""
    for cls, term in table.items():
        if isinstance(spec, cls):
            return term
    accepted = ", ".join(f"a kdrt.losses.{c.__name__}" for c in table if c is not type(None))
    raise error(f"{what} must be {accepted} or None, got {type(spec).__name__}")


def check_hard_loss(spec):
    """ValueError unless spec is None (the weighted CE) or one of HARD_LOSSES"""
    _term(_HARD_TERMS, "hard_loss", spec)


def check_hard_classes(spec, num_classes):
    """KDError when the hard-label term of `spec` does not hold `num_classes` classes (RegionLoss and LovaszLoss: at most 4)"""
    _term(_HARD_TERMS, "hard_loss", spec).check_classes(spec, num_classes)


class _HardLossFn(torch.autograd.Function):
    """The hard-label term of one row (+ alpha*T^2*KL to a teacher's logits).  forward: the loss values only; backward: the row's call
    once more, which now writes dL/dlogits scaled by the upstream gradient read from device memory (no host sync, no extra
    elementwise pass)."""

    @staticmethod
    def forward(ctx, term, spec, zs, zt, target, class_w, ignore_index, T, alpha):
        ops.require_gpu_tensor(zs, term.fn)
        zs_c = zs.detach().contiguous()
        zt_c = None if zt is None else zt.detach().contiguous()
        target = target.contiguous()
        if target.dtype != torch.int64:
            raise KDError("segmentation target must be int64")
        _check_target(zs_c, target)
        _check_class_weights(zs_c, class_w)
        term.check_classes(spec, zs_c.shape[1])
        bufs = term.alloc(zs.device)
        term.call(spec, zs_c, zt_c, target, class_w, ignore_index, T, alpha, None, *bufs, None)
        ctx.args = (term, spec, zs_c, zt_c, target, class_w, ignore_index, T, alpha)
        kl = bufs[0][1]
        parts = term.read(spec, _FUNCTION, bufs, zs_c.shape[1]).values()
        ctx.mark_non_differentiable(kl, *parts)
        return (bufs[0][0], kl, *parts)

    @staticmethod
    def backward(ctx, g_hard, *_):
        # the gradient through `hard` is d(L_hard + alpha*T^2*KL)/dzs (kd_objective adds KL's value separately)
        term, spec, zs_c, zt_c, target, class_w, ignore_index, T, alpha = ctx.args
        bufs = term.alloc(zs_c.device, scratch=True)
        dzs = torch.empty_like(zs_c)
        term.call(spec, zs_c, zt_c, target, class_w, ignore_index, T, alpha, g_hard.contiguous().view(1), *bufs, dzs)
        return (None, None, dzs) + (None,) * 6


def _hard_seg_loss(term, form, logits, target, spec, class_weights, ignore_index, teacher_logits, T, alpha):
    """-> (hard, kl, the parts that `form` reports) through the row `term` of `spec`"""
    if teacher_logits is None:
        alpha = 0.0
    hard, kl, *vals = _HardLossFn.apply(term, spec, logits, teacher_logits, target, class_weights, ignore_index, T, alpha)
    parts = dict(zip(term.names(spec, _FUNCTION), vals))
    return hard, kl, {k: parts[k] for k in term.names(spec, form)}


def hard_seg_loss(logits, target, spec=None, class_weights: Optional[torch.Tensor] = None, ignore_index: int = -1,
                  teacher_logits: Optional[torch.Tensor] = None, T: float = 4.0, alpha: float = 1.0):
    """-> (hard, kl, parts) for any hard-label spec (None: the weighted CE, no parts): what seg_loss, region_seg_loss, lovasz_seg_loss
    and ohem_seg_loss return (the OhemCE parts under their names in the objective), chosen by the type of `spec`; ValueError for any
    other.  The gradient that flows back through `hard` is that of hard + alpha*T^2*kl."""
    term = _term(_HARD_TERMS, "hard_loss", spec)
    return _hard_seg_loss(term, _FUNCTION, logits, target, spec, class_weights, ignore_index, teacher_logits, T, alpha)


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ops.require_gpu_tensor(a, "feature_mse")
        am, _ = ops.nhwc_view(a.detach())
        bm, _ = ops.nhwc_view(b.detach())
        n = am.numel()
        loss = torch.empty(1, device=a.device, dtype=torch.float32)
        nbytes = lib.kd_mse_ws_bytes(n)
        ws = ops.workspace(nbytes, a.device)
        lib.call("kd_mse_fwd_bwd", P(am), P(bm), n, 0.0, None, P(loss), None, P(ws), nbytes, stream())
        ctx.am, ctx.bm = am, bm
        ctx.geom = (a.shape[0], a.shape[2], a.shape[3])
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        am, bm = ctx.am, ctx.bm
        n = am.numel()
        da = torch.empty_like(am)
        nbytes = lib.kd_mse_ws_bytes(n)
        ws = ops.workspace(nbytes, am.device)
        lib.call("kd_mse_fwd_bwd", P(am), P(bm), n, 2.0 / n, P(g.contiguous().view(1)), None, P(da), P(ws), nbytes, stream())
        return ops.nchw_from_matrix(da, ctx.geom), None


def feature_mse(student_feat, teacher_feat):
    return _MSEFn.apply(student_feat, teacher_feat)


@dataclass(frozen=True)
class ChannelKD:
    """Channel-wise distillation (Shu et al., ICCV 2021) as the feature term of the KD objective, in the
    feature MSE's place:

      phi(X)[b,c,i] = exp(X[b,c,i]/tau) / sum_j exp(X[b,c,j]/tau)         i, j over the H*W positions of image b, channel c
      CWD(S, T)     = tau^2 / (B*C) * sum_{b,c} sum_i phi(T) (log phi(T) - log phi(S)),    dCWD/dS = tau / (B*C) * (phi(S) - phi(T))

    It matches WHERE a channel fires, not how strongly: no adapter, no parameter, same channel count on both sides (a multiple of
    4 up to 512).  beta keeps its meaning, but the term's magnitude is not the MSE's: re-tune beta when switching.
    The term is a mean over images: with equal shards under data parallelism the mean of the per-rank values IS the value of the
    global batch and the reducer's averaged gradient its gradient."""
    tau: float = 4.0

    def __post_init__(self):
        t = self.tau
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t <= 0:
            raise ValueError(f"ChannelKD: tau must be a finite number > 0, got {t!r}")


CWD_MAX_C = 512           # csrc/kd_loss_cwd.hip: a thread owns 4 channels, a workgroup of 256 threads at least 2 rows


@dataclass(frozen=True)
class PairKD:
    """Pair-wise distillation (Liu et al., "Structured Knowledge Distillation for Semantic Segmentation", CVPR 2019; DESIGN.md
    section 3) as the feature term of the KD objective, in the feature MSE's place.  S [B, n, Cs] and T [B, n, Ct] are the NHWC
    matrices of the student's and the teacher's map, n = H*W; for image b:

      r_i   = sqrt(sum_c x_ic^2)                 for the rows of S_b and of T_b
      xh_i  = x_i / r_i  if r_i > 1e-12, else 0  (such a row also receives no gradient: empty BEV cells are all-zero after ReLU)
      a_ij  = xh_i . xh_j                        the cosine similarity of positions i and j
      L_b   = 1/n^2 * sum_ij (a^S_ij - a^T_ij)^2 = 1/n^2 * (|Gss|_F^2 - 2 |Gts|_F^2 + |Gtt|_F^2)
              Gss = Sh^T Sh [Cs x Cs],  Gts = Th^T Sh [Ct x Cs],  Gtt = Th^T Th [Ct x Ct]
      PAIR  = 1/B * sum_b L_b
      dPAIR/dSh_b = 4/(B n^2) * (Sh_b Gss - Th_b Gts) =: gh,     dPAIR/dS_i = (gh_i - xh_i (xh_i . gh_i)) / r_i

    It matches WHICH positions look alike, not the features themselves: no adapter, no parameter, no pooling (the Gram form costs
    O(n C^2), so the full-resolution map is affordable), and the two widths need not be equal (multiples of 4 from 4 to 256).
    beta keeps its meaning, but the term's magnitude is not the MSE's: with the 1/n^2 mean the gradient entries at n = 4096 are of
    order 1e-7 before beta -- re-tune beta when switching.
    The term is a mean over images: with equal shards under data parallelism the mean of the per-rank values IS the value of the
    global batch and the reducer's averaged gradient its gradient.
    The Gram form subtracts quantities of order 1: once the student's map is within about 1 % of the teacher's, the relative error
    of the small gradient that is left grows (absolute in the scale of the cancelling terms)."""


PAIR_MIN_C, PAIR_MAX_C = 4, 256   # csrc/kd_loss_pair.hip: widths in multiples of 4


@dataclass(frozen=True)
class IntraClassKD:
    """Intra-class feature variation distillation (Wang et al., "Intra-class Feature Variation Distillation for Semantic
    Segmentation", ECCV 2020) as the feature term of the KD objective, in the feature MSE's place.  S [B, n, Cs]
    and T [B, n, Ct] are the NHWC matrices of the student's and the teacher's map, n = H*W, y [B, n] the label map at the maps'
    resolution and NC the number of classes (the logits' class count).  Pixel i of image b is kept when y != ignore_index and
    0 <= y < NC; K_b kept pixels, N_bc of class c.  For X in {S, T}, per image:

      r_i   = sqrt(sum_k x_ik^2),  xh_i = x_i / r_i  if r_i > 1e-12, else 0
      m_c   = 1/N_bc * sum_{i kept, y_i = c} x_i       the prototype of class c (classes with N_bc = 0 are absent)
      mh_c  = m_c / |m_c|  if |m_c| > 1e-12, else 0
      s_i   = xh_i . mh_{y_i}                           the cosine similarity of a kept pixel to its own class's prototype
      L_b   = 1/K_b * sum_{i kept} (sS_i - sT_i)^2      (0 if K_b = 0; the image still counts in B)
      IFV   = 1/B * sum_b L_b
      g_i   = 2 (sS_i - sT_i) / (B K_b),   D_c = sum_{i kept, y_i = c} g_i (xh_i - s_i mh_c) / |m_c|        (all from S)
      dIFV/dS_j = g_j (mh_c - s_j xh_j) / r_j + D_c / N_bc,  c = y_j, for kept j; 0 for a pixel that is not kept

    A kept all-zero row still receives D_c / N_bc: the prototype is linear in it.  The compared quantity is one scalar per pixel:
    no adapter, no parameter, and the two widths need not be equal (multiples of 4 from 4 to 256), 2 to 16 classes.  It is the one
    feature term that reads the labels: where most BEV cells are background, the label-blind terms spend their gradient there.
    beta keeps its meaning, but the term's magnitude is not the MSE's (a mean of squared cosine differences, at most 4) -- re-tune
    beta when switching.
    The term is a mean over images: with equal shards under data parallelism the mean of the per-rank values IS the value of the
    global batch and the reducer's averaged gradient its gradient."""


IFV_MIN_C, IFV_MAX_C = 4, 256     # csrc/kd_loss_ifv.hip: widths in multiples of 4
IFV_MIN_NC, IFV_MAX_NC = 2, 16


def _check_cwd_pair(a, b):
    """the kernel indexes both maps as [B*H*W, C] of the student's shape"""
    if a.dim() != 4 or tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise KDError(f"channel_kd: student map {tuple(a.shape)} on {a.device} and teacher map {tuple(b.shape)} on {b.device} must be "
                      "[B, C, H, W] of one shape on one device")
    C = a.shape[1]
    if C % 4 != 0 or C > CWD_MAX_C or C < 4:
        raise KDError(f"channel_kd: {C} channels unsupported (a multiple of 4 up to {CWD_MAX_C})")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise KDError(f"channel_kd: fp32 maps expected, got {a.dtype} and {b.dtype}")


# The three calls below share one signature, (spec, am, bm, geom, target, NC, ignore_index, gcoef, gdev, val, ds), on the NHWC matrices
# am [B*H*W, Cs] and bm [B*H*W, Ct] of a map pair: val[0] = the term, ds = gcoef * gdev[0] * (the term's gradient over its own gcoef).
def _cwd_call(spec, am, bm, geom, target, NC, ignore_index, gcoef, gdev, val, ds):
    """one kd_feat_cwd_fwd_bwd call: val[0] = CWD, ds = gcoef * gdev[0] * (phi(s) - phi(t))"""
    B, H, W = geom
    C = am.shape[1]
    nbytes = lib.kd_feat_cwd_ws_bytes(B, H * W, C)
    ws = ops.workspace(nbytes, am.device)
    lib.call("kd_feat_cwd_fwd_bwd", P(am), P(bm), B, H * W, C, float(spec.tau), float(gcoef), P(gdev), P(val), P(ds), None, P(ws), nbytes,
             stream())


def _cwd_gcoef(spec, geom, am):
    """tau / (B*C), the host's double rounded to fp32 by the call"""
    return spec.tau / (geom[0] * am.shape[1])


def channel_kd(student_feat, teacher_feat, tau: float = 4.0):
    """CWD(student_feat, teacher_feat; tau) of two [B, C, H, W] fp32 maps (see ChannelKD): a device scalar whose gradient flows to
    the student map only.  KDError on a shape or device mismatch and on a channel count that is no multiple of 4 or above 512."""
    return _FEATURE_TERMS[ChannelKD].value(ChannelKD(tau), student_feat, teacher_feat, None, None, None)


def _check_pair_pair(a, b):
    """the kernel indexes the maps as [B*H*W, Cs] and [B*H*W, Ct]: one B, H, W, either width"""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.dim() != 4 or b.dim() != 4:
        raise KDError("pair_kd: two [B, C, H, W] tensors expected")
    ops.require_gpu_tensor(a, "pair_kd")
    if a.device != b.device or a.shape[0] != b.shape[0] or tuple(a.shape[2:]) != tuple(b.shape[2:]):
        raise KDError(f"pair_kd: student map {tuple(a.shape)} on {a.device} and teacher map {tuple(b.shape)} on {b.device} must share "
                      "B, H, W and the device")
    for C in (a.shape[1], b.shape[1]):
        if C % 4 != 0 or C < PAIR_MIN_C or C > PAIR_MAX_C:
            raise KDError(f"pair_kd: {C} channels unsupported (a multiple of 4 from {PAIR_MIN_C} to {PAIR_MAX_C})")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise KDError(f"pair_kd: fp32 maps expected, got {a.dtype} and {b.dtype}")


def _pair_call(spec, am, bm, geom, target, NC, ignore_index, gcoef, gdev, val, ds):
    """one kd_feat_pair_fwd_bwd call: val[0] = PAIR, ds = gcoef * gdev[0] * (B n^2 / 4) * dPAIR/dS"""
    B, H, W = geom
    Cs, Ct = am.shape[1], bm.shape[1]
    nbytes = lib.kd_feat_pair_ws_bytes(B, H * W, Cs, Ct)
    ws = ops.workspace(nbytes, am.device)
    lib.call("kd_feat_pair_fwd_bwd", P(am), P(bm), B, H * W, Cs, Ct, float(gcoef), P(gdev), P(val), P(ds), None, P(ws), nbytes, stream())


def _pair_gcoef(spec, geom, am):
    """4 / (B n^2), the host's double rounded to fp32 by the call"""
    B, H, W = geom
    return 4.0 / (float(B) * float(H * W) * float(H * W))


def pair_kd(student_feat, teacher_feat):
    """PAIR(student_feat, teacher_feat) of two fp32 maps [B, Cs, H, W] and [B, Ct, H, W] (see PairKD): a device scalar whose gradient
    flows to the student map only.  KDError on CPU tensors, a dtype other than fp32, differing B, H, W or devices, and on a width that is
    no multiple of 4 or outside 4..256."""
    return _FEATURE_TERMS[PairKD].value(PairKD(), student_feat, teacher_feat, None, None, None)


def _check_ifv_args(a, b, target, num_classes):
    """the kernel indexes the maps as [B*H*W, Cs] and [B*H*W, Ct] and the labels as [B*H*W]: one B, H, W for all three"""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or not torch.is_tensor(target) or a.dim() != 4 or b.dim() != 4:
        raise KDError("intra_class_kd: two [B, C, H, W] tensors and a [B, H, W] label map expected")
    ops.require_gpu_tensor(a, "intra_class_kd")
    if a.device != b.device or a.shape[0] != b.shape[0] or tuple(a.shape[2:]) != tuple(b.shape[2:]):
        raise KDError(f"intra_class_kd: student map {tuple(a.shape)} on {a.device} and teacher map {tuple(b.shape)} on {b.device} must "
                      "share B, H, W and the device")
    B, _, H, W = a.shape
    if tuple(target.shape) != (B, H, W) or target.device != a.device:
        raise KDError(f"intra_class_kd: label map {tuple(target.shape)} on {target.device} does not match the feature maps' [B, H, W] = "
                      f"{(B, H, W)} on {a.device} (the term needs labels at the maps' resolution: output_mode=\"same\")")
    if target.dtype != torch.int64:
        raise KDError(f"intra_class_kd: the label map must be int64, got {target.dtype}")
    for C in (a.shape[1], b.shape[1]):
        if C % 4 != 0 or C < IFV_MIN_C or C > IFV_MAX_C:
            raise KDError(f"intra_class_kd: {C} channels unsupported (a multiple of 4 from {IFV_MIN_C} to {IFV_MAX_C})")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise KDError(f"intra_class_kd: fp32 maps expected, got {a.dtype} and {b.dtype}")
    if int(num_classes) != num_classes or not IFV_MIN_NC <= num_classes <= IFV_MAX_NC:
        raise KDError(f"intra_class_kd: {num_classes} classes unsupported ({IFV_MIN_NC} to {IFV_MAX_NC})")


def _ifv_call(spec, am, bm, geom, target, NC, ignore_index, gcoef, gdev, val, ds):
    """one kd_feat_ifv_fwd_bwd call under the labels [B, H, W]: val[0] = IFV, ds = gcoef * gdev[0] * (B / 2) * dIFV/dS"""
    B, H, W = geom
    Cs, Ct = am.shape[1], bm.shape[1]
    nbytes = lib.kd_feat_ifv_ws_bytes(B, H * W, Cs, Ct, NC)
    ws = ops.workspace(nbytes, am.device)
    lib.call("kd_feat_ifv_fwd_bwd", P(am), P(bm), P(target), int(ignore_index), B, H * W, Cs, Ct, NC, float(gcoef), P(gdev), P(val), P(ds),
             None, P(ws), nbytes, stream())


def _ifv_gcoef(spec, geom, am):
    """2 / B, the host's double rounded to fp32 by the call"""
    return 2.0 / float(geom[0])


def intra_class_kd(student_feat, teacher_feat, target, num_classes, ignore_index=-1):
    """IFV(student_feat, teacher_feat; target) of two fp32 maps [B, Cs, H, W] and [B, Ct, H, W] under the int64 label map [B, H, W] with
    `num_classes` classes (see IntraClassKD): a device scalar whose gradient flows to the student map only.  KDError, before any
    launch, on CPU tensors, a dtype other than fp32 / int64, differing B, H, W or devices (a label map of another size included), a
    width that is no multiple of 4 or outside 4..256, and a class count outside 2..16."""
    return _FEATURE_TERMS[IntraClassKD].value(IntraClassKD(), student_feat, teacher_feat, target, int(num_classes), int(ignore_index))


# ---------------------------------------------------------------------------------------------
# The feature terms, one row each: all that channel_kd .. intra_class_kd, kd_objective and kd_objective_backward know of a term.  A new
# term supplies a spec class, a check of a map pair, a call of the signature above, its host-side gradient coefficient and a row.
class _FeatureTerm:
    """one feature term: its check, its call, its gradient coefficient, its part names and how the fused form finishes"""

    def __init__(self, fn, parts, check=lambda a, b, target, NC: None, call=None, gcoef=None):
        self.fn = fn              # the term's public function, for messages
        self.parts = parts        # the names of the camera map's and the LiDAR map's value in the objective's parts
        self.check = check        # (a, b, target, NC): KDError for a map pair (or labels) the kernel cannot take; no launch
        self.call = call
        self.gcoef = gcoef        # (spec, geom, am) -> the coefficient of the term's gradient, a Python float

    def value(self, spec, a, b, target, NC, ignore_index):
        """the autograd form: a device scalar whose gradient flows to the student map `a`"""
        return _FeatureFn.apply(self, spec, a, b, target, NC, ignore_index)

    def fused_map(self, spec, am, bm, geom, target, NC, ignore_index, beta, out, i, da):
        """the fused form, map i: ONE call that writes the value to out[i] and the gradient beta * d term / d am to da"""
        gcoef = float(np.float32(self.gcoef(spec, geom, am)) * np.float32(beta))      # the product the autograd form's backward forms
        self.call(spec, am, bm, geom, target, NC, ignore_index, gcoef, None, out[i:i + 1], da)

    def fused_total(self, hard, out, maps, ckl, beta):
        """the fused form's last launch: out[2] = hard[0] + ckl * hard[1] + beta * (out[0] + out[1])"""
        lib.call("kd_kd_total", P(hard), P(out[0:1]), P(out[1:2]), ckl, beta, P(out[2:3]), stream())


class _MSETerm(_FeatureTerm):
    """The default, the feature MSE: the fused form leaves per-block sums per map and kd_kd_objective_final finishes the two values
    together with the total."""

    def value(self, spec, a, b, target, NC, ignore_index):
        return _MSEFn.apply(a, b)

    def fused_map(self, spec, am, bm, geom, target, NC, ignore_index, beta, out, i, da):
        n = am.numel()
        slab = torch.empty(lib.kd_mse_slab_blocks(n), device=am.device, dtype=torch.float32)
        gcoef = float(np.float32(2.0 / n) * np.float32(beta))      # the product autograd's fp32 chain rule forms
        lib.call("kd_mse_partial", P(am), P(bm), n, gcoef, P(da), P(slab), stream())
        return slab, n

    def fused_total(self, hard, out, maps, ckl, beta):
        (slab_c, n_c), (slab_l, n_l) = maps
        lib.call("kd_kd_objective_final", P(hard), P(slab_c), n_c, P(slab_l), n_l, ckl, beta, P(out), stream())


_FEATURE_TERMS = {
    type(None): _MSETerm("feature_mse", ("mse_cam", "mse_lidar")),
    ChannelKD: _FeatureTerm("channel_kd", ("cwd_cam", "cwd_lidar"), lambda a, b, target, NC: _check_cwd_pair(a, b), _cwd_call, _cwd_gcoef),
    PairKD: _FeatureTerm("pair_kd", ("pair_cam", "pair_lidar"), lambda a, b, target, NC: _check_pair_pair(a, b), _pair_call, _pair_gcoef),
    IntraClassKD: _FeatureTerm("intra_class_kd", ("ifv_cam", "ifv_lidar"), _check_ifv_args, _ifv_call, _ifv_gcoef),
}
FEATURE_LOSSES = tuple(c for c in _FEATURE_TERMS if c is not type(None))


def check_feature_loss(spec):
    """ValueError unless spec is None (the feature MSE) or one of FEATURE_LOSSES"""
    _term(_FEATURE_TERMS, "feature_loss", spec)


class _FeatureFn(torch.autograd.Function):
    """The feature term of one row, in _MSEFn's shape: forward the value only; backward one more call with the upstream gradient read
    from device memory, so the gradient coefficient is k = fl32(fl32(gcoef) * g) -- with g = fl32(beta) from the objective's autograd
    graph the product kd_objective_backward folds into gcoef on the host."""

    @staticmethod
    def forward(ctx, term, spec, a, b, target, NC, ignore_index):
        term.check(a, b, target, NC)
        ops.require_gpu_tensor(a, term.fn)
        am, geom = ops.nhwc_view(a.detach())
        bm, _ = ops.nhwc_view(b.detach())
        if target is not None:
            target = target.contiguous()
        val = torch.empty(1, device=a.device, dtype=torch.float32)
        term.call(spec, am, bm, geom, target, NC, ignore_index, 0.0, None, val, None)
        ctx.args = (term, spec, am, bm, geom, target, NC, ignore_index)
        return val[0]

    @staticmethod
    def backward(ctx, g):
        term, spec, am, bm, geom, target, NC, ignore_index = ctx.args
        ds = torch.empty_like(am)
        val = torch.empty(1, device=am.device, dtype=torch.float32)
        term.call(spec, am, bm, geom, target, NC, ignore_index, term.gcoef(spec, geom, am), g.contiguous().view(1), val, ds)
        return None, None, ops.nchw_from_matrix(ds, geom), None, None, None, None

_KD_MAPS = ("camera_feat", "lidar_feat")          # the two feature maps of the objective, in the order of a feature term's part names


def kd_objective(student_logits, student_mids: Dict[str, torch.Tensor], teacher_logits, teacher_mids, target,
                 class_weights=None, T: float = 4.0, alpha: float = 1.0, beta: float = 1.0, ignore_index: int = -1,
                 feature_loss=None, hard_loss=None):
    """total = CE + alpha*T^2*KL + beta*(MSE(camera_feat) + MSE(lidar_feat)); returns (total, parts).
    hard_loss (a RegionLoss): wf*Focal + wt*Tversky takes the CE's place; parts["ce"] then carries it and parts gains "focal"
    and "tversky".  Under data parallelism the Tversky sums cover this rank's shard (see RegionLoss).
    hard_loss (a LovaszLoss): weight * Lovasz is added to its base term (the CE or a RegionLoss); parts["ce"] carries the sum and
    parts gains "lovasz" and "class_lovasz" (and the base's "focal" / "tversky").  A mean over images: exact under data parallelism.
    hard_loss (an OhemCE): the weighted CE over the mined pixels takes the CE's place (2 to 16 classes); parts["ce"] carries it and
    parts gains "ce_all" (the CE over every labelled pixel), "ohem_theta" and "ohem_kept".  Each rank mines its own shard.
    feature_loss (a ChannelKD): beta * (CWD(camera_feat) + CWD(lidar_feat)) at its tau takes the two MSEs' place and parts carries
    "cwd_cam" / "cwd_lidar" instead of "mse_cam" / "mse_lidar".  A mean over images as well.  beta needs re-tuning (see ChannelKD).
    feature_loss (a PairKD): beta * (PAIR(camera_feat) + PAIR(lidar_feat)) takes the two MSEs' place and parts carries "pair_cam" /
    "pair_lidar".  A mean over images as well.  beta needs re-tuning (see PairKD).
    feature_loss (an IntraClassKD): beta * (IFV(camera_feat) + IFV(lidar_feat)) under `target` with the logits' class count takes the
    two MSEs' place and parts carries "ifv_cam" / "ifv_lidar".  The label map must have the feature maps' H x W.  A mean over images
    as well.  beta needs re-tuning (see IntraClassKD)."""
    feat = _term(_FEATURE_TERMS, "feature_loss", feature_loss, KDError)
    hard_term = _term(_HARD_TERMS, "hard_loss", hard_loss, KDError)
    NC = student_logits.shape[1]
    maps = [(student_mids[key], teacher_mids[key]) for key in _KD_MAPS]
    for a, b in maps:                                             # before any launch
        feat.check(a, b, target, NC)
    ce, kl, extra = _hard_seg_loss(hard_term, _AUTOGRAD, student_logits, target, hard_loss, class_weights, ignore_index, teacher_logits, T, alpha)
    f_c, f_l = (feat.value(feature_loss, a, b, target, NC, ignore_index) for a, b in maps)
    # `ce` carries the CE+KL gradient; add KL's value without a second gradient path
    total = ce + (alpha * T * T) * kl.detach() + beta * (f_c + f_l)
    return total, {"ce": ce.detach(), "kl": kl.detach(), feat.parts[0]: f_c.detach(), feat.parts[1]: f_l.detach(), **extra}


def kd_objective_backward(student_logits, student_mids: Dict[str, torch.Tensor], teacher_logits, teacher_mids, target,
                          class_weights=None, T: float = 4.0, alpha: float = 1.0, beta: float = 1.0, ignore_index: int = -1,
                          feature_loss=None, hard_loss=None):
    """kd_objective(...)[0].backward() in one: returns (total, parts) with the student's gradients already propagated.
    hard_loss as in kd_objective: the region-loss call writes dL/dlogits together with L_hard / KL in the CE call's place; the
    Lovasz call follows its base call on the same stream and adds its value and its gradient to what that call wrote, before the
    final kernel reads the hard-label term (parts gains "lovasz"; "class_lovasz" comes from the autograd form only).
    An OhemCE makes ONE kd_seg_ohem_fwd_bwd call in the CE call's place (value, KL and dL/dlogits; parts gains "ce_all",
    "ohem_theta", "ohem_kept").
    feature_loss (a ChannelKD): each map gets ONE kd_feat_cwd_fwd_bwd call that writes the value and the gradient, with
    gcoef = fl32(fl32(tau / (B*C)) * fl32(beta)) -- the product the autograd form's backward call forms on the device from its
    gcoef fl32(tau / (B*C)) and the upstream gradient fl32(beta), so both forms store the same gradient bits; the gradient is
    deposited exactly as the MSE's is, and kd_kd_total forms the total from the two values ("cwd_cam" / "cwd_lidar").
    feature_loss (a PairKD): the same with ONE kd_feat_pair_fwd_bwd call per map and gcoef = fl32(fl32(4 / (B n^2)) * fl32(beta))
    ("pair_cam" / "pair_lidar").
    feature_loss (an IntraClassKD): the same with ONE kd_feat_ifv_fwd_bwd call per map and gcoef = fl32(fl32(2 / B) * fl32(beta))
    ("ifv_cam" / "ifv_lidar"); a label map that has not the feature maps' H x W is refused before the first launch.

    Same values and the same gradient bits as the autograd formulation, fewer passes: the segmentation-loss call writes
    dL/dlogits together with CE / KL; each feature MSE writes its gradient in the pass that sums its value, and that
    gradient is deposited (gradsink.deposit) for the fusion block's projection of the same map, whose data-gradient GEMM
    adds it in its epilogue -- no gradient-accumulation pass over the [B, 128, H, W] maps, no scalar-arithmetic kernels."""
    zs = student_logits
    ops.require_gpu_tensor(zs, "kd_objective_backward")
    if not zs.requires_grad:
        raise KDError("kd_objective_backward: the student logits carry no autograd graph (was the forward run under no_grad?)")
    hard_term = _term(_HARD_TERMS, "hard_loss", hard_loss, KDError)
    feat = _term(_FEATURE_TERMS, "feature_loss", feature_loss, KDError)
    dev = zs.device
    zs_c = zs.detach().contiguous()
    zt_c = teacher_logits.detach().contiguous()
    target = target.contiguous()
    if target.dtype != torch.int64:
        raise KDError("segmentation target must be int64")
    _check_target(zs_c, target)
    _check_class_weights(zs_c, class_weights)
    NC = zs_c.shape[1]
    hard_term.check_classes(hard_loss, NC)
    maps = [(student_mids[key], teacher_mids[key]) for key in _KD_MAPS]
    for a, b in maps:                                             # before any launch
        feat.check(a, b, target, NC)
    bufs = hard_term.alloc(dev)
    hard = bufs[0]                                                # [0] the hard-label term, [1] KL: what the final kernel reads
    dzs = torch.empty_like(zs_c)
    out = torch.empty(3, device=dev, dtype=torch.float32)         # the camera map's feature term, the LiDAR map's, the total
    hard_term.call(hard_loss, zs_c, zt_c, target, class_weights, ignore_index, T, alpha, None, *bufs, dzs)
    gradsink.drop_pending()
    done = []
    for i, (a, b) in enumerate(maps):
        am, geom = ops.nhwc_view(a.detach())
        bm, _ = ops.nhwc_view(b.detach())
        want = beta != 0.0 and a.requires_grad
        da = torch.empty_like(am) if want else None
        done.append(feat.fused_map(feature_loss, am, bm, geom, target, NC, ignore_index, beta, out, i, da))
        if want:
            gradsink.deposit(am, da)
    feat.fused_total(hard, out, done, float(alpha * T * T), float(beta))
    torch.autograd.backward([zs], [dzs])
    if gradsink.pending():
        gradsink.drop_pending()
        raise KDError("kd_objective_backward: a feature-map gradient was not collected by the fusion block's backward "
                      "(unsupported model structure for the fused objective; use kd_objective(...).backward())")
    return out[2], {"ce": hard[0], "kl": hard[1], feat.parts[0]: out[0], feat.parts[1]: out[1],
                    **hard_term.read(hard_loss, _FUSED, bufs, NC)}


def confusion(logits, target, num_classes: int = 2, ignore_index: int = -1, out: Optional[torch.Tensor] = None):
    """Accumulates into (or creates) an int64 [M, M] device confusion matrix, M = num_classes; returns (conf, argmax).
    Up to 16 classes and M <= 16 (KDError beyond).  M need not be the logits' class count: a pixel counts at [t, argmax] when 0 <= t < M and argmax < M (trainer.py:18-26);
    the returned argmax is over all classes."""
    ops.require_gpu_tensor(logits, "confusion")
    z = logits.detach().contiguous()
    B, NC, H, W = z.shape
    M = int(num_classes)
    _check_target(z, target)
    if target.dtype != torch.int64:
        raise KDError("segmentation target must be int64")
    if out is None:
        out = torch.zeros(M, M, device=z.device, dtype=torch.int64)
    elif (out.dtype != torch.int64 or tuple(out.shape) != (M, M) or out.device != z.device or not out.is_contiguous()):
        raise KDError(f"confusion: `out` must be a contiguous int64 [{M}, {M}] tensor on {z.device}, got "
                      f"{tuple(out.shape)} {out.dtype} on {out.device}")
    pred = torch.empty(B, H, W, device=z.device, dtype=torch.int64)
    # up to 4 classes and a 4 x 4 matrix: the entry the default path has always called; beyond, the 16-wide one
    entry = "kd_argmax_confusion" if NC <= 4 and M <= 4 else "kd_argmax_confusion16"
    lib.call(entry, P(z), P(target.contiguous()), int(ignore_index), P(out), P(pred), B, NC, M, H * W, stream())
    return out, pred


def class_weights_from_counts(counts, scheme: str = "median_freq"):
    """Class weights for the weighted cross-entropy from a class histogram of the labels (PandaSetDataset.label_counts), as a list
    of Python floats, computed in float64 on the host.  `median_freq` (median frequency balancing): f_c = counts[c] / sum(counts),
    w_c = median{f_k : counts[k] > 0} / f_c; a class that never occurs gets weight 0.  All-zero, negative or non-integer counts and
    an unknown scheme are a ValueError."""
    if scheme != "median_freq":
        raise ValueError(f"class_weights_from_counts: scheme must be 'median_freq', got {scheme!r}")
    c = np.asarray(counts)
    if c.ndim != 1 or c.size == 0 or not (np.issubdtype(c.dtype, np.integer) or np.issubdtype(c.dtype, np.floating)):
        raise ValueError("class_weights_from_counts: counts must be a non-empty 1-D sequence of numbers")
    c = c.astype(np.float64)
    if not np.all(np.isfinite(c)) or np.any(c < 0) or np.any(c != np.floor(c)):
        raise ValueError("class_weights_from_counts: counts must be non-negative whole numbers")
    if c.sum() <= 0:
        raise ValueError("class_weights_from_counts: every count is zero")
    f = c / c.sum()
    med = np.median(f[c > 0])
    return [float(med / v) if v > 0 else 0.0 for v in f]
