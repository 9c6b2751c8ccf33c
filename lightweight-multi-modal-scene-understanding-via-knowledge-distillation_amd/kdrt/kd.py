"""The knowledge-distillation training step (teacher forward, student forward, CE + T-softmax KL +
feature MSE, student backward, gradient all-reduce, fused AdamW) as one callable.

The reference trains one model with plain CE (trainer.py:86-90) and has no KD code; this step is
what BASELINE.json's north_star adds on top of the reference's `return_intermediates` affordance
(fusion_module.py:234,260-262).  Defaults: T=4, alpha=beta=1."""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import gradsink, ops, units
from .ddp import BucketedAllReduce
from .lib import KDError
from .losses import check_feature_loss, check_hard_loss, kd_objective, kd_objective_backward
from .optim import AccumCycle, FusedAdamW


KD_FEATURES = ("camera_feat", "lidar_feat", "logits")       # what the objective reads of each model's intermediates


class _TakesAccumSteps(type):
    """`KDStep(..., accum_steps=k, feature_loss=spec)`: keyword-only options taken here, so that KDStep.__init__ keeps the argument
    list callers and tests/test_gpu_region_loss.py pin, name for name.  accum_steps None (the default) takes the optimiser's value.
    feature_loss (kdrt.losses.ChannelKD): channel-wise distillation of the two feature maps in the feature MSE's place, or
    (kdrt.losses.PairKD) pair-wise distillation in Gram form, or (kdrt.losses.IntraClassKD) intra-class feature variation distillation
    under the step's label map; None (the default) keeps the MSE and the calls it makes.  All are
    means over images: with equal shards the reducer's averaged gradient is the global batch's.  beta needs re-tuning when switching
    (see ChannelKD, PairKD, IntraClassKD)."""

    def __call__(cls, *args, accum_steps=None, feature_loss=None, **kw):
        check_feature_loss(feature_loss)
        step = super().__call__(*args, **kw)
        step.feature_loss = feature_loss
        step.cycle = AccumCycle(step.opt, step.reducer, accum_steps)
        return step


class KDStep(metaclass=_TakesAccumSteps):
    """Gradient accumulation: with FusedAdamW(accum_steps=k), k > 1, every call is ONE micro-batch.  Calls 1 .. k-1 of a cycle run
    forward and backward and add the gradients to the optimiser's accumulation buffer (no update, no collective;
    parts["stepped"] is False); call k folds the sum into the gradient buffer and steps on it with 1/k (parts["stepped"] is
    True).  BatchNorm statistics are per micro-batch, as in torch.  `flush()` steps a partial cycle.  `accum_steps=k` on this
    constructor only cross-checks the optimiser, which owns the buffer: a different value raises ValueError."""

    def __init__(self, student, teacher, optimizer: FusedAdamW, class_weights: Optional[torch.Tensor] = None,
                 T: float = 4.0, alpha: float = 1.0, beta: float = 1.0, ignore_index: int = -1,
                 reducer: Optional[BucketedAllReduce] = None, teacher_storage: str = "fp32",
                 fused_objective: bool = True, hard_loss=None):
        if teacher_storage not in ("fp32", "bf16"):
            raise ValueError(f"teacher_storage must be 'fp32' or 'bf16', got {teacher_storage!r}")
        if teacher_storage == "bf16":
            cls_conv = getattr(getattr(teacher, "head", None), "cls", None)
            nc = cls_conv.weight.shape[0] if cls_conv is not None else 0
            if nc > 4:             # here and not at the first step: the bf16 classifier kernel is the limit
                raise KDError(f"teacher_storage='bf16': the bf16 classifier (kd_bf16_cls_conv) holds at most 4 classes, the teacher "
                              f"emits {nc}; 5 to 16 classes need teacher_storage='fp32'")
        # fused objective (default): loss values and loss gradients from the same kernel passes, feature-MSE gradients added
        # inside the fusion block's data-gradient GEMMs (losses.kd_objective_backward); False keeps the
        # autograd formulation kd_objective(...).backward() -- same bits, more passes (tests compare the two)
        self.fused_objective = bool(fused_objective)
        # "bf16": the frozen teacher runs kdrt.bf16.forward_bf16 (bf16 activations in HBM, fp32 accumulate); a second,
        # separately gated mode -- the default keeps every tensor of the step fp32
        self.teacher_storage = teacher_storage
        self.student, self.teacher, self.opt = student, teacher, optimizer
        self.cw, self.T, self.alpha, self.beta, self.ignore_index = class_weights, T, alpha, beta, ignore_index
        # hard_loss (kdrt.losses.RegionLoss): wf*Focal + wt*Tversky as the hard-label term instead of the weighted CE; None keeps
        # the CE.  Data parallel: the Tversky sums cover each rank's own shard, the reducer averages the per-rank gradients.
        # A kdrt.losses.LovaszLoss adds weight * Lovasz-Softmax to its base term (the CE or a RegionLoss): a mean over images, so
        # with equal shards the averaged per-rank gradient is the global batch's.
        # A kdrt.losses.OhemCE averages the weighted CE over the mined pixels only (2 to 16 classes): one kd_seg_ohem_fwd_bwd call in
        # the CE call's place, no host read, so GraphedKDStep replays it unchanged.  Each rank mines its own shard.
        check_hard_loss(hard_loss)
        self.hard_loss = hard_loss
        self.reducer = reducer
        self.sink = gradsink.install(optimizer.flat, reducer)      # backward kernels write into the flat grad buffer
        self.teacher.eval()
        for p in self.teacher.parameters():
            p.requires_grad_(False)

    def teacher_forward(self, images, points):
        with torch.no_grad():
            if self.teacher_storage == "bf16":
                from .bf16 import forward_bf16
                return forward_bf16(self.teacher, images, points, return_intermediates=KD_FEATURES)
            return self.teacher(images, points, return_intermediates=KD_FEATURES)

    def objective_backward(self, zs, ms, zt, mt, labels):
        """Loss values + the student's backward pass -> (total, parts of detached device scalars)."""
        a = (zs, ms, zt, mt, labels, self.cw, self.T, self.alpha, self.beta, self.ignore_index)
        if self.fused_objective:
            return kd_objective_backward(*a, feature_loss=self.feature_loss, hard_loss=self.hard_loss)
        total, parts = kd_objective(*a, feature_loss=self.feature_loss, hard_loss=self.hard_loss)
        gradsink.drop_pending()
        total.backward()
        if gradsink.pending():
            gradsink.drop_pending()
            raise RuntimeError("a deposited feature gradient was not collected (kdrt.gradsink): set KD_GRAD_ROUTING=0")
        return total.detach(), parts

    def flush(self) -> bool:
        """Step on a partial cycle (j < k accumulated micro-batches, divisor j) -> whether a step was made"""
        return self.cycle.flush()

    def __call__(self, images, points, labels):
        self.cycle.begin()
        units.share_point_bins(True)       # teacher and student of THIS step sort the same points once ...
        try:
            zt, mt = self.teacher_forward(images, points)
            gradsink.active = self.sink
            self.sink.begin_step()
            self.opt.zero_grad()
            zs, ms = self.student(images, points, return_intermediates=KD_FEATURES)
        finally:
            units.share_point_bins(False)  # ... and nothing of it outlives the two forward passes
        total, parts = self.objective_backward(zs, ms, zt, mt, labels)
        self.sink.end_step()
        stepped = self.cycle.finish()
        if self.cycle.k > 1:
            parts["stepped"] = stepped
        if stepped and self.opt.max_grad_norm is not None:
            parts["grad_norm"] = self.opt.last_grad_norm      # device scalar (pre-clip norm of the applied gradient): no sync
        parts["total"] = total
        parts["logits"] = zs.detach()
        return parts


class GraphedKDStep:
    """The whole KD step captured ONCE into a hipGraph (through torch.cuda.CUDAGraph) and replayed:
    ~600 kernel launches become one graph launch, so small per-GPU batches (the reference trains at
    B=4) are no longer bound by the ~5.8 ms of host launch work per step.  Everything that varies
    between steps lives on the device: the batch is copied into static input buffers, the AdamW
    step counter / bias corrections / learning rate are device state (kd_adamw_step_dev), BatchNorm
    running statistics are updated by the kernels themselves.

    With a gradient reducer (data parallel) the bucketed all-reduces are captured INSIDE the graph: ProcessGroupNCCL
    forks its collective stream off the capturing stream with an event and `work.wait()` joins it back, so the replayed
    graph holds backward kernels -> RCCL all-reduce per bucket -> AdamW with the same dependencies as the eager step.
    The capture then runs in "thread_local" error mode (the process group's watchdog thread polls events of earlier
    collectives from another thread, which the default "global" mode would treat as a capture violation).

    Over a KDStep with gradient accumulation (accum_steps = k > 1) the graph holds one whole CYCLE: the static buffers and
    `__call__` take k * B frames, the captured body runs the k micro-batches on consecutive slices of B frames (k - 1
    accumulations, one fold, one AdamW update), and a replay is one optimiser step.  The returned parts are those of the last
    micro-batch, except "logits" (all k * B frames) and "total" (the mean of the k micro-batch losses).  Not with a reducer.

    Restrictions: fixed batch shape; `optimizer.sync_lr()` happens automatically before each replay; more than one rank is
    an explicit opt-in (see __init__)."""

    def __init__(self, step: KDStep, images, points, labels, warmup: int = 3, allow_multi_rank: bool = False):
        # Captured collectives have only ever executed in a world of ONE rank here (tests/test_gpu_rccl_world1.py: a real RCCL
        # communicator, forced buckets); a multi-rank capture or replay problem would show as a hang in user training, so a
        # world of more than one rank is refused unless the caller opts in (`allow_multi_rank=True` / KD_GRAPH_MULTI_RANK=1)
        # -- to be lifted once a multi-GPU run has executed the captured path.
        world = step.reducer.world if step.reducer is not None else 1
        if world > 1 and not (allow_multi_rank or os.environ.get("KD_GRAPH_MULTI_RANK") == "1"):
            raise RuntimeError(f"GraphedKDStep: capturing the gradient all-reduces of a {world}-rank job has not run on hardware "
                               "yet; pass allow_multi_rank=True (or KD_GRAPH_MULTI_RANK=1) to try it, or use the eager KDStep")
        self.k = k = step.cycle.k
        if k > 1 and step.reducer is not None:
            raise RuntimeError("GraphedKDStep: gradient accumulation (accum_steps > 1) together with a gradient reducer inside a "
                               "capture is not supported; use the eager KDStep")
        if k > 1 and (step.cycle.pending or images.shape[0] % k):
            raise RuntimeError(f"GraphedKDStep: accum_steps={k} needs k * B frames ({images.shape[0]} given) and a KDStep at the "
                               "start of a cycle")
        self.step = step
        self.images, self.points, self.labels = images.clone(), points.clone(), labels.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm-up on a side stream (allocator, workspaces, caches)
            for _ in range(warmup):
                for im, pt, lb in self._micro_batches():    # (whole cycles: the capture starts at the beginning of one)
                    self.out = step(im, pt, lb)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        step.opt.sync_lr()
        mode = {} if step.reducer is None else {"capture_error_mode": "thread_local"}
        with torch.cuda.graph(self.graph, **mode):
            self.out = self._body()
        self.transposes = ops.TRANSPOSES.hold()     # the captured W^T refresh reads this table: it lives as long as the graph
        self.replays = 0

    def _micro_batches(self):
        """the static buffers as k slices of B frames (k == 1: the buffers themselves)"""
        if self.k == 1:
            return [(self.images, self.points, self.labels)]
        B = self.images.shape[0] // self.k
        return [(self.images[j * B:(j + 1) * B], self.points[j * B:(j + 1) * B], self.labels[j * B:(j + 1) * B]) for j in range(self.k)]

    def _body(self):
        s = self.step
        totals, logits = [], []
        for images, points, labels in self._micro_batches():
            s.cycle.begin()
            zt, mt = s.teacher_forward(images, points)
            gradsink.active = s.sink
            s.sink.begin_step()
            s.opt.zero_grad()
            zs, ms = s.student(images, points, return_intermediates=KD_FEATURES)
            total, parts = s.objective_backward(zs, ms, zt, mt, labels)
            s.sink.end_step()
            stepped = s.cycle.finish(enqueue_only=True)
            totals.append(total)
            logits.append(zs.detach())
        if s.opt.max_grad_norm is not None:
            parts["grad_norm"] = s.opt.last_grad_norm
        if self.k > 1:
            parts["stepped"] = stepped
            parts["total"] = torch.stack(totals).mean()
            parts["logits"] = torch.cat(logits)
        else:
            parts["total"] = total
            parts["logits"] = zs.detach()
        return parts

    def __call__(self, images=None, points=None, labels=None):
        if images is not None:
            self.images.copy_(images, non_blocking=True)
            self.points.copy_(points, non_blocking=True)
            self.labels.copy_(labels, non_blocking=True)
        self.step.opt.sync_lr()
        self.graph.replay()
        ops.bump_global_epoch()            # the replay rewrote parameters and BatchNorm buffers behind torch's back
        self.step.opt.note_steps(1)
        self.replays += 1
        return self.out
