"""Fused AdamW over one flat parameter buffer (torch.optim.AdamW math, trainer.py:56).

All parameters are re-homed as views of one contiguous fp32 buffer, gradients likewise, so the
optimiser step is ONE kernel launch and the DDP all-reduce works on contiguous bucket slices.
`state_dict()` / `load_state_dict()` keep torch.optim.AdamW's layout (per-parameter `step`,
`exp_avg`, `exp_avg_sq`) so reference checkpoints (`optimizer_state`, trainer.py:116-142) load.

`max_grad_norm` (off by default) clips the gradients to a global L2 norm inside the same device step
(kd_adamw_step_clip_dev): one more reduction launch, no second pass over the gradients, no host sync, so a captured
graph of the step replays it.  `p.grad` keeps the UNCLIPPED gradients after the step (under data parallelism the summed
ones), as it does today for `grad_scale`.  A non-finite gradient norm skips the step on the device instead of writing
NaN into every parameter -- a deliberate departure from torch.nn.utils.clip_grad_norm_.

Parameter groups (torch's list-of-dicts form: per-group `lr` and `weight_decay`; `betas` and `eps` are shared) and an EMA copy
of the weights (`ema_decay`, off by default) go through kd_adamw_step_groups_dev: the same launches, every float4 of the flat
buffer looks its group up in a segment table, and the averaged copy is updated from the registers that hold the new parameters.
Both live on the device, so a captured graph of the step follows a scheduler and the EMA warm-up on replay.  With one group and
no EMA the optimiser calls exactly kd_adamw_step_dev / kd_adamw_step_clip_dev, as before.  `decay_groups` builds the usual
groups: no weight decay on BatchNorm parameters and biases, a learning-rate multiplier per top-level module.

Gradient accumulation (`accum_steps=k`, 1 by default): backward kernels OVERWRITE their slot of the flat gradient buffer, so the
sum over the k micro-batches of a cycle lives in a second flat buffer, `flat.accum`.  `accumulate()` adds the gradient buffer
to it after each of the first k-1 micro-batches; `fold()` after the last writes accum + grad into the gradient buffer and zeroes
accum in the same pass (kd_grad_accumulate), and the step is then the unchanged AdamW entry point on the summed gradient with
`grad_scale / k`.  `AccumCycle` is the bookkeeping KDStep and Trainer share.  With k == 1 nothing is allocated and no call is added.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Iterable, List, Optional

import torch

from .lib import lib
from .ops import P, stream


class FlatParams:
    """Re-homes `params` (in the given order) into one flat buffer; p.data and p.grad become views."""

    def __init__(self, params: Iterable[torch.nn.Parameter]):
        self.params: List[torch.nn.Parameter] = [p for p in params if p.requires_grad]
        dev = self.params[0].device
        sizes = [p.numel() for p in self.params]
        self.offsets = [0]
        for s in sizes:
            self.offsets.append(self.offsets[-1] + ((s + 3) // 4) * 4)      # keep 16-byte alignment per tensor
        self.numel = self.offsets[-1]
        self.data = torch.zeros(self.numel, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(self.numel, device=dev, dtype=torch.float32)
        self.accum: Optional[torch.Tensor] = None        # FusedAdamW(accum_steps > 1): the running sum over micro-batches
        for p, o in zip(self.params, self.offsets):
            n = p.numel()
            self.data[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.data[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):      # re-attach views if something replaced .grad
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view(p.shape)


def decay_groups(model: torch.nn.Module, lr: float, weight_decay: float, lr_mult: Optional[Dict[str, float]] = None,
                 no_decay: bool = True) -> List[dict]:
    """Parameter groups for FusedAdamW (or torch.optim.AdamW): weight decay 0 for every parameter with ndim <= 1 (BatchNorm scales
    and biases, all biases), and `lr * lr_mult[name]` for the parameters of the top-level module `name` (e.g. {"camera_encoder":
    0.1} for a pre-trained encoder).  Groups come in the order their first parameter has in model.named_parameters()."""
    lr_mult = dict(lr_mult or {})
    top = {n for n, _ in model.named_children()}
    unknown = sorted(set(lr_mult) - top)
    if unknown:
        raise ValueError(f"lr_mult names {unknown} are not top-level modules of the model (it has {sorted(top)})")
    groups: Dict[tuple, dict] = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        mult = float(lr_mult.get(name.split(".")[0], 1.0))
        nd = bool(no_decay) and p.ndim <= 1
        g = groups.setdefault((mult, nd), {"params": [], "lr": lr * mult, "weight_decay": 0.0 if nd else weight_decay})
        g["params"].append(p)
    return list(groups.values())


def check_accum_steps(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f"accum_steps must be an int >= 1, got {k!r}")
    return k


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, flat_order=None,
                 ema_decay=None, ema_warmup=False, accum_steps=1):
        params = list(params)
        self.accum_steps = check_accum_steps(accum_steps)
        if max_grad_norm is not None and not (math.isfinite(float(max_grad_norm)) and float(max_grad_norm) > 0):
            raise ValueError(f"max_grad_norm must be None or a finite value > 0, got {max_grad_norm!r}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) <= 1.0:
            raise ValueError(f"ema_decay must be None or lie in [0, 1], got {ema_decay!r}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        for i, g in enumerate(self.param_groups):
            if tuple(float(b) for b in g["betas"]) != tuple(float(b) for b in betas) or float(g["eps"]) != float(eps):
                raise ValueError(f"param group {i}: per-group betas / eps are not supported (betas, eps are shared by all groups: "
                                 f"{tuple(betas)}, {eps}); got betas={tuple(g['betas'])}, eps={g['eps']}")
        # layout of the flat buffer: the concatenation of the groups, or `flat_order` (e.g. model.parameters(), so that contiguous
        # per-module gradient buckets do not depend on the grouping)
        grouped = [p for g in self.param_groups for p in g["params"]]
        order = grouped if flat_order is None else list(flat_order)
        if flat_order is not None and ({id(p) for p in order if p.requires_grad} != {id(p) for p in grouped if p.requires_grad}
                                       or len(order) != len({id(p) for p in order})):
            raise ValueError("flat_order must list exactly the parameters of the groups, each once")
        self.flat = FlatParams(order)
        if self.accum_steps > 1:
            self.flat.accum = torch.zeros_like(self.flat.grad)
        self.exp_avg = torch.zeros_like(self.flat.data)
        self.exp_avg_sq = torch.zeros_like(self.flat.data)
        self._step = 0
        self.epoch = 0                   # bumped on every device update: caches keyed on parameter contents read it
        for q in self.flat.params:       # (ops.owner_epoch -- the update goes through raw pointers, not tensor versions)
            q._kd_owner = self
        self.grad_scale = 1.0            # set to 1/world_size by the DDP wrapper (sum all-reduce)
        # step-to-step state lives on the device so a captured hipGraph of the step replays correctly:
        # dev_state = [lr, step, 1-beta1^step, sqrt(1-beta2^step)]   (kd_adamw_step_dev)
        self.dev_state = torch.zeros(4, device=self.flat.data.device, dtype=torch.float32)
        self._dev_lr = None
        # global-norm clipping: an attribute, not a param_groups key, so state_dict() keeps torch.optim.AdamW's layout.
        # clip_state = [grad_norm, gscale, skipped_steps, last_step_finite]   (kd_adamw_step_clip_dev)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.clip_state = self._clip_ws = None
        if self.max_grad_norm is not None:
            self.clip_state = torch.zeros(4, device=self.flat.data.device, dtype=torch.float32)
            self._clip_ws = torch.zeros(lib.kd_grad_sumsq_ws_bytes(self.flat.numel) // 8, device=self.flat.data.device, dtype=torch.float64)
        for p, o in zip(self.flat.params, self.flat.offsets):
            n = p.numel()
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": self.exp_avg[o:o + n].view(p.shape),
                             "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape)}
        # EMA of the weights: attributes, not param_groups keys, as max_grad_norm is.  ema_state = [d_t, 1 - d_t] on the device.
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = self.ema_state = None
        if self.ema_decay is not None:
            self.ema = self.flat.data.clone()
            self.ema_state = torch.zeros(2, device=self.flat.data.device, dtype=torch.float32)
        # several groups or an EMA: kd_adamw_step_groups_dev with a segment table (ends in float4 units, consecutive tensors of
        # one group merged) and group_state = [G][2] (lr, weight_decay) on the device
        self.grouped = len(self.param_groups) > 1 or self.ema_decay is not None
        self.group_state = self._dev_groups = None
        if self.grouped:
            self.seg_end_host, self.seg_group_host = self.segment_table()
            dev = self.flat.data.device
            self.seg_end, self.seg_group = self.seg_end_host.to(dev), self.seg_group_host.to(dev)
            self.group_state = torch.zeros(len(self.param_groups), 2, device=dev, dtype=torch.float32)

    def segment_table(self):
        """(ends, groups) as int32 CPU tensors: ascending segment ends of the flat buffer in float4 units and the group of each
        segment.  A tensor's padding belongs to it; consecutive tensors of one group share a segment."""
        gidx = {id(p): i for i, g in enumerate(self.param_groups) for p in g["params"]}
        ends, grps = [], []
        for p, e in zip(self.flat.params, self.flat.offsets[1:]):
            if p.numel() == 0:                   # an empty tensor takes no float4
                continue
            if grps and grps[-1] == gidx[id(p)]:
                ends[-1] = e // 4
            else:
                ends.append(e // 4)
                grps.append(gidx[id(p)])
        return torch.tensor(ends, dtype=torch.int32), torch.tensor(grps, dtype=torch.int32)

    def zero_grad(self, set_to_none: bool = False):
        self.flat.zero_grad()

    # ---- gradient accumulation ---------------------------------------------------------------------------------------------
    def _need_accum(self):
        if self.flat.accum is None:
            raise RuntimeError("this needs FusedAdamW(accum_steps=k) with k > 1: no accumulation buffer is kept")

    def accumulate(self):
        """accum += grad over the whole buffer (after each micro-batch of a cycle but the last); one launch"""
        self._need_accum()
        lib.call("kd_grad_accumulate", P(self.flat.accum), P(self.flat.grad), self.flat.numel, 0, stream())

    def fold(self, lo: Optional[int] = None, hi: Optional[int] = None):
        """grad = accum + grad and accum = 0 over the whole buffer, or over the floats [lo, hi) of it (a gradient bucket: tensor
        starts, so 16-byte aligned).  After the last micro-batch of a cycle, once per element, before the step."""
        self._need_accum()
        lo, hi = 0 if lo is None else int(lo), self.flat.numel if hi is None else int(hi)
        if not 0 <= lo <= hi <= self.flat.numel:
            raise ValueError(f"fold: [{lo}, {hi}) is not a slice of the {self.flat.numel} floats of the flat buffer")
        lib.call("kd_grad_accumulate", P(self.flat.accum[lo:hi]), P(self.flat.grad[lo:hi]), hi - lo, 1, stream())

    def sync_lr(self):
        """Push the current learning rate to the device state (call after a scheduler step; cheap no-op otherwise).  With
        parameter groups: every group's lr and weight_decay, into group_state."""
        if self.grouped:
            vals = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]
            if vals != self._dev_groups:
                self.group_state.copy_(torch.tensor(vals, dtype=torch.float32))
                self._dev_groups = vals
            return
        lr = float(self.param_groups[0]["lr"])
        if lr != self._dev_lr:
            self.dev_state[0:1].fill_(lr)
            self._dev_lr = lr

    def enqueue_update(self):
        """The device part of a step (two kernel launches, three with clipping; graph-capturable)."""
        self.epoch += 1
        g = self.param_groups[0]
        if self.grouped:
            clip = self.max_grad_norm is not None
            lib.call("kd_adamw_step_groups_dev", P(self.flat.data), P(self.flat.grad), P(self.exp_avg), P(self.exp_avg_sq),
                     self.flat.numel, P(self.dev_state), P(self.seg_end), P(self.seg_group), P(self.seg_end_host),
                     P(self.seg_group_host), self.seg_end_host.numel(), P(self.group_state), len(self.param_groups), P(self.ema),
                     P(self.ema_state), self.ema_decay or 0.0, int(self.ema_warmup), P(self.clip_state), P(self._clip_ws),
                     self._clip_ws.numel() * 8 if clip else 0, float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                     float(self.grad_scale), self.max_grad_norm if clip else 0.0, stream())
            return
        if self.max_grad_norm is not None:
            lib.call("kd_adamw_step_clip_dev", P(self.flat.data), P(self.flat.grad), P(self.exp_avg), P(self.exp_avg_sq),
                     self.flat.numel, P(self.dev_state), P(self.clip_state), P(self._clip_ws), self._clip_ws.numel() * 8,
                     float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                     float(self.grad_scale), self.max_grad_norm, stream())
            return
        lib.call("kd_adamw_step_dev", P(self.flat.data), P(self.flat.grad), P(self.exp_avg), P(self.exp_avg_sq),
                 self.flat.numel, P(self.dev_state), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
                 float(g["weight_decay"]), float(self.grad_scale), stream())

    @property
    def last_grad_norm(self):
        """0-d device view of the last step's gradient norm (of the gradient the optimiser applied: the rank average under
        data parallelism), taken before clipping.  Reading the attribute does not synchronise."""
        if self.clip_state is None:
            raise RuntimeError("last_grad_norm needs FusedAdamW(max_grad_norm=...): the norm is only computed when clipping is on")
        return self.clip_state[0]

    def skipped_steps(self) -> int:
        """Steps skipped so far because the gradient norm was not finite (one device synchronisation)."""
        return 0 if self.clip_state is None else int(self.clip_state[2].item())

    # ---- the averaged weights ----------------------------------------------------------------------------------------------
    def _need_ema(self):
        if self.ema is None:
            raise RuntimeError("this needs FusedAdamW(ema_decay=...): no averaged copy of the weights is kept")

    def _ema_views(self, model):
        """{state_dict key: view of the EMA buffer} for the parameters of `model` this optimiser owns"""
        off = {id(p): (o, p.numel(), p.shape) for p, o in zip(self.flat.params, self.flat.offsets)}
        return {k: self.ema[off[id(t)][0]:off[id(t)][0] + off[id(t)][1]].view(off[id(t)][2])
                for k, t in model.state_dict(keep_vars=True).items() if id(t) in off}

    def ema_state_dict(self, model):
        """A state_dict of `model` with the EMA values in the place of the parameters and COPIES of the model's current buffers
        (BatchNorm running statistics are not averaged: torch.optim.swa_utils.AveragedModel(use_buffers=False))."""
        self._need_ema()
        views = self._ema_views(model)
        return type(model.state_dict())((k, (views[k] if k in views else t).detach().clone()) for k, t in model.state_dict().items())

    def load_ema(self, state, model=None):
        """Reload the EMA values: from a flat tensor of the buffer's length, or, with the model the names belong to, from a
        mapping as ema_state_dict returns (entries that are not owned parameters are ignored)."""
        self._need_ema()
        if isinstance(state, torch.Tensor):
            self.ema.copy_(state.reshape(-1))
            return
        if model is None:
            raise RuntimeError("load_ema(mapping) needs the model the names belong to: load_ema(state, model)")
        views = self._ema_views(model)
        missing = [k for k in views if k not in state]
        if missing:
            raise KeyError(f"load_ema: the state lacks {missing[:3]}{' ...' if len(missing) > 3 else ''}")
        for k, view in views.items():
            view.copy_(state[k].reshape(view.shape))

    def reset_ema(self):
        """The EMA starts again from the current weights (after loading weights without an EMA)."""
        self._need_ema()
        self.ema.copy_(self.flat.data)

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the block the live flat buffer holds the EMA values; on exit the live values are back, bit for bit.  `epoch`
        goes up both ways so caches keyed on the parameter contents (ops.owner_epoch) refresh.  Not for use inside a capture."""
        self._need_ema()
        live = self.flat.data.clone()
        self.flat.data.copy_(self.ema)
        self.epoch += 1
        try:
            yield self
        finally:
            self.flat.data.copy_(live)
            self.epoch += 1

    def state_dict(self):
        if self.clip_state is not None:          # a skipped step does not count: the device counter is the truth
            self._step = int(self.dev_state[1].item())
            t = torch.tensor(float(self._step))
            for st in self.state.values():
                st["step"] = t
        return super().state_dict()

    def note_steps(self, k: int = 1):
        """Host-side bookkeeping for k device steps (state_dict compatibility with torch.optim.AdamW)."""
        self._step += k
        self.epoch += 1
        t = torch.tensor(float(self._step))
        for st in self.state.values():
            st["step"] = t

    @torch.no_grad()
    def step(self, closure=None):
        self.sync_lr()
        self.enqueue_update()
        self.note_steps(1)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # re-home the loaded moments into the flat buffers.  torch.optim.AdamW creates per-parameter state lazily, so a
        # reference checkpoint may lack it for a parameter that never received a gradient: zeros / step 0 then.
        steps = []
        for p, o in zip(self.flat.params, self.flat.offsets):
            st = self.state[p]
            n = p.numel()
            if "exp_avg" not in st or "exp_avg_sq" not in st:
                st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                st.setdefault("step", torch.tensor(0.0))
            self.exp_avg[o:o + n].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
            st["exp_avg"] = self.exp_avg[o:o + n].view(p.shape)
            st["exp_avg_sq"] = self.exp_avg_sq[o:o + n].view(p.shape)
            steps.append(int(float(st["step"])))
        self._step = max(steps) if steps else 0
        self.epoch += 1
        self.dev_state[1:2].fill_(float(self._step))
        self._dev_lr = self._dev_groups = None


class AccumCycle:
    """The k-micro-batch cycle of a training step's owner (KDStep, Trainer): which call accumulates, which folds and steps.

    begin() before a micro-batch's backward pass says whether it is the last of its cycle and, under data parallelism, opens the
    reducer for that one only (the hooks stay silent on the others: one set of collectives per optimiser step).  finish() after
    the backward pass accumulates (-> False) or folds, sets `grad_scale = (1 / world) * (1 / k)` and steps (-> True); with a
    reducer every bucket is folded by the reducer itself the moment its last gradient lands (BucketedAllReduce.fold), before its
    all-reduce.  flush() steps a partial cycle of j < k micro-batches with divisor j.  With k == 1 finish() is the step as it was:
    `grad_scale = reducer.finish()` or 1, `opt.step()`."""

    def __init__(self, opt: "FusedAdamW", reducer=None, accum_steps: Optional[int] = None):
        k = opt.accum_steps if accum_steps is None else check_accum_steps(accum_steps)
        if k != opt.accum_steps:
            raise ValueError(f"accum_steps={k} disagrees with the optimiser's accum_steps={opt.accum_steps}: build "
                             f"FusedAdamW(accum_steps={k}), which owns the accumulation buffer")
        self.opt, self.reducer, self.k = opt, reducer, k
        self.pending = 0                   # micro-batches accumulated since the last optimiser step
        self.final = True
        if reducer is not None and k > 1:
            reducer.fold = opt.fold

    def begin(self) -> bool:
        self.final = self.pending == self.k - 1
        if self.reducer is not None and self.k > 1:
            self.reducer.enabled = self.final
        return self.final

    def _update(self, scale: float, enqueue_only: bool):
        self.opt.grad_scale = scale
        if enqueue_only:                   # inside a graph capture: the host bookkeeping happens per replay
            self.opt.enqueue_update()
        else:
            self.opt.step()

    def finish(self, enqueue_only: bool = False) -> bool:
        if self.k == 1:
            self._update(self.reducer.finish() if self.reducer is not None else 1.0, enqueue_only)
            return True
        if not self.final:
            self.opt.accumulate()
            self.pending += 1
            return False
        if self.reducer is not None:
            scale = self.reducer.finish()  # folds (and reduces) every bucket the hooks have not launched yet
        else:
            self.opt.fold()
            scale = 1.0
        self.pending = 0
        self._update(scale * (1.0 / self.k), enqueue_only)
        return True

    def flush(self) -> bool:
        """Step on the j < k micro-batches accumulated so far (divisor j); nothing pending: nothing happens.  Every rank of a
        data-parallel job must call it at the same point (their loaders give them the same number of batches)."""
        j = self.pending
        if j == 0:
            return False
        self.opt.zero_grad()               # the last micro-batch's gradient is in accum already: the fold adds zeros to it
        if self.reducer is not None:
            self.reducer.enabled = True
            self.reducer.reset()
            scale = self.reducer.finish()
        else:
            self.opt.fold()
            scale = 1.0
        self.pending = 0
        self._update(scale * (1.0 / j), False)
        return True
