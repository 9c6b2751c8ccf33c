"""MI355X-native training loop -- drop-in for the reference's src/training/trainer.py.

`Trainer` and `SegmentationMetrics` keep the reference's constructor signatures, method names,
checkpoint dictionary keys and history JSON layout (trainer.py:9-194).  What changed underneath:
the loss is the fused HIP CE kernel, the optimiser is the one-launch fused AdamW over a flat
buffer (state_dict-compatible with torch.optim.AdamW), the confusion matrix is accumulated on the
device by an integer kernel instead of a per-pixel Python loop (107 ms per batch in the reference),
and `loss.item()` is read once per epoch instead of once per step (no per-step host sync).

`KDTrainer` adds what BASELINE.json's north_star names and the reference lacks: a frozen teacher,
the CE + T^2*KL + feature-MSE objective, and (when torch.distributed is initialised) the bucketed
RCCL gradient all-reduce overlapped with backward.
"""
import json
import os

import numpy as np
import torch
import torch.distributed as dist
import torch.optim as optim

from kdrt import gradsink
from kdrt.ddp import BucketedAllReduce, broadcast_buffers, broadcast_module, distributed
from kdrt.kd import KDStep
from kdrt.losses import OhemCE, check_feature_loss, check_hard_classes, check_hard_loss, confusion, hard_seg_loss, seg_loss
from kdrt.optim import AccumCycle, FusedAdamW, check_accum_steps, decay_groups

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(x, **kw):
        return x


def optim_options_from_env(env=None):
    """Trainer keywords from the entry scripts' switches: KD_EMA_DECAY=0.999, KD_EMA_WARMUP=1, KD_NO_DECAY_NORM_BIAS=1,
    KD_LR_MULT="camera_encoder=0.1,lidar_encoder=0.5", KD_ACCUM_STEPS=4 (an integer >= 1: loader batches per optimiser step).
    Nothing set: {} -- the scripts then build the trainer exactly as before."""
    env = os.environ if env is None else env
    kw = {}
    if env.get("KD_EMA_DECAY"):
        kw["ema_decay"] = float(env["KD_EMA_DECAY"])
        kw["ema_warmup"] = env.get("KD_EMA_WARMUP") == "1"
    elif env.get("KD_EMA_WARMUP") == "1":
        raise ValueError("KD_EMA_WARMUP=1 needs KD_EMA_DECAY")
    if env.get("KD_NO_DECAY_NORM_BIAS") == "1":
        kw["no_decay_norm_bias"] = True
    if env.get("KD_LR_MULT"):
        mult = {}
        for item in env["KD_LR_MULT"].split(","):
            name, sep, val = item.partition("=")
            if not sep or not name.strip():
                raise ValueError(f"KD_LR_MULT must look like 'camera_encoder=0.1,head=2', got {env['KD_LR_MULT']!r}")
            mult[name.strip()] = float(val)
        kw["lr_mult"] = mult
    if env.get("KD_ACCUM_STEPS"):
        try:
            k = int(env["KD_ACCUM_STEPS"])
        except ValueError:
            raise ValueError(f"KD_ACCUM_STEPS must be an integer >= 1, got {env['KD_ACCUM_STEPS']!r}") from None
        kw["accum_steps"] = check_accum_steps(k)
    return kw


class SegmentationMetrics:
    """Confusion-matrix mIoU.  `update` accepts logits [B,C,H,W] and int64 targets [B,H,W] on the GPU
    (integer-exact device kernel) -- same semantics as the reference's numpy loop."""

    def __init__(self, num_classes=2, ignore_index=-1, device=None):
        self.num_classes = num_classes
        self.ignore_index = ignore_index
        self.device = device             # only needed by a data-parallel rank that never sees a batch (see _sync)
        self.reset()

    def reset(self):
        self._dev = None
        self.confusion = np.zeros((self.num_classes, self.num_classes), dtype=np.int64)

    def update(self, preds, targets):
        self._dev, _ = confusion(preds, targets, self.num_classes, self.ignore_index, out=self._dev)

    def _sync(self):
        if distributed():
            # Data parallel: every rank counted its own shard of the frames.  EVERY rank takes part in the all-reduce,
            # also one whose shard was empty (fewer validation frames than ranks): a skipped collective would pair with
            # the next one the other ranks issue -- a hang or silently mixed tensors.
            if self._dev is not None:
                g = self._dev.clone()               # (the device matrix keeps this rank's own counts)
            else:
                dev = self.device
                if dev is None:
                    dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
                g = torch.zeros(self.num_classes, self.num_classes, device=dev, dtype=torch.int64)
            dist.all_reduce(g)
            self.confusion = g.cpu().numpy().astype(np.int64)
        elif self._dev is not None:
            self.confusion = self._dev.cpu().numpy().astype(np.int64)

    def compute(self):
        self._sync()
        ious = []
        for i in range(self.num_classes):
            tp = self.confusion[i, i]
            fp = self.confusion[:, i].sum() - tp
            fn = self.confusion[i, :].sum() - tp
            denom = tp + fp + fn
            ious.append(tp / denom if denom > 0 else 0.0)
        return {"class_iou": ious, "miou": float(np.mean(ious))}


class _TakesNumClasses(type):
    """`Trainer(..., num_classes=n)` / `KDTrainer(..., num_classes=n)`: a keyword-only option taken here, so that Trainer.__init__
    keeps the argument list the tests pin, name for name (as KDStep does for accum_steps and feature_loss).  None (the default)
    changes nothing."""

    def __call__(cls, *args, num_classes=None, **kw):
        if num_classes is not None and (isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= 16):
            raise ValueError(f"num_classes must be an integer in [2, 16] or None, got {num_classes!r}")
        trainer = super().__call__(*args, **kw)
        trainer.set_num_classes(num_classes)
        return trainer


class Trainer(metaclass=_TakesNumClasses):
    def __init__(self, model, train_loader, val_loader, device, lr=1e-3, weight_decay=1e-3, save_dir="checkpoints",
                 class_weights=None, num_epochs=20, accum_steps=1, max_grad_norm=None, ema_decay=None, ema_warmup=False,
                 no_decay_norm_bias=False, lr_mult=None, hard_loss=None):
        self.model = model
        self.train_loader = train_loader
        self.val_loader = val_loader
        self.device = device
        self.num_epochs = num_epochs
        if class_weights is not None:
            class_weights = torch.FloatTensor(class_weights).to(device)
        self.class_weights = class_weights
        self.ignore_index = -1
        self.num_classes, self.metric_classes = None, 2        # `num_classes=` is taken by _TakesNumClasses, see set_num_classes
        self.train_confusion = self.val_confusion = None       # the confusion matrices of the last train_epoch() / validation pass
        # hard_loss (kdrt.losses.RegionLoss): train AND validate with wf*Focal + wt*Tversky instead of the weighted CE (the class
        # weights then enter the focal term only).  Data parallel: the Tversky sums cover each rank's own shard of the batch.
        # hard_loss (kdrt.losses.LovaszLoss): its base term (the weighted CE or a RegionLoss) + weight * Lovasz-Softmax, a mean over
        # images (exact under data parallelism with equal shards); maps of at most 128 x 128 pixels.
        # hard_loss (kdrt.losses.OhemCE): the weighted CE over the mined pixels, 2 to 16 classes.  Mining is a training device:
        # validation reports the plain weighted CE.  Data parallel: each rank mines its own shard.
        check_hard_loss(hard_loss)
        self.hard_loss = hard_loss
        self.criterion = lambda logits, seg: hard_seg_loss(logits, seg, self.hard_loss, self.class_weights, self.ignore_index)[0]
        self.val_criterion = None                              # None: validate with the training criterion
        if isinstance(hard_loss, OhemCE):
            self.val_criterion = lambda logits, seg: seg_loss(logits, seg, self.class_weights, self.ignore_index)[0]
        # Parameter groups (no weight decay on BatchNorm parameters and biases, a learning-rate multiplier per top-level module)
        # and an EMA of the weights: all off by default, and the optimiser then makes exactly the calls it made before.  The
        # flat buffer keeps the model.parameters() order whatever the grouping, so the gradient buckets stay contiguous.
        self.ema_decay = ema_decay
        params = model.parameters()
        if no_decay_norm_bias or lr_mult:
            params = decay_groups(model, lr, weight_decay, lr_mult, no_decay=bool(no_decay_norm_bias))
        # Gradient accumulation (accum_steps = k > 1): every loader batch is one micro-batch, an optimiser step is made on every
        # k-th (and on what is left when the loader is exhausted), on the mean of the k gradients; BatchNorm statistics, the loss
        # and the metrics stay per batch.  Under data parallelism the gradients are reduced once per optimiser step.
        self.accum_steps = check_accum_steps(accum_steps)
        self.optimizer = FusedAdamW(params, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm,
                                    flat_order=model.parameters(), ema_decay=ema_decay, ema_warmup=ema_warmup,
                                    accum_steps=self.accum_steps)
        self.scheduler = optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=num_epochs, eta_min=1e-5)
        # Data parallel (torch.distributed initialised, world > 1): every rank starts from rank 0's weights and the
        # gradients are summed over ranks in buckets as backward produces them (kdrt.ddp), for plain CE training as for KD.
        self.reducer = None
        if distributed():
            broadcast_module(model)
            if ema_decay is not None:          # the EMA was cloned from this rank's own initial weights: restart it from rank 0's,
                self.optimizer.reset_ema()     # so that it is the same function of the same parameters on every rank
            names = [n for n, p in model.named_parameters() if p.requires_grad]
            self.reducer = BucketedAllReduce(self.optimizer.flat, names, n_buckets=3)
        self.is_main = not distributed() or dist.get_rank() == 0
        if class_weights is not None:
            self._log(f"Using class weights: {class_weights.tolist()}")
        self.sink = gradsink.install(self.optimizer.flat, self.reducer)   # backward kernels write into the flat grad buffer
        self.cycle = AccumCycle(self.optimizer, self.reducer)
        self.stepped = True              # whether the last _step() made an optimiser step (always, without accumulation)
        self.save_dir = save_dir
        self.epoch = 0
        if self.is_main:
            os.makedirs(save_dir, exist_ok=True)
        self.best_miou = 0.0
        self.history_path = os.path.join(save_dir, "training_history.json")
        self.history = {"train_loss": [], "train_miou": [], "val_loss": [], "val_miou": [], "lr": []}
        # global-norm gradient clipping (FusedAdamW(max_grad_norm=...)): off by default, and the history then keeps the
        # reference's layout; on, it gains the epoch mean of the pre-clip gradient norm and the count of skipped steps.
        # Under data parallelism the norm is taken after reducer.finish(), over the summed buffer, so every rank computes
        # the same coefficient and the same skip decision without a further collective.
        self.max_grad_norm = max_grad_norm
        if max_grad_norm is not None:
            self.history.update({"grad_norm": [], "skipped_steps": []})
        self.last_epoch_grad_norm = None
        # EMA on: validation, best.pth and the checkpoint's "ema_state" use the averaged weights (the model's own BatchNorm
        # statistics with them); "val_miou_live" holds the live weights' mIoU when KD_EMA_VALIDATE_LIVE=1, None otherwise.
        # The EMA is a function of the parameters, identical on every rank once it starts from the broadcast weights (above):
        # no collective.
        if ema_decay is not None:
            self.history["val_miou_live"] = []
        self.last_val_miou_live = None

    def set_num_classes(self, num_classes):
        """num_classes (None, the default: the reference's 2-class metrics on whatever the head emits): the width of the confusion
        matrix of training and validation, 2 to 16; it must agree with the length of class_weights.  The head's own class count
        is the model's (CompleteSegmentationModel(num_classes=...)); more than 4 classes need the same-resolution head, the weighted
        CE (hard_loss=None) or its mined form (an OhemCE) and, for KD, an fp32 teacher."""
        if num_classes is not None:
            if self.class_weights is not None and self.class_weights.numel() != num_classes:
                raise ValueError(f"class_weights has {self.class_weights.numel()} entries for num_classes={num_classes}")
            check_hard_classes(self.hard_loss, num_classes)
        self.num_classes = num_classes
        self.metric_classes = 2 if num_classes is None else num_classes

    def _log(self, *a, **k):
        """Console output of the training loop: rank 0 only under data parallelism (errors and warnings of the other
        ranks still reach their own stderr -- nothing is patched process-wide)."""
        if self.is_main:
            print(*a, **k)

    # one loader batch: an optimisation step, or with accum_steps > 1 a micro-batch of one; overridden by KDTrainer
    def _step(self, imgs, pts, seg):
        self.cycle.begin()
        gradsink.active = self.sink
        self.sink.begin_step()           # (also drops anything an earlier step that failed half-way -- a caught OOM -- left deposited)
        self.optimizer.zero_grad()
        logits = self.model(imgs, pts)
        loss = self.criterion(logits, seg)
        loss.backward()
        if gradsink.pending():           # a feature-map gradient deposited for a later kernel that never ran: a missing gradient term
            gradsink.drop_pending()
            raise RuntimeError("a deposited feature gradient was not collected (kdrt.gradsink): unsupported model structure; set KD_GRAD_ROUTING=0")
        self.sink.end_step()
        self.stepped = self.cycle.finish()
        return loss.detach(), logits.detach()

    def flush(self):
        """Step on a partial accumulation cycle (fewer than accum_steps batches since the last optimiser step), dividing by
        their number -> whether a step was made.  train_epoch calls it when the loader is exhausted: no gradient crosses an
        epoch or reaches a checkpoint."""
        self.stepped = self.cycle.flush()
        return self.stepped

    def _mean_over_ranks(self, total, n_batches):
        """(sum of per-batch losses, batch count) -> mean over every rank's batches."""
        if distributed():
            t = torch.stack([total.double(), torch.tensor(float(n_batches), device=total.device, dtype=torch.float64)])
            dist.all_reduce(t)
            return float(t[0].item() / max(t[1].item(), 1.0))
        return total.item() / max(n_batches, 1)

    def train_epoch(self):
        self.model.train()
        metrics = SegmentationMetrics(num_classes=self.metric_classes, device=self.device)
        total = torch.zeros((), device=self.device)
        gnorm = torch.zeros((), device=self.device) if self.max_grad_norm is not None else None
        steps = 0
        if hasattr(self.train_loader, "set_epoch"):       # rank-sharded loaders reshuffle per epoch, identically on all ranks
            self.train_loader.set_epoch(self.epoch)
        for batch in tqdm(self.train_loader, desc="Train", disable=not self.is_main):
            imgs = batch["image"].to(self.device, non_blocking=True)
            pts = batch["points"].to(self.device, non_blocking=True)
            seg = batch["segmentation"].to(self.device, non_blocking=True)
            loss, logits = self._step(imgs, pts, seg)
            total += loss                      # stays on the device: no per-step sync
            if gnorm is not None and self.stepped:
                gnorm += self.optimizer.last_grad_norm
                steps += 1
            metrics.update(logits, seg)
        if self.flush() and gnorm is not None:
            gnorm += self.optimizer.last_grad_norm
            steps += 1
        if gnorm is not None:                  # identical on every rank: no mean over ranks (a skipped step's inf / NaN shows here)
            # the mean over optimiser steps (without accumulation: one per loader batch, the divisor as it was)
            self.last_epoch_grad_norm = gnorm.item() / max(steps if self.accum_steps > 1 else len(self.train_loader), 1)
        out = metrics.compute()
        self.train_confusion = metrics.confusion.copy()      # int64 [metric_classes, metric_classes], summed over ranks
        return self._mean_over_ranks(total, len(self.train_loader)), out

    def validate(self):
        if self.ema_decay is None:
            return self._validate()
        with self.optimizer.swap_ema():
            out = self._validate()
        self.last_val_miou_live = self._validate()[1]["miou"] if os.environ.get("KD_EMA_VALIDATE_LIVE") == "1" else None
        return out

    def _validate(self):
        self.model.eval()
        if distributed():
            broadcast_buffers(self.model)       # all ranks evaluate rank 0's BatchNorm statistics (the model that is saved)
        metrics = SegmentationMetrics(num_classes=self.metric_classes, device=self.device)
        total = torch.zeros((), device=self.device)
        with torch.no_grad():
            for batch in tqdm(self.val_loader, desc="Val", disable=not self.is_main):
                imgs = batch["image"].to(self.device, non_blocking=True)
                pts = batch["points"].to(self.device, non_blocking=True)
                seg = batch["segmentation"].to(self.device, non_blocking=True)
                logits = self.model(imgs, pts)
                total += (self.val_criterion or self.criterion)(logits, seg)
                metrics.update(logits, seg)
        out = metrics.compute()
        self.val_confusion = metrics.confusion.copy()
        return self._mean_over_ranks(total, len(self.val_loader)), out

    def save_checkpoint(self, epoch, val_miou, is_best=False):
        if not self.is_main:
            return
        ckpt = {"epoch": epoch, "model_state": self.model.state_dict(), "optimizer_state": self.optimizer.state_dict(),
                "scheduler_state": self.scheduler.state_dict(), "val_miou": val_miou}
        if self.ema_decay is not None:         # loads with model.load_state_dict(ckpt["ema_state"]); "model_state" stays the live weights
            ckpt["ema_state"] = self.optimizer.ema_state_dict(self.model)
        torch.save(ckpt, os.path.join(self.save_dir, "latest.pth"))
        if is_best:
            torch.save(ckpt, os.path.join(self.save_dir, "best.pth"))

    def load_checkpoint(self, path):
        ckpt = torch.load(path, map_location=self.device)
        self.model.load_state_dict(ckpt["model_state"])
        self.optimizer.load_state_dict(ckpt["optimizer_state"])
        if self.ema_decay is not None:
            if "ema_state" in ckpt:
                self.optimizer.load_ema(ckpt["ema_state"], self.model)
            else:                              # a checkpoint written without an EMA: the average starts from its weights
                self.optimizer.reset_ema()
        if "scheduler_state" in ckpt:
            self.scheduler.load_state_dict(ckpt["scheduler_state"])
        self.best_miou = ckpt.get("val_miou", 0.0)
        start_epoch = ckpt.get("epoch", 0) + 1
        self._log(f"Resumed from {path}, starting at epoch {start_epoch}, best mIoU {self.best_miou:.4f}")
        return start_epoch

    def update_history(self, train_loss, train_miou, val_loss, val_miou, lr):
        for k, v in zip(("train_loss", "train_miou", "val_loss", "val_miou", "lr"),
                        (train_loss, train_miou, val_loss, val_miou, lr)):
            self.history[k].append(v)
        if self.max_grad_norm is not None:
            self.history["grad_norm"].append(self.last_epoch_grad_norm)
            self.history["skipped_steps"].append(self.optimizer.skipped_steps())
        if self.ema_decay is not None:
            self.history["val_miou_live"].append(self.last_val_miou_live)
        if self.is_main:                       # one writer: ranks share the working directory
            with open(self.history_path, "w") as f:
                json.dump(self.history, f, indent=2)

    def train(self, start_epoch=0):
        self._log(f"\nStarting training from epoch {start_epoch + 1}/{self.num_epochs}")
        self._log("=" * 60)
        for epoch in range(start_epoch, self.num_epochs):
            self.epoch = epoch
            self._log(f"\nEpoch {epoch+1}/{self.num_epochs}")
            self._log("-" * 60)
            train_loss, train_metrics = self.train_epoch()
            val_loss, val_metrics = self.validate()
            self.scheduler.step()
            current_lr = self.optimizer.param_groups[0]["lr"]
            train_miou, val_miou = train_metrics["miou"], val_metrics["miou"]
            self._log("\nResults:")
            self._log(f"  Train Loss: {train_loss:.4f} | Train mIoU: {train_miou:.4f}")
            self._log(f"  Val Loss:   {val_loss:.4f} | Val mIoU:   {val_miou:.4f}")
            self._log(f"  Learning Rate: {current_lr:.6f}")
            self._log("\n  Per-class IoU (Val):")
            names = ["Background", "Drivable"] if self.num_classes is None else ["Background"] + [f"Class {i}" for i in range(1, self.num_classes)]
            for name, iou in zip(names, val_metrics["class_iou"]):
                self._log(f"    {name:12s}: {iou:.4f}")
            self.update_history(train_loss, train_miou, val_loss, val_miou, current_lr)
            is_best = val_miou > self.best_miou
            if is_best:
                self.best_miou = val_miou
                self._log(f"  New best mIoU: {val_miou:.4f}")
            self.save_checkpoint(epoch, val_miou, is_best=is_best)
        self._log("\n" + "=" * 60)
        self._log(f"Training completed! Best validation mIoU: {self.best_miou:.4f}")
        self._log("=" * 60)
        return self.best_miou


class KDTrainer(Trainer):
    """Teacher -> student distillation on top of `Trainer`.  total = CE + alpha*T^2*KL + beta*(MSE(camera_feat)
    + MSE(lidar_feat)) (`hard_loss=RegionLoss(...)`: focal + Tversky in the CE's place; `feature_loss=ChannelKD(tau)`: channel-wise
    distillation of the two feature maps in the MSEs' place, `feature_loss=PairKD()`: pair-wise distillation in Gram form,
    `feature_loss=IntraClassKD()`: intra-class feature variation distillation under the labels, training only -- validation reports the hard-label loss -- and beta
    needs re-tuning); the teacher runs in eval mode under no_grad.  With torch.distributed initialised the
    student is broadcast from rank 0 and gradients are all-reduced in buckets overlapped with backward."""

    def __init__(self, model, teacher, train_loader, val_loader, device, T=4.0, alpha=1.0, beta=1.0, feature_loss=None, **kw):
        check_feature_loss(feature_loss)
        super().__init__(model, train_loader, val_loader, device, **kw)
        self.teacher = teacher
        if distributed():
            broadcast_module(teacher)           # (a teacher loaded from the same checkpoint on every rank: a no-op in value)
        self.kd_step = KDStep(model, teacher, self.optimizer, self.class_weights, T, alpha, beta, self.ignore_index, self.reducer,
                              hard_loss=self.hard_loss, feature_loss=feature_loss)
        self.sink = self.kd_step.sink
        self.cycle = self.kd_step.cycle         # one cycle: the KD step's (flush() goes to it)

    def _step(self, imgs, pts, seg):
        parts = self.kd_step(imgs, pts, seg)
        self.stepped = parts.get("stepped", True)
        return parts["total"], parts["logits"]
