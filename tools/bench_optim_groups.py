#!/usr/bin/env python3
"""KD step at the benchmarked shape with FusedAdamW's parameter groups and EMA weight copy off and on, same process, same box.

  a : today's path      FusedAdamW(student.parameters())                              -> kd_adamw_step_dev
  b : two groups        decay_groups (no weight decay on BatchNorm parameters, biases) -> kd_adamw_step_groups_dev
  c : b + EMA           ema_decay = 0.999 with warm-up
  d : c + clipping      max_grad_norm

B = 256, 80 000 points per frame, eager KDStep.  Every configuration is built once (own models, own optimiser, the same resident
batch) and timed in alternating rounds: a, b, c, d, a, b, ...  Each timing is `--steps` steps between two device synchronisations
after `--warmup` steps.  The table gives every round, the mean and the spread (max - min over rounds) per configuration; the
spread of row a is the noise figure every difference has to be read against.  Below it: the optimiser's own device time, HIP
events around `enqueue_update()` alone (the tick, the update and with clipping the reduction), median of `--opt-iters` calls.
`--base-only` runs row a alone (it then also runs on a tree that predates the feature, for the parent commit's figure).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402

B = 256


def build(key, args, dev):
    from bench import build_models
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    teacher, student = build_models(64, "concat", "weighted")
    teacher, student = teacher.to(dev).eval(), student.to(dev).train()
    if key == "a":
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
    else:
        from kdrt.optim import decay_groups
        kw = {}
        if key in "cd":
            kw.update(ema_decay=0.999, ema_warmup=True)
        if key == "d":
            kw.update(max_grad_norm=args.max_grad_norm)
        opt = FusedAdamW(decay_groups(student, 1e-3, 1e-3), lr=1e-3, weight_decay=1e-3, flat_order=student.parameters(), **kw)
    return KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0), opt


def optimiser_us(opt, iters):
    """median device time of enqueue_update() alone, in microseconds"""
    opt.sync_lr()
    for _ in range(5):
        opt.enqueue_update()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        opt.enqueue_update()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--opt-iters", type=int, default=101)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--base-only", action="store_true", help="time configuration a alone")
    ap.add_argument("--label", default="", help="a line to put at the top of the table (which tree this is)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim_groups.py needs an MI355X: the product path has no CPU fallback")
    from bench import synth_batch
    dev = torch.device("cuda", 0)
    images, pts, labels = synth_batch(B, args.points, 256, 64, 1234, dev)
    names = {"a": "a today", "b": "b groups", "c": "c +ema", "d": "d +clip"}
    runs = {k: build(k, args, dev) for k in ("a" if args.base_only else "abcd")}

    def timed(step):
        for _ in range(args.warmup):
            step(images, pts, labels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(images, pts, labels)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    rows = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, (step, _) in runs.items():
            rows[k].append(timed(step))
    out = ["KD step with FusedAdamW parameter groups / EMA weight copy off and on; times in ms per step",
           f"device: {torch.cuda.get_device_name(0)}; concat teacher -> weighted student, image 3x256x256, BEV 64x64",
           f"B = {B}, {args.points} points per frame, eager KDStep; {args.steps} timed steps after {args.warmup} warm-up per round, "
           f"{args.rounds} alternating rounds", ""]
    if args.label:
        out.insert(0, args.label)
    out.append(f"  {'config':<10}{'ms/step per round':<{10 * args.rounds + 2}}{'mean':>10}{'spread':>10}{'vs a':>10}")
    mean = {k: sum(v) / len(v) for k, v in rows.items()}
    for k, v in rows.items():
        out.append(f"  {names[k]:<10}{' '.join(f'{x:9.3f}' for x in v):<{10 * args.rounds + 2}}{mean[k]:>10.3f}{max(v) - min(v):>10.3f}"
                   f"{mean[k] - mean['a']:>+10.3f}")
    out.append("")
    out.append(f"optimiser alone (HIP events around enqueue_update(), median / min / max of {args.opt_iters} calls, microseconds):")
    for k, (_, opt) in runs.items():
        med, lo, hi = optimiser_us(opt, args.opt_iters)
        extra = ""
        if opt.__dict__.get("grouped"):
            extra = f"   {opt.seg_end_host.numel()} segments, {len(opt.param_groups)} groups"
        out.append(f"  {names[k]:<10}{med:9.1f} {lo:9.1f} {hi:9.1f}   {opt.flat.numel} parameters{extra}")
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
