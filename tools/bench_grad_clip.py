#!/usr/bin/env python3
"""KD step with global-norm gradient clipping off and on (FusedAdamW(max_grad_norm=...)), same process, same box.

Two shapes, the two ways the step is run in practice:

  bench : B = 256, 80 000 points per frame, eager KDStep                 (the benchmarked shape)
  ref   : B = 4,   80 000 points per frame, GraphedKDStep (one replayed hipGraph per step: the only way B = 4 runs at rate)

Per shape both configurations are built once (own models, own optimiser, the same resident batch) and timed in alternating
rounds: off, on, off, on, ...  Each timing is `--steps` steps between two device synchronisations after `--warmup` steps.
The table gives every round, the mean and the spread (max - min over rounds) per configuration; the spread of the off rows
is the noise figure the on - off difference has to be read against.  `--off-only` runs the off rows alone (it then also
runs on a tree that predates the feature, for the parent commit's figure).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402

SHAPES = {"bench": (256, False), "ref": (4, True)}


def run_shape(name, args, out):
    from bench import build_models, synth_batch
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    B, graphed = SHAPES[name]
    dev = torch.device("cuda", 0)
    images, pts, labels = synth_batch(B, args.points, 256, 64, 1234, dev)
    runs = {}
    for key, kw in (("off", {}), ("on", {"max_grad_norm": args.max_grad_norm})):
        if key == "on" and args.off_only:
            continue
        teacher, student = build_models(64, "concat", "weighted")
        teacher, student = teacher.to(dev).eval(), student.to(dev).train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3, **kw)
        step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0)
        run = GraphedKDStep(step, images, pts, labels) if graphed else (lambda s=step: s(images, pts, labels))
        runs[key] = (run, opt)

    def timed(run):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    rows = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, (run, _) in runs.items():
            rows[k].append(timed(run))
    out.append(f"shape {name}: B = {B}, {args.points} points per frame, {'GraphedKDStep (replayed hipGraph)' if graphed else 'eager KDStep'}; "
               f"{args.steps} timed steps after {args.warmup} warm-up per round, {args.rounds} alternating rounds")
    out.append(f"  {'clipping':<10}{'ms/step per round':<{10 * args.rounds + 2}}{'mean':>10}{'spread':>10}")
    mean = {}
    for k, v in rows.items():
        mean[k] = sum(v) / len(v)
        out.append(f"  {k:<10}{' '.join(f'{x:9.3f}' for x in v):<{10 * args.rounds + 2}}{mean[k]:>10.3f}{max(v) - min(v):>10.3f}")
    if "on" in rows:
        opt = runs["on"][1]
        out.append(f"  on - off = {mean['on'] - mean['off']:+.3f} ms/step ({(mean['on'] / mean['off'] - 1) * 100:+.2f} %); last grad norm "
                   f"{opt.last_grad_norm.item():.4g}, max_grad_norm {args.max_grad_norm:g}, skipped steps {opt.skipped_steps()}")
    out.append("")
    del runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="bench,ref")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--off-only", action="store_true", help="time the off configuration alone")
    ap.add_argument("--label", default="", help="a line to put at the top of the table (which tree this is)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_clip.py needs an MI355X: the product path has no CPU fallback")
    out = ["KD step with global-norm gradient clipping off / on (FusedAdamW(max_grad_norm=...)); times in ms per step",
           f"device: {torch.cuda.get_device_name(0)}; concat teacher -> weighted student, image 3x256x256, BEV 64x64", ""]
    if args.label:
        out.insert(0, args.label)
    for name in [v for v in args.shapes.split(",") if v]:
        run_shape(name, args, out)
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
