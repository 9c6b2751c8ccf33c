#!/usr/bin/env python3
"""Gradient accumulation against plain steps at the benchmarked frame shape, same box, one call.

  i   : k plain KD steps of B frames          FusedAdamW(student.parameters()), k optimiser steps
  ii  : one accumulating cycle of k x B       FusedAdamW(..., accum_steps=k): k - 1 accumulate launches, one fold, ONE optimiser step
  iii : row i of this tree against row i of a build of the parent commit (`--parent-tree DIR`: a checkout with its own
        csrc/libkd_hip.so), the plain step at accum_steps = 1 against the step as it was

B = 64 frames per micro-batch, k = 4, 80 000 points per frame, image 3x256x256, BEV 64x64, eager KDStep, k different resident
micro-batches.  One window is `--reps` repetitions of the k calls between two device events, after a device synchronisation and
followed by one (the events see the device timeline of the window, host launch gaps included); windows of i and ii alternate
for `--rounds` rounds after `--warmup` untimed repetitions of each.  Every tree runs in a process of its own, alternating
(parent, this tree, parent, this tree), so the parent's figures bracket this tree's.  The table gives every window in ms per k
calls (k * B frames), the mean and the spread (max - min) per row; the spread of identical windows is the noise figure every
difference has to be read against.
"""
import argparse
import json
import os
import subprocess
import sys

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"
B, K = 64, 4


def child(args):
    root = os.path.abspath(args.tree)
    sys.path[:0] = [os.path.join(root, PKG_NAME), root]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_grad_accum.py needs an MI355X: the product path has no CPU fallback")
    from bench import build_models, synth_batch
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    batches = [synth_batch(B, args.points, 256, 64, 1234 + j, dev) for j in range(K)]

    def build(accum):
        teacher, student = build_models(64, "concat", "weighted")
        teacher, student = teacher.to(dev).eval(), student.to(dev).train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3, **({"accum_steps": K} if accum else {}))
        return KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0), opt

    runs = {"i": build(False)}
    if not args.plain_only:
        runs["ii"] = build(True)

    def window(step, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            for b in batches:
                step(*b)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    rows = {k: [] for k in runs}
    for k, (step, _) in runs.items():
        window(step, args.warmup)
    for _ in range(args.rounds):
        for k, (step, _) in runs.items():
            rows[k].append(window(step, args.reps))
    steps = {k: opt._step for k, (_, opt) in runs.items()}
    print("RESULT " + json.dumps({"rows": rows, "optimiser_steps": steps, "device": torch.cuda.get_device_name(0),
                                  "parameters": runs["i"][1].flat.numel}), flush=True)


def run_child(tree, plain_only, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--rounds", str(args.rounds), "--reps", str(args.reps),
           "--warmup", str(args.warmup), "--points", str(args.points)] + (["--plain-only"] if plain_only else [])
    env = dict(os.environ)
    env.pop("KD_HIP_LIB", None)                    # every tree loads its own library
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if r.returncode != 0:
        raise SystemExit(f"{tree}: the measuring process failed ({r.returncode})\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: adds row iii")
    ap.add_argument("--passes", type=int, default=2, help="processes per tree, alternating")
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=HERE_ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    results = []                                   # (label, result), in the order the processes ran
    for p in range(args.passes):
        if args.parent_tree:
            results.append((f"parent commit, process {p + 1}", run_child(args.parent_tree, True, args)))
        results.append((f"this tree, process {p + 1}", run_child(HERE_ROOT, False, args)))
    dev, npar = results[-1][1]["device"], results[-1][1]["parameters"]
    out = [f"Gradient accumulation: {K} plain KD steps of {B} frames against one accumulating cycle of {K} x {B}; ms per {K} calls ({K * B} frames)",
           f"device: {dev}; concat teacher -> weighted student ({npar} floats in the flat buffer), image 3x256x256, BEV 64x64, "
           f"{args.points} points per frame, eager KDStep",
           f"a window = {args.reps} x {K} calls between two device events; {args.rounds} alternating rounds after {args.warmup} warm-up "
           "repetitions; processes in the order listed", ""]
    w = 9 * args.rounds + 2
    out.append(f"  {'process':<26}{'row':<22}{'ms per window, per round':<{w}}{'mean':>9}{'spread':>9}")
    names = {"i": f"i   {K} plain steps", "ii": f"ii  1 cycle of {K}"}
    means = {}
    for label, res in results:
        for k, v in res["rows"].items():
            m = sum(v) / len(v)
            means.setdefault((label.split(",")[0], k), []).append((m, max(v) - min(v)))
            out.append(f"  {label:<26}{names[k]:<22}{' '.join(f'{x:8.3f}' for x in v):<{w}}{m:>9.3f}{max(v) - min(v):>9.3f}")
        out.append(f"  {'':<26}optimiser steps made: {res['optimiser_steps']}")
    out.append("")
    t_i, t_ii = means[("this tree", "i")], means[("this tree", "ii")]
    for (mi, si), (mii, _) in zip(t_i, t_ii):
        out.append(f"ii - i, same process: {mii - mi:+.3f} ms per {K * B} frames ({(mii / mi - 1) * 100:+.2f} %); spread of i in that process {si:.3f} ms")
    if args.parent_tree:
        p_i = means[("parent commit", "i")]
        pm = [m for m, _ in p_i]
        out.append(f"iii: row i, this tree {', '.join(f'{m:.3f}' for m, _ in t_i)} ms against the parent commit {', '.join(f'{m:.3f}' for m in pm)} ms; "
                   f"the parent's own processes differ by {max(pm) - min(pm):.3f} ms, its windows by up to {max(s for _, s in p_i):.3f} ms")
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
