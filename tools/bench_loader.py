#!/usr/bin/env python3
"""KD step fed by DeviceBatchLoader over SyntheticRawPandaSet, next to the same step over a batch resident in HBM.

What is timed: everything between two steps that a real run pays after decode -- packing the raw frames of a batch,
host-to-device copies, rasteriser / point / image preparation -- at prefetch = 0 (synchronous, the per-frame path) and
with batches prepared ahead on a side stream (prefetch >= 1).  What is NOT timed: JPEG decode and unpickling (the raw
frames are generated once and served from memory, num_workers = 0).

Per shape and prefetch depth: ms/step loader-fed, ms/step resident (same process, same models), the exposed preparation
time per step = their difference, and beside it the compute stream's idle gap between two steps measured with HIP events
recorded on it around the loader's `next()` (before: after the last kernel of the previous step; after: once the batch
is usable).  The rounds alternate the configurations; the spread over rounds is the table's own noise figure.

  ref   : B = 4,   169 000-point sweeps, max_points = 5 000   (the reference's own shape)
  bench : B = 256, 169 000-point sweeps, max_points = 80 000  (the benchmarked shape; weighted student, concat teacher)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402

SHAPES = {"ref": (4, 169000, 5000), "bench": (256, 169000, 80000)}


def run_shape(name, args, out):
    from bench import build_models
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, SyntheticRawPandaSet
    B, sweep, max_points = SHAPES[name]
    dev = torch.device("cuda", 0)
    teacher, student = build_models(64, "concat", "weighted")
    teacher, student = teacher.to(dev).eval(), student.to(dev).train()
    opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
    step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0)
    n_batches = args.warmup + args.steps
    ds = SyntheticRawPandaSet(n_frames=B * n_batches, sweep_points=sweep, max_points=max_points, unique=min(B, 64), seed=1)
    for u in range(ds.unique):
        ds.load_raw(u)                                                       # generate once, outside every timed window

    def resident():
        b = next(iter(DeviceBatchLoader(ds, B, shuffle=False, num_workers=0, prefetch=0)))
        im, pt, sg = b["image"], b["points"], b["segmentation"]
        for _ in range(args.warmup):
            step(im, pt, sg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(im, pt, sg)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    def fed(prefetch):
        loader = DeviceBatchLoader(ds, B, shuffle=False, num_workers=0, prefetch=prefetch, sample_seed=1)
        it, gaps, t0, t_host = iter(loader), [], None, 0.0
        for k in range(n_batches):
            if k == args.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h0 = time.perf_counter()
            b = next(it)
            h1 = time.perf_counter()
            e1.record()
            step(b["image"], b["points"], b["segmentation"])
            if k >= args.warmup:
                gaps.append((e0, e1))
                t_host += h1 - h0
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        gap = sum(a.elapsed_time(b) for a, b in gaps) / len(gaps)
        del it
        return ms, gap, t_host / args.steps * 1e3

    rows = {}
    for rnd in range(args.rounds):
        rows.setdefault("resident", []).append((resident(), 0.0, 0.0))
        for p in args.prefetch:
            rows.setdefault(f"prefetch={p}", []).append(fed(p))
    res = [r[0] for r in rows["resident"]]
    res_ms = sum(res) / len(res)
    out.append(f"shape {name}: B = {B}, {sweep}-point sweeps, max_points = {max_points}; {args.steps} timed steps after {args.warmup} "
               f"warm-up, {args.rounds} alternating rounds (figures per round, then mean)")
    out.append(f"  {'configuration':<14}{'ms/step':>34}{'exposed = fed - resident':>28}{'stream gap (HIP events)':>34}{'host ms in next()':>28}")
    fmt = lambda vs: " ".join(f"{v:9.2f}" for v in vs) + f" |{sum(vs) / len(vs):9.2f}"
    out.append(f"  {'resident':<14}{fmt(res):>34}")
    for p in args.prefetch:
        r = rows[f"prefetch={p}"]
        out.append(f"  {'prefetch=' + str(p):<14}{fmt([v[0] for v in r]):>34}{fmt([v[0] - res_ms for v in r]):>28}"
                   f"{fmt([v[1] for v in r]):>34}{fmt([v[2] for v in r]):>28}")
    out.append("")
    del step, opt, teacher, student
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="ref,bench")
    ap.add_argument("--prefetch", default="0,1,2", help="comma-separated prefetch depths; 0 = the synchronous path")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    args.prefetch = [int(v) for v in args.prefetch.split(",")]
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py needs an MI355X: the product path has no CPU fallback")
    out = ["KD step fed by DeviceBatchLoader over SyntheticRawPandaSet (decode and unpickle excluded: raw frames served from memory)",
           f"device: {torch.cuda.get_device_name(0)}; concat teacher -> weighted student, image 3x256x256, BEV 64x64; times in ms", ""]
    for name in args.shapes.split(","):
        run_shape(name, args, out)
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
