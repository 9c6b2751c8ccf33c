#!/usr/bin/env python3
"""The cost of the intra-class feature variation distillation feature term (kd_feat_ifv_fwd_bwd, csrc/kd_loss_ifv.hip), same box, one
process.

  calls : the call alone through the C ABI on one feature map [B * HW, C] (default 256 x 4096 x 128: 537 MB per map) under a label
          map of `--classes` classes (a tenth of the pixels ignored), value + gradient (seven launches: 4 sweeps of S, 2 of T, one
          store) and forward only (five: 2 sweeps of each map), with 2 and with 16 classes, beside kd_mse_partial over the same map
          (the feature MSE of the default objective: the baseline, 3 sweeps).  Each row carries the bytes its sweeps move and the
          TB/s that implies.
  steps : the eager KD step at the benchmarked frame shape (B frames, 80 000 points, image 3x256x256, BEV 64x64, two classes) with
          feature_loss = None (the feature MSE: the calls of the parent commit) twice, with PairKD() and with IntraClassKD(); the
          figures to read are the added ms per step over the MSE step, against the difference of the two identical MSE rows

A call figure is the mean of `--reps` back-to-back calls between two device events; a step window is `--step-reps` steps between
two device events after a device synchronisation.  Rows alternate over `--rounds` rounds; the spread (max - min over rounds) of a
row is the noise a difference has to be read against.  With `--trace-only` the calls run untimed for
`rocprofv3 --kernel-trace --stats -- python3 tools/bench_ifv_loss.py --trace-only`.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402


def table(title, rows, rounds, unit, extra=None):
    out = [title, f"  {'row':<44}{unit + ' per round':<{10 * rounds + 2}}{'mean':>10}{'spread':>9}" + ("      GB    TB/s" if extra else "")]
    for k, v in rows.items():
        mean = sum(v) / len(v)
        line = f"  {k:<44}{' '.join(f'{x:9.3f}' for x in v):<{10 * rounds + 2}}{mean:>10.3f}{max(v) - min(v):>9.3f}"
        if extra:
            nbytes = extra[k]
            line += f"{nbytes / 1e9:>8.2f}{nbytes / (mean * 1e-6) / 1e12:>8.2f}"
        out.append(line)
    return out


def bench_calls(args):
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    B, HW, C = args.batch, args.hw, args.channels
    n = B * HW * C
    g = torch.Generator(device="cuda").manual_seed(7)
    s = torch.randn(B * HW, C, generator=g, device="cuda").clamp_min_(0)          # post-ReLU maps, as the fusion block's are
    t = (s * 0.7 + torch.randn(B * HW, C, generator=g, device="cuda") * 0.6).clamp_min_(0)
    ds, val = torch.empty_like(s), torch.empty(4, device="cuda")
    slab = torch.empty(lib.kd_mse_slab_blocks(n), device="cuda")
    classes = sorted({2, args.classes})
    ys = {nc: torch.randint(0, nc, (B, HW), generator=g, device="cuda") for nc in classes}
    for y in ys.values():
        y[torch.rand(B, HW, generator=g, device="cuda") < 0.1] = -1
    nb = max(lib.kd_feat_ifv_ws_bytes(B, HW, C, C, nc) for nc in classes)
    ws = torch.empty(nb // 4 + 4, device="cuda")

    def mse(grad):
        lib.call("kd_mse_partial", P(s), P(t), n, 2.0 / n, P(ds) if grad else None, P(slab), stream())

    def ifv(grad, nc):
        lib.call("kd_feat_ifv_fwd_bwd", P(s), P(t), P(ys[nc]), -1, B, HW, C, C, nc, 2.0 / B, None, P(val), P(ds) if grad else None, None, P(ws),
                 nb, stream())

    runs = {"MSE (kd_mse_partial), value + gradient": lambda: mse(True)}
    sweeps = [3]
    for nc in classes:
        runs[f"IFV, {nc} classes, value + gradient"] = lambda nc=nc: ifv(True, nc)
        sweeps.append(7)
    runs["MSE (kd_mse_partial), forward only"] = lambda: mse(False)
    sweeps.append(2)
    for nc in classes:
        runs[f"IFV, {nc} classes, forward only"] = lambda nc=nc: ifv(False, nc)
        sweeps.append(4)
    nbytes = dict(zip(runs, (4.0 * n * k for k in sweeps)))
    for f in runs.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    if args.trace_only:
        for f in runs.values():
            for _ in range(args.reps):
                f()
        torch.cuda.synchronize()
        return []
    rows = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            rows[k].append(e0.elapsed_time(e1) / args.reps * 1e3)
    out = table(f"feature-loss calls on one map [{B} x {HW}, {C}] fp32 ({n * 4 / 1e6:.0f} MB); us per call, mean of {args.reps} back-to-back "
                f"calls (launch overhead included); slices per image {lib.kd_feat_ifv_slices(B, HW)}; GB = the map sweeps of the call",
                rows, args.rounds, "us/call", nbytes)
    mean = {k: sum(v) / len(v) for k, v in rows.items()}
    keys = list(rows)
    out += ["", f"IFV ({classes[0]} classes) / MSE, value + gradient: {mean[keys[1]] / mean[keys[0]]:.2f} x (the sweep counts predict "
                f"{7 / 3:.2f} x: 7 against 3)", ""]
    return out


def bench_steps(args):
    from bench import build_models, synth_batch
    from kdrt.kd import KDStep
    from kdrt.losses import IntraClassKD, PairKD
    from kdrt.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    B = args.batch
    batch = synth_batch(B, args.points, 256, 64, 1234, dev)

    def build(feature_loss):
        teacher, student = build_models(64, "concat", "weighted")
        teacher, student = teacher.to(dev).eval(), student.to(dev).train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        return KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0, feature_loss=feature_loss)

    steps = {"i   feature MSE (the parent commit's calls)": build(None), "ii  PairKD()": build(PairKD()),
             "iii IntraClassKD()": build(IntraClassKD()), "iv  feature MSE again (same as i)": build(None)}
    for s in steps.values():
        for _ in range(args.step_warmup):
            s(*batch)
    rows = {k: [] for k in steps}
    for _ in range(args.rounds):
        for k, s in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.step_reps):
                s(*batch)
            e1.record()
            torch.cuda.synchronize()
            rows[k].append(e0.elapsed_time(e1) / args.step_reps)
    out = table(f"eager KD step, concat teacher -> weighted student, {B} frames x {args.points} points, image 3x256x256, BEV 64x64, feature "
                f"maps {B} x 128 x 64 x 64, 2 classes; ms per step, windows of {args.step_reps} steps", rows, args.rounds, "ms/step")
    mean = {k: sum(v) / len(v) for k, v in rows.items()}
    keys = list(rows)
    spread = max(max(rows[keys[0]]) - min(rows[keys[0]]), max(rows[keys[3]]) - min(rows[keys[3]]))
    out += ["", f"ii - i  : {mean[keys[1]] - mean[keys[0]]:+.3f} ms per step (pair-wise distillation over the MSE step)",
            f"iii - i : {mean[keys[2]] - mean[keys[0]]:+.3f} ms per step (intra-class feature variation distillation over the MSE step)",
            f"iv - i  : {mean[keys[3]] - mean[keys[0]]:+.3f} ms per step (two identical MSE steps); largest spread of the windows of i and iv "
            f"{spread:.3f} ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=4096)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--step-reps", type=int, default=8)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ifv_loss.py needs an MI355X: the product path has no CPU fallback")
    out = [f"Intra-class feature variation distillation feature term (kd_feat_ifv_fwd_bwd); device: {torch.cuda.get_device_name(0)}",
           "command: python tools/bench_ifv_loss.py --out profiles/ifv_kd_ab.txt", ""]
    out += bench_calls(args)
    if not (args.no_steps or args.trace_only):
        out += bench_steps(args)
    text = "\n".join(out)
    print(text, flush=True)
    if args.out and not args.trace_only:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
