#!/usr/bin/env python3
"""The cost of the OHEM cross-entropy (kd_seg_ohem_fwd_bwd, csrc/kd_loss_ohem.hip), same box, one process.

  calls : the loss call alone through the C ABI at logits B x NC x 64 x 64 (the benchmarked label shape), value + gradient (seven
          launches) and forward only (six), beside the CE call (kd_seg_loss_fwd_bwd, three / two launches) whose place it takes in the
          step; both with the KL term
  steps : the eager KD step at the benchmarked frame shape (B frames, 80 000 points, image 3x256x256, BEV 64x64) with
          hard_loss = None (the weighted CE: the calls of the parent commit) and hard_loss = OhemCE(); the figure to read is the
          added ms per step over the CE step

A call figure is the mean of `--reps` back-to-back calls between two device events; a step window is `--step-reps` steps between
two device events after a device synchronisation.  Rows alternate over `--rounds` rounds; the spread (max - min over rounds) of a
row is the noise a difference has to be read against.  With `--trace-only` the calls run untimed for
`rocprofv3 --kernel-trace --stats -- python3 tools/bench_ohem_loss.py --trace-only`.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402


def table(title, rows, rounds, unit):
    out = [title, f"  {'row':<40}{unit + ' per round':<{10 * rounds + 2}}{'mean':>10}{'spread':>9}"]
    for k, v in rows.items():
        out.append(f"  {k:<40}{' '.join(f'{x:9.3f}' for x in v):<{10 * rounds + 2}}{sum(v) / len(v):>10.3f}{max(v) - min(v):>9.3f}")
    return out


def bench_calls(args):
    from kdrt.lib import lib
    from kdrt.losses import OhemCE
    from kdrt.ops import P, stream
    B, NC, side = args.batch, args.classes, 64
    HW = side * side
    spec = OhemCE()
    g = torch.Generator(device="cuda").manual_seed(7)
    zs = torch.randn(B, NC, HW, generator=g, device="cuda") * 3
    zt = torch.randn(B, NC, HW, generator=g, device="cuda") * 3
    y = torch.randint(-1, NC, (B, HW), generator=g, device="cuda")
    cw = torch.tensor(([0.4, 3.5] + [1.0] * 14)[:NC], device="cuda")
    dzs, vals = torch.zeros_like(zs), torch.empty(32, device="cuda")
    nb_ce, nb_oh = lib.kd_seg_loss_ws_bytes(B * HW), lib.kd_seg_ohem_ws_bytes(B * HW)
    ws = torch.empty(max(nb_ce, nb_oh) // 4 + 2, device="cuda")

    def ce(grad):
        lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), -1, 4.0, 1.0, 1.0, None, P(vals), P(dzs) if grad else None, B, NC, HW,
                 P(ws), nb_ce, stream())

    def ohem(grad):
        lib.call("kd_seg_ohem_fwd_bwd", P(zs), P(zt), P(y), P(cw), -1, 4.0, 1.0, 1.0, None, spec.lam(), spec.min_kept, spec.min_divisor,
                 P(vals), None, P(dzs) if grad else None, None, None, B, NC, HW, P(ws), nb_oh, stream())

    runs = {"CE + KL, value + gradient": lambda: ce(True), "OHEM + KL, value + gradient": lambda: ohem(True),
            "CE + KL, forward only": lambda: ce(False), "OHEM + KL, forward only": lambda: ohem(False)}
    for f in runs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    if args.trace_only:
        for f in runs.values():
            for _ in range(args.reps):
                f()
        torch.cuda.synchronize()
        return []
    ohem(False)
    torch.cuda.synchronize()
    kept = vals[5].item()
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
    return table(f"loss calls at logits {B} x {NC} x {side} x {side} ({B * HW} keys, {kept * 100:.1f} % kept by {spec}); us per call, mean of "
                 f"{args.reps} back-to-back calls (launch overhead included)", rows, args.rounds, "us/call") + [""]


def bench_steps(args):
    from bench import build_models, synth_batch
    from kdrt.kd import KDStep
    from kdrt.losses import OhemCE
    from kdrt.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    B = args.batch
    batch = synth_batch(B, args.points, 256, 64, 1234, dev)

    def build(hard_loss):
        teacher, student = build_models(64, "concat", "weighted")
        teacher, student = teacher.to(dev).eval(), student.to(dev).train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        return KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0, hard_loss=hard_loss)

    steps = {"i   CE (the parent commit's calls)": build(None), "ii  OhemCE()": build(OhemCE())}
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
    out = table(f"eager KD step, concat teacher -> weighted student, {B} frames x {args.points} points, image 3x256x256, BEV 64x64, logits "
                f"{B} x 2 x 64 x 64; ms per step, windows of {args.step_reps} steps", rows, args.rounds, "ms/step")
    mean = {k: sum(v) / len(v) for k, v in rows.items()}
    keys = list(rows)
    out += ["", f"ii - i : {mean[keys[1]] - mean[keys[0]]:+.3f} ms per step (OhemCE() over the CE step); spread of i "
                f"{max(rows[keys[0]]) - min(rows[keys[0]]):.3f} ms, of ii {max(rows[keys[1]]) - min(rows[keys[1]]):.3f} ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--step-reps", type=int, default=8)
    ap.add_argument("--step-warmup", type=int, default=3)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ohem_loss.py needs an MI355X: the product path has no CPU fallback")
    out = [f"OHEM cross-entropy (kd_seg_ohem_fwd_bwd); device: {torch.cuda.get_device_name(0)}",
           "command: python tools/bench_ohem_loss.py --out profiles/ohem_loss_ab.txt", ""]
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
