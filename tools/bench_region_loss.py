#!/usr/bin/env python3
"""The region-loss call (kd_seg_region_loss_fwd_bwd: focal + Tversky + KL) beside the CE call it replaces (kd_seg_loss_fwd_bwd:
CE + KL) at the benchmark's logits, B x NC x 64 x 64, through the C ABI: value + gradient (three launches) and forward only (two).

Each figure is the mean of `--reps` back-to-back calls between two device events, the two entry points alternating over
`--rounds` rounds; the spread (max - min over rounds) is the noise a difference has to be read against.  With `--trace-only` the
calls run untimed, for `rocprofv3 --kernel-trace --stats -- python3 tools/bench_region_loss.py --trace-only`, whose per-kernel
averages give the time of each launch.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"), ROOT]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_loss.py needs an MI355X: the product path has no CPU fallback")
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    B, NC, HW = args.batch, args.classes, 64 * 64
    g = torch.Generator(device="cuda").manual_seed(7)
    zs = torch.randn(B, NC, HW, generator=g, device="cuda") * 3
    zt = torch.randn(B, NC, HW, generator=g, device="cuda") * 3
    y = torch.randint(-1, NC, (B, HW), generator=g, device="cuda")
    cw = torch.tensor([0.4, 3.5, 1.0, 1.0][:NC], device="cuda")
    dzs, vals = torch.empty_like(zs), torch.empty(32, device="cuda")
    nb_ce, nb_rg = lib.kd_seg_loss_ws_bytes(B * HW), lib.kd_seg_region_loss_ws_bytes(B * HW)
    ws = torch.empty(max(nb_ce, nb_rg) // 4, device="cuda")

    def ce(grad):
        lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), -1, 4.0, 1.0, 1.0, None, P(vals), P(dzs) if grad else None, B, NC, HW,
                 P(ws), nb_ce, stream())

    def region(grad):
        lib.call("kd_seg_region_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), -1, 4.0, 1.0, 1.0, None, 2.0, 1.0, 1.0, 0.7, 0.3, 1.0, P(vals),
                 P(dzs) if grad else None, B, NC, HW, P(ws), nb_rg, stream())

    runs = {"CE + KL, value + gradient": lambda: ce(True), "region + KL, value + gradient": lambda: region(True),
            "CE + KL, forward only": lambda: ce(False), "region + KL, forward only": lambda: region(False)}
    for f in runs.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    if args.trace_only:
        for f in runs.values():
            for _ in range(args.reps):
                f()
        torch.cuda.synchronize()
        return
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
    out = [f"segmentation-loss calls at logits {B} x {NC} x 64 x 64 ({B * HW} pixels), teacher logits given, class weights given",
           f"device: {torch.cuda.get_device_name(0)}; us per call, mean of {args.reps} back-to-back calls between two device events (launch "
           "overhead included), entry points alternating", "",
           f"  {'call':<32}{'us/call per round':<{9 * args.rounds + 2}}{'mean':>9}{'spread':>9}"]
    for k, v in rows.items():
        out.append(f"  {k:<32}{' '.join(f'{x:8.2f}' for x in v):<{9 * args.rounds + 2}}{sum(v) / len(v):>9.2f}{max(v) - min(v):>9.2f}")
    text = "\n".join(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
