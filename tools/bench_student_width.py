#!/usr/bin/env python3
"""Dev tool: one KD step (or one student eval forward) at the bench shape for a student of width b.

The bench workload of bench.py -- 256 frames, 256 x 256 images, 80 000 points per frame, 64 x 64 BEV grid, a concat teacher
at base_channels 32 -- with a weighted student whose TwinLiteEncoder has base_channels = b.  Timed with HIP events around
`--steps` calls after `--warmup` calls (bench.py's counts).  One configuration per process, so that each can run under its
own time limit; prints one JSON line.

usage: bench_student_width.py --b 16 [--mode kd|eval_fp32|eval_bf16] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"))
sys.path.insert(0, ROOT)


def build(fusion, oc, grid, b):
    from src.models.camera_encoder import TwinLiteEncoder
    from src.models.fusion_module import CompleteSegmentationModel
    from src.models.lidar_encoder import LiDAREncoder
    return CompleteSegmentationModel(TwinLiteEncoder(base_channels=b, return_multiscale=True),
                                     LiDAREncoder(encoder_type="spatial", grid_size=(grid, grid)), num_classes=2, fusion_type=fusion,
                                     fusion_out_channels=oc, camera_fpn_stages=["stage3", "stage4", "stage5"], camera_fpn_channels=128,
                                     output_mode="same")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, required=True, help="student base_channels")
    ap.add_argument("--mode", choices=("kd", "eval_fp32", "eval_bf16"), default="kd")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--points", type=int, default=80000)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_student_width.py measures on the GPU; no device found")
    from bench import synth_batch
    from kdrt.bf16 import forward_bf16
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    teacher = build("concat", 256, args.grid, 32).to(dev).eval()
    student = build("weighted", 128, args.grid, args.b).to(dev)
    images, pts, labels = synth_batch(args.batch, args.points, args.image, args.grid, 1234, dev)
    if args.mode == "kd":
        student.train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5], device=dev), T=4.0, alpha=1.0, beta=1.0)
        run = lambda: step(images, pts, labels)["total"]
    elif args.mode == "eval_fp32":
        student.eval()

        def run():
            with torch.no_grad():
                return student(images, pts)
    else:
        student.eval()
        run = lambda: forward_bf16(student, images, pts)
    for _ in range(args.warmup):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.steps
    n_cam = sum(p.numel() for p in student.camera_encoder.parameters())
    print(json.dumps({"mode": args.mode, "student_base_channels": args.b, "ms_per_step": round(ms, 3),
                      "frames_per_s": round(args.batch / ms * 1e3, 1), "steps": args.steps, "warmup": args.warmup,
                      "student_params": sum(p.numel() for p in student.parameters()), "student_camera_encoder_params": n_cam,
                      "finite": bool(torch.isfinite(out).all().item()),
                      "shape": f"B={args.batch} {args.image}x{args.image} N={args.points} grid={args.grid}, concat b=32 teacher"}))


if __name__ == "__main__":
    main()
