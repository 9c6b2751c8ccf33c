#!/usr/bin/env python3
"""Dev tool: the stage-2 expand layer's backward (32 -> 192 at 128 x 128) at the benchmarked size (256 frames) -- kd_pwconv_bwd (data +
weight gradient in one launch) against kd_pwconv_wgrad + kd_pwconv_gemm(pro 2, epi 0) on the same buffers, in one process, alternating,
warmed, HIP-event timed.  usage: bench_pw_bwd.py [frames] [rounds]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd"))
import torch
from kdrt import ops
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 6
N, K = 192, 32
M = B * 128 * 128
g = torch.Generator(device="cuda").manual_seed(1)
v = lambda n: torch.rand(n, device="cuda", generator=g) + 0.5
D, X, A = torch.randn(M, N, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g), torch.randn(M, K, device="cuda", generator=g)
Wt = torch.randn(K, N, device="cuda", generator=g) / N ** 0.5
al, be, ga, msc, msh = v(N), v(N) * 0.1, v(N) * 0.1, v(N), v(N) - 1.0
out = {f: (torch.empty(N, K, device="cuda"), torch.empty(M, K, device="cuda")) for f in ("two", "one")}
kw = dict(M=M, N=N, K=K, X=X, d_mode=2, d_act=2, al=al, be=be, ga=ga, msc=msc, msh=msh)


def two():
    dW, dX = out["two"]
    ops.pw_wgrad(D, A, dW, **kw)
    ops.pw_gemm(D, Wt, dX, M=M, K=N, N=K, A2=X, pro=2, pro_act=2, p=(al, be, ga, msc, msh), epi=0)


def one():
    dW, dX = out["one"]
    ops.pw_bwd(D, A, Wt, dX, dW, **kw)


assert ops.lib.kd_pwconv_bwd_supported(N, K, 2, 0, 0) == 1
for f in (two, one, two, one):
    f()
times = {"two": [], "one": []}
for _ in range(ROUNDS):
    for name, f in (("two", two), ("one", one)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            f()
        e1.record(); torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / 5 * 1e3)
by2 = 4.0 * (2 * (2 * M * N) + 2 * M * K)          # two launches: (D, X) twice, A in, dX out
by1 = 4.0 * (2 * M * N + 2 * M * K)                # one launch: (D, X) once
med = lambda a: sorted(a)[len(a) // 2]
t2, t1 = med(times["two"]), med(times["one"])
same = [bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(out["two"], out["one"])]
print(f"  stage2 expand backward 32->192 @128^2, {B} frames, M={M}")
print(f"  kd_pwconv_wgrad + kd_pwconv_gemm : {' '.join(f'{t:7.1f}' for t in times['two'])} us   median {t2:7.1f} us  {by2 / t2 / 1e6:5.2f} TB/s of {by2 / 1e9:.2f} GB")
print(f"  kd_pwconv_bwd (one launch)       : {' '.join(f'{t:7.1f}' for t in times['one'])} us   median {t1:7.1f} us  {by1 / t1 / 1e6:5.2f} TB/s of {by1 / 1e9:.2f} GB")
print(f"  x{t2 / t1:4.2f}; dW bitwise equal: {same[0]}, dX bitwise equal: {same[1]}")
