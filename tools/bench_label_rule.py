#!/usr/bin/env python3
"""Cost of the voting rasteriser (kd_bev_rasterize_vote, majority rule) next to the first-point rasteriser (kd_bev_rasterize) on
the same inputs: 256 sweeps of 169 000 points, grid 64 x 64, 8 classes, class indices as kd_semantic_remap_table writes them.
Three scenes: `uniform` (x, y ~ N(0, 40 m): the reference's recipe), `concentrated` (N(0, 1 m), what `bench.py --points-sigma 1`
makes: every point in a few cells round the sensor, classes in random order) and `concentrated, scan order` (the same positions,
but position and class change only every 16 .. 512 points, as consecutive returns of a real sweep do).

Each figure is the mean of `--reps` back-to-back calls between two device events; the candidates alternate over `--rounds`
rounds and the table gives the median, the smallest and the largest round.  `--compare-lib PATH`: another build of libkd_hip.so
whose kd_bev_rasterize_vote joins the rounds (how the run-merged count pass was compared with one atomic per point); masks and
votes of the two builds must be identical.  Writes profiles/label_rule_ab.txt."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd")]
from kdrt.lib import lib  # noqa: E402
from kdrt.ops import P, stream  # noqa: E402


def scene(kind, B, n, NC, seed):
    r = np.random.RandomState(seed)
    N = B * n
    if kind == "uniform":
        x, y = r.randn(N).astype(np.float32) * 40, r.randn(N).astype(np.float32) * 40
        c = r.randint(0, NC, N)
    elif kind == "concentrated":
        x, y = r.randn(N).astype(np.float32), r.randn(N).astype(np.float32)
        c = r.randint(0, NC, N)
    else:                                                    # concentrated, scan order: runs of 16 .. 512 equal points
        runs = r.randint(16, 513, N // 16 + 1)
        runs = runs[: int(np.searchsorted(np.cumsum(runs), N)) + 1]
        x = np.repeat(r.randn(runs.size).astype(np.float32), runs)[:N]
        y = np.repeat(r.randn(runs.size).astype(np.float32), runs)[:N]
        c = np.repeat(r.randint(0, NC, runs.size), runs)[:N]
    return (torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda(),
            torch.from_numpy(c.astype(np.int64)).cuda())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=256)
    ap.add_argument("--points", type=int, default=169000)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--classes", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--compare-lib", default="")
    ap.add_argument("--compare-name", default="other build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_rule_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_rule.py measures on the MI355X; there is no CPU fallback")
    B, n, G, NC = a.sweeps, a.points, a.grid, a.classes
    other = None
    if a.compare_lib:
        other = ctypes.CDLL(a.compare_lib)
        other.kd_bev_rasterize_vote.restype, other.kd_bev_rasterize_vote.argtypes = lib.protos["kd_bev_rasterize_vote"]
    off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * n
    mask = torch.empty(B, G, G, dtype=torch.int64, device="cuda")
    votes = torch.empty(B, G, G, dtype=torch.int32, device="cuda")
    nb_first, nb_vote = lib.kd_bev_rasterize_ws_bytes(B, G, G), lib.kd_bev_rasterize_vote_ws_bytes(B, G, G, NC)
    ws = torch.empty(max(nb_first, nb_vote), dtype=torch.uint8, device="cuda")
    rng = (-50.0, 100.0, 50.0, -50.0, 100.0, 50.0)
    lines = [f"kd_bev_rasterize_vote (majority, min_points 1, no ranks) against kd_bev_rasterize (first point, remap 0) on one MI355X",
             f"{B} sweeps x {n} points, grid {G} x {G}, {NC} classes; device events, mean of {a.reps} calls per round, {a.rounds} rounds, "
             "candidates alternating; ms per call: median [smallest .. largest round]", ""]
    for kind in ("uniform", "concentrated", "concentrated, scan order"):
        x, y, c = scene(kind, B, n, NC, 7)

        def first():
            lib.call("kd_bev_rasterize", P(x), P(y), P(c), P(off), B, x.numel(), 0, 0, G, G, *rng, P(ws), nb_first, P(mask), stream())

        def vote(fn=lib.kd_bev_rasterize_vote):
            rc = fn(P(x), P(y), P(c), P(off), B, x.numel(), NC, 1, None, 1, G, G, *rng, P(ws), nb_vote, P(mask), P(votes), stream())
            assert rc == 0, rc

        cands = [("kd_bev_rasterize (first point)", first), ("kd_bev_rasterize_vote (majority)", vote)]
        if other is not None:
            cands.append((f"kd_bev_rasterize_vote, {a.compare_name}", lambda: vote(other.kd_bev_rasterize_vote)))
        results = {}
        for name, fn in cands:                              # warm-up; keep the outputs to compare the two builds
            fn()
            torch.cuda.synchronize()
            results[name] = (mask.clone(), votes.clone())
        if other is not None:
            (m0, v0), (m1, v1) = results[cands[1][0]], results[cands[2][0]]
            assert torch.equal(m0, m1) and torch.equal(v0, v1), "the two builds disagree"
        times = {name: [] for name, _ in cands}
        for _ in range(a.rounds):
            for name, fn in cands:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.reps)
        m_vote = results[cands[1][0]][0]
        lines.append(f"{kind}: {int((m_vote != 0).sum())} labelled cells of {m_vote.numel()}, largest vote {int(results[cands[1][0]][1].max())}")
        base = float(np.median(times[cands[0][0]]))
        for name, _ in cands:
            t = np.asarray(times[name])
            lines.append(f"  {name:<48} {np.median(t):8.3f} [{t.min():8.3f} .. {t.max():8.3f}]   x{np.median(t) / base:5.2f} of the first-point call")
        lines.append("")
        del x, y, c
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
