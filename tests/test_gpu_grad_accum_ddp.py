"""Gradient accumulation under data parallelism, on ONE MI355X: one set of collectives per optimiser step, not per micro-batch.

A world of one rank over RCCL with the reducer forced (the setting of tests/test_gpu_rccl_world1.py): bit-identical to the
reducer-less accumulating step, three collectives per cycle of two micro-batches, buckets folded and launched head -> fusion/FPN/
LiDAR -> camera on the last micro-batch, nothing on the first.  Two ranks on the one GPU over gloo (the setting of
tests/test_gpu_ddp_one_gpu.py): the folded and reduced buffer is exactly (g_00 + g_01) + (g_10 + g_11), the parameters a plain
AdamW step on it with grad_scale = 1/4, BatchNorm statistics per rank.  Every child runs under its own timeout."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "lightweight-multi-modal-scene-understanding-via-knowledge-distillation_amd")


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world_of_one_with_a_forced_reducer(tmp_path):
    out = tmp_path / "res.json"
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_port()),
               KD_ACCUM_OUT=str(out), OMP_NUM_THREADS="2")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_grad_accum_world1_worker.py")], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["backend"] == "nccl" and res["world"] == 1 and res["ranks_seen"] == 1
    assert res["stepped"] == [False, True, False, True] == res["stepped_plain"] and res["steps"] == 2
    assert res["bit_identical_cycles"] == [True, True], res        # parameters, folded gradients, Adam moments, accum, BN buffers
    assert res["accum_zero"] == [True, True] and res["moved"]
    assert res["collectives"] == [0, 3, 3, 6], res                  # 3 per cycle, not 6: nothing on the first micro-batch
    assert res["orders"] == [[], [2, 1, 0], [], [2, 1, 0]], res["orders"]
    spans = res["spans"]
    assert res["folds"] == [[], spans[::-1], [], spans[::-1]], res["folds"]      # each bucket's slice once, right before its launch
    assert res["grad_scale"] == 0.5


def test_two_ranks_reduce_the_folded_buckets_once_per_cycle(tmp_path):
    e = dict(os.environ, KD_ACCUM_OUT=str(tmp_path), KD_REHEARSE_ON_ONE_GPU="1", OMP_NUM_THREADS="2")
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    e["PYTHONPATH"] = PKG + os.pathsep + e.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), os.path.join(HERE, "_grad_accum_ddp_worker.py")]
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for rank in range(2):
        res = json.load(open(tmp_path / f"rank{rank}.json"))
        print(json.dumps(res))
        assert res["stepped"] == [False, True] and res["steps"] == 1
        assert res["orders"] == [[], [2, 1, 0]] and res["collectives"] == [0, 3], res
        assert res["reduced_equals_sum"] and res["not_own_only"], res          # (g_00 + g_01) + (g_10 + g_11), exactly
        assert res["grad_scale"] == 0.25 and res["params_equal"] and res["moments_equal"], res
        assert res["accum_zero"] and res["ranks_agree"], res
        assert res["bn_own"] == 0.0 and res["bn_other"] > 0.0, res             # BatchNorm statistics stay per rank
