"""bench.py's contract at a small size: a plain run times exactly --steps steps and prints the headline line only;
`--dump-outputs DIR` writes what the last timed step returned, identically for identical arguments; `--full` adds the
self-check, the roofline, the bf16 modes and the side lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--batch", "4", "--points", "2048"]


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert out["metric"] == "PandaSet 2-class KD training frames/sec" and out["unit"] == "frames/s"
        assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["steps"] == 3 and out["warmup"] == 1
        assert out["ms_per_step"] > 0 and abs(out["value"] - 4 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]
        assert out["checks"]["finite"]
        for k in ("roofline", "cpu_baseline", "bf16_forward", "kd_step_bf16_teacher", "ablation", "small_batch", "comm"):
            assert k not in out, k
        assert out["checks"]["selfcheck"] is None
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert set(arrays) == {"total", "ce", "kl", "mse_cam", "mse_lidar", "logits", "student_state"}, sorted(arrays)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert arrays["logits"].shape[:2] == (4, 2) and arrays["student_state"].size > 4e5
        assert abs(float(arrays["total"]) - out["checks"]["losses_last"]["total"]) <= 1e-5 * max(1.0, abs(float(arrays["total"])))
        runs.append(arrays)
    for k in runs[0]:                 # same arguments -> same inputs and weights -> the same outputs
        np.testing.assert_allclose(runs[1][k], runs[0][k], rtol=1e-5, atol=1e-6, err_msg=k)


def test_full_run_reports_the_extra_measurements():
    out = _bench("--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert out["steps"] == 2 and out["checks"]["selfcheck"]["ok"]
    assert out["roofline"]["launches_per_step"] > 0
    assert out["bf16_forward"]["unit"] == "frames/s" and out["kd_step_bf16_teacher"]["finite"]
    assert set(out["ablation"]) >= {"concat", "minimal", "weighted"} and "B4_hipgraph" in out["small_batch"]
