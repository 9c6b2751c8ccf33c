"""tests/_fp64_step_ref.py on the CPU: the helper's first step is _gpu_util.fp64_oracle_grads, its AdamW is torch.optim.AdamW in
float64, and the float32 oracle meets every assertion tests/test_gpu_step_sequence.py makes of the device over the committed
three-step sequences (gross gradient bound and the 1 % cap of left-out elements included)."""
import pytest
import torch

import kd_oracle as O
import _fp64_step_ref as R


@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
@pytest.mark.parametrize("case", R.CASES)
def test_first_step_is_the_single_step_oracle(case, dtype):
    from _gpu_util import FP64_B, FP64_G, FP64_HW, FP64_N, fp64_oracle_grads
    assert (R.B, R.HW, R.N, R.G) == (FP64_B, FP64_HW, FP64_N, FP64_G)
    objective, fusion = case.split("/")
    want = fp64_oracle_grads(fusion, objective, R.SEEDS[0], dtype)
    got = R.oracle_step(objective, fusion, R.student_state(fusion), R.inputs(1), dtype)
    assert set(got["grads"]) == set(want) and len(want) > 75
    for name, g in want.items():
        assert got["grads"][name].dtype == dtype
        assert torch.equal(got["grads"][name].double(), g), name
    assert all(int(v) == 1 for k, v in got["state"].items() if k.endswith("num_batches_tracked"))


def test_adamw64_is_torch_adamw_over_three_steps():
    g = torch.Generator().manual_seed(3)
    shapes = {"a.weight": (5, 3, 1, 1), "a.bias": (5,), "b.weight": (7,)}
    params = {n: torch.randn(s, generator=g, dtype=torch.float64) for n, s in shapes.items()}
    m = {n: torch.zeros_like(p) for n, p in params.items()}
    v = {n: torch.zeros_like(p) for n, p in params.items()}
    tp = [torch.nn.Parameter(p.clone()) for p in params.values()]
    opt = torch.optim.AdamW(tp, lr=R.LR, betas=R.BETAS, eps=1e-8, weight_decay=R.WD)
    for k in (1, 2, 3):
        grads = {n: torch.randn(s, generator=g, dtype=torch.float64) for n, s in shapes.items()}
        before = {n: p.clone() for n, p in params.items()}
        params, m, v = R.adamw64(params, grads, m, v, k)
        assert all(not torch.equal(before[n], params[n]) for n in shapes)
        for p, n in zip(tp, shapes):
            p.grad = grads[n].clone()
        opt.step()
        for p, n in zip(tp, shapes):                      # (torch forms exp_avg with lerp_: the last bits differ)
            assert (p.detach() - params[n]).abs().max().item() <= 1e-13 * max(1.0, params[n].abs().max().item()), (k, n)
            assert (opt.state[p]["exp_avg"] - m[n]).abs().max().item() <= 1e-13, (k, n)
            assert (opt.state[p]["exp_avg_sq"] - v[n]).abs().max().item() <= 1e-13, (k, n)
    # the bias correction of step 2 is 0.19, not step 1's 0.1: a counter stuck at 1 moves the parameters by lr-class amounts
    stuck = R.adamw64(before, grads, {n: torch.zeros_like(p) for n, p in params.items()}, {n: torch.zeros_like(p) for n, p in params.items()}, 1)[0]
    moved = R.adamw64(before, grads, {n: torch.zeros_like(p) for n, p in params.items()}, {n: torch.zeros_like(p) for n, p in params.items()}, 2)[0]
    assert max((stuck[n] - moved[n]).abs().max().item() for n in shapes) > 0.1 * R.LR


def test_bias_in_front_of_batchnorm_names():
    for fusion in ("weighted", "concat", "minimal"):
        st = R.student_state(fusion)
        hits = [k for k in O.trainable_keys(st) if R.bias_in_front_of_batchnorm(k, st)]
        assert hits == [f"lidar_encoder.encoder.point_mlp.{i}.bias" for i in (0, 3, 6)], (fusion, hits)
        hits = [k for k in O.trainable_keys(st) if R.stage_shift_in_front_of_batchnorm(k, st)]
        assert hits == ["camera_encoder.stage1.conv.4.bias"] + [f"camera_encoder.stage{i}.conv.7.bias" for i in (2, 3, 4, 5)], (fusion, hits)


@pytest.mark.parametrize("case", R.CASES)
def test_float32_oracle_meets_the_step_assertions_over_the_sequence(case):
    objective, fusion = case.split("/")
    seen = []
    for k, snap, got in R.host_sequence(objective, fusion, torch.float32):
        R.check_step(got, snap, k, objective, fusion, tag=f"{case} step {k} (float32 CPU oracle)")
        assert not torch.equal(got["state"]["head.cls.weight"], snap["state"]["head.cls.weight"])      # the parameters moved
        seen.append(k)
    assert seen == [1, 2, 3]
