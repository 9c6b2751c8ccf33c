"""One training step of the CPU oracle (oracle/kd_oracle.py) started from a GIVEN state -- the device's own, copied before step k
-- in float64 or float32, and the assertions tests/test_gpu_step_sequence.py makes at every step of a sequence.

Re-seeding the oracle from the device state at every step keeps rounding from compounding: the comparison at step k is as
tight as at step 1 and no chaotic divergence of two trajectories enters it.  The same assertions run on the CPU in
tests/test_fp64_step_ref_host.py, with the float32 oracle in the device's place."""
import re
import struct

import torch

import kd_oracle as O
from _util import state_template

B, HW, N, G = 2, 64, 512, 16                  # _gpu_util.FP64_*: the smallest shapes at which every unit of the model still runs
PAD_TAIL = 40
CW = (0.4, 3.5)
SEEDS = (1, 2, 5)                             # the batch of step k is O.make_inputs seed SEEDS[k - 1]: a different one per step
K = len(SEEDS)
LR, WD = 1e-2, 1e-3                           # lr 1e-2: every parameter visibly moves at every step
T, ALPHA, BETA = 4.0, 1.0, 1.0
# The betas of the float64 AdamW are the ones the device HAS: the C ABI takes them as float, so beta2 is float32(0.999) =
# 0.99900001287..., and the kernels form 1 - beta2 from that value -- an exact AdamW for that beta2 (gain and decay sum to 1, the
# bias correction is 1 - beta2^k of the same number), as tests/_fp64_loss_ref.py and tests/test_gpu_grad_clip.py already model it.
# Against beta2 = 0.999 as a double, 1 - beta2 differs by 1.3e-5 relative and so does every exp_avg_sq (measured on the device at
# step 1, kd/weighted: |d| 6.7e-9 of a largest magnitude 5.2e-4, 13 times the bound below); parameters move by 6e-8 at most.
BETAS = (struct.unpack("f", struct.pack("f", 0.9))[0], struct.unpack("f", struct.pack("f", 0.999))[0])
STUDENT_SEED, TEACHER_SEED = 12, 11
CASES = ("kd/weighted", "kd/concat", "kd/minimal", "ce/concat")

# absolute tolerances of tests/test_gpu_parity.py::test_kd_step_vs_oracle_and_adamw (parts 1e-4, total 2e-4) and its LOGIT_TOL
PART_TOL, TOTAL_TOL, LOGIT_TOL = 1e-4, 2e-4, 1e-4
BN_RTOL = 1e-4                                # test_train_step_vs_oracle: 1e-4 * max(1, |v|max)
PARAM_RTOL, MOMENT_RTOL, TINY_GRAD = 2e-6, 1e-6, 1e-6
LEFT_OUT_CAP = 0.01                           # share of the elements with |g| < TINY_GRAD (CPU oracle: 0.17 %)
GROSS_GRAD_TOL = 8e-2                         # _gpu_util.grads_match's gross bound: a wiring error can never hide


def inputs(k):
    """the batch of step k (1-based)"""
    return O.make_inputs(B, HW, N, G, SEEDS[k - 1], pad_tail=PAD_TAIL)


def student_state(fusion):
    return O.randomize_state(state_template(fusion), STUDENT_SEED)


def teacher_state():
    return O.randomize_state(state_template("concat"), TEACHER_SEED)


def build_model(fusion, num_classes=2, base=32, grid=None):
    """the product model of the step tests on the CPU: TwinLite camera encoder of width `base`, spatial LiDAR encoder on a
    grid x grid BEV (default G), FPN over stages 3 - 5, same-resolution head"""
    from src.models.camera_encoder import TwinLiteEncoder
    from src.models.fusion_module import CompleteSegmentationModel
    from src.models.lidar_encoder import LiDAREncoder
    from _gpu_util import FUSIONS
    cam = TwinLiteEncoder(base_channels=base, return_multiscale=True)
    lid = LiDAREncoder(encoder_type="spatial", grid_size=(grid or G, grid or G), use_vectorized=True)
    return CompleteSegmentationModel(cam, lid, num_classes=num_classes, fusion_type=fusion, fusion_out_channels=FUSIONS[fusion],
                                     camera_fpn_stages=["stage3", "stage4", "stage5"], camera_fpn_channels=128, output_mode="same")


def random_state(model, seed):
    """kd_oracle.randomize_state over the model's own names and shapes (the recipe of _gpu_util.load_random_state)"""
    sd = model.state_dict()
    st = O.randomize_state({k: v.detach().cpu().clone() for k, v in sd.items()}, seed)
    for k, v in sd.items():
        if k.endswith("grid_tensor"):
            st[k] = v.detach().cpu().clone()
    return st


def _cast(st, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in st.items()}


def oracle_step(objective, fusion, state, batch, dtype, t_state=None, kd_objective=None, cw=CW, grid=G):
    """Forward, loss and backward of one step from `state` (a name-keyed CPU state_dict; not modified) in `dtype`.
    -> {"parts": {name: float}, "logits", "grads": {name: tensor}, "state": the state after the forward pass (BatchNorm running
    statistics and num_batches_tracked updated)}.  The same calls in the same order as _gpu_util.fp64_oracle_grads.
    kd_objective: a callable with kd_oracle.kd_loss's signature in its place (tests/_fp64_objective_ref.step_objective: the KD
    objective under a hard_loss / feature_loss option); cw, grid: the class weights and the BEV grid of a case that has its own."""
    images, pts, labels = batch
    cw = torch.tensor(cw)
    s = O.clone_state(_cast(state, dtype), requires_grad=True)
    zs, ms = O.complete_model(images.to(dtype), pts.to(dtype), s, fusion_type=fusion, grid=(grid, grid), training=True)
    if objective == "kd":
        t = _cast(teacher_state() if t_state is None else t_state, dtype)
        with torch.no_grad():
            zt, mt = O.complete_model(images.to(dtype), pts.to(dtype), t, fusion_type="concat", grid=(grid, grid), training=False)
        total, parts = (O.kd_loss if kd_objective is None else kd_objective)(zs, ms, zt, mt, labels, cw.to(dtype), T, ALPHA, BETA)
        parts = {k: v.item() for k, v in parts.items()}
    else:
        total, parts = O.weighted_ce(zs, labels, cw.to(dtype)), {}
    total.backward()
    parts["total"] = total.item()
    return {"parts": parts, "logits": zs.detach(), "grads": {k: v.grad for k, v in s.items() if v.grad is not None},
            "state": {k: v.detach() for k, v in s.items()}}


def adamw64(params, grads, exp_avg, exp_avg_sq, k, lr=LR, weight_decay=WD):
    """float64 AdamW at step k on {name: tensor} dictionaries (not modified) -> (params, exp_avg, exp_avg_sq) after it"""
    keys = list(params)
    p, m, v = ([d[n].detach().double().cpu().clone() for n in keys] for d in (params, exp_avg, exp_avg_sq))
    O.adamw_step(p, [grads[n].detach().double().cpu() for n in keys], m, v, step=k, lr=lr, betas=BETAS, weight_decay=weight_decay)
    return tuple(dict(zip(keys, x)) for x in (p, m, v))


# ---- the assertions of a step -----------------------------------------------------------------------------------------------------

def _d(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def check_losses_and_logits(got_parts, got_logits, ref64, ref32, tag=""):
    """every loss part, the total and the logits within max(T, 3 * d_cpu) of float64, d_cpu the float32 CPU oracle's own distance"""
    for name, want in ref64["parts"].items():
        tol = max(TOTAL_TOL if name == "total" else PART_TOL, 3 * abs(ref32["parts"][name] - want))
        d = abs(float(got_parts[name]) - want)
        print(f"{tag} {name}: {float(got_parts[name]):.9g} float64 {want:.9g} |d| {d:.3g} tol {tol:.3g}")
        assert d <= tol, (tag, name, d, tol)
    tol = max(LOGIT_TOL, 3 * _d(ref32["logits"], ref64["logits"]))
    d = _d(got_logits, ref64["logits"])
    print(f"{tag} logits: |d| {d:.3g} tol {tol:.3g}")
    assert d <= tol, (tag, "logits", d, tol)


def check_bn_buffers(got_state, ref64, k, tag=""):
    n = 0
    for name, want in ref64["state"].items():
        if name.endswith(("running_mean", "running_var")):
            d = _d(got_state[name], want)
            assert d <= BN_RTOL * max(1.0, want.abs().max().item()), (tag, name, d)
            n += 1
        elif name.endswith("num_batches_tracked"):
            assert int(got_state[name]) == int(want) == k, (tag, name, int(got_state[name]), int(want), k)
            n += 1
    assert n >= 75 and n % 3 == 0, n          # every BatchNorm of the model: mean, variance and counter (29 in the weighted student)


def bias_in_front_of_batchnorm(name, state):
    """a conv bias whose output goes straight into a BatchNorm (train mode: the true gradient is 0, both sides hold rounding noise)"""
    head, _, leaf = name.rpartition(".")
    parent, _, idx = head.rpartition(".")
    return (leaf == "bias" and idx.isdigit() and state[head + ".weight"].dim() > 1
            and f"{parent}.{int(idx) + 1}.running_mean" in state)


def stage_shift_in_front_of_batchnorm(name, state):
    """The bias of the LAST BatchNorm of a camera stage.  The stage's output has no activation and no skip connection, and every
    consumer (the next stage's expand convolution, the FPN lateral) is a bias-free 1x1 convolution directly in front of a train-mode
    BatchNorm: a per-channel constant goes through the 1x1 convolution as a per-channel constant, which the batch mean removes.
    The same zero gradient as a conv bias in front of a BatchNorm, one linear map further on: 2e-16 at most in the float64 oracle."""
    m = re.fullmatch(r"(camera_encoder\.stage\d+\.conv)\.(\d+)\.bias", name)
    if m is None or name[:-4] + "running_mean" not in state:
        return False
    later = [k for k in state if k.startswith(m.group(1) + ".") and int(k[len(m.group(1)) + 1:].split(".")[0]) > int(m.group(2))]
    return not later


def check_adamw(before, after, grads, k, state, tag="", lr=LR, weight_decay=WD, g64=None):
    """`before` / `after`: ({name: param}, {name: exp_avg}, {name: exp_avg_sq}) around step k, `grads` the device's OWN gradient of
    that step.  float64 AdamW at step k from `before` must give `after`: parameters within 2e-6 * max(1, |w|max), moments within
    1e-6 of the tensor's largest magnitude, elements with |g| < 1e-6 left out (Adam turns rounding-noise gradients into +-lr).
    A tensor left out whole must be a shift in front of a train-mode BatchNorm, and (`g64`: the float64 oracle's gradients) its true
    gradient zero to float64 rounding."""
    want_p, want_m, want_v = adamw64(before[0], grads, before[1], before[2], k, lr, weight_decay)
    left_out = total = 0
    worst = 0.0
    for name, g in grads.items():
        keep = g.detach().double().cpu().abs() >= TINY_GRAD
        total += keep.numel()
        left_out += int((~keep).sum())
        if not keep.any():
            assert bias_in_front_of_batchnorm(name, state) or stage_shift_in_front_of_batchnorm(name, state), (tag, name, "left out whole")
            assert g64 is None or g64[name].abs().max().item() < 1e-12, (tag, name, "left out whole, float64 gradient not zero")
            continue
        for what, got, want, rtol, floor in (("param", after[0], want_p, PARAM_RTOL, 1.0), ("exp_avg", after[1], want_m, MOMENT_RTOL, 0.0),
                                             ("exp_avg_sq", after[2], want_v, MOMENT_RTOL, 0.0)):
            w = want[name]
            d = (got[name].detach().double().cpu() - w).abs()[keep].max().item()
            tol = rtol * max(floor, w.abs().max().item())
            worst = max(worst, d / tol if tol > 0 else 0.0)
            assert d <= tol, (tag, what, name, d, tol)
    print(f"{tag} AdamW step {k}: worst |d| / tol {worst:.3g}, left out {left_out} of {total} elements ({100.0 * left_out / total:.2f} %)")
    assert left_out <= LEFT_OUT_CAP * total, (tag, left_out, total)


def rel_l2(got, want):
    """per tensor: ||got - want|| / max(||want||, 1e-3 * sqrt(numel)) -- _gpu_util.grads_match's relL2(all)"""
    a, b = got.detach().double().cpu(), want.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-3 * b.numel() ** 0.5)).item()


def check_gradients(got, ref64, ref32, tag=""):
    """Asserted: per tensor the gross bound only.  Printed: the sorted relative errors of `got` and of the float32 CPU oracle against
    float64 (median and maximum, one RATIO line) -- at moved weights the float32 oracle itself lands on activation kinks, so the
    strict criterion of test_gradients_against_fp64_oracle is not asserted at k >= 2; gradient exactness at step k follows from
    restart equivalence (step k equals, bit for bit, a first step from the same state)."""
    from _gpu_util import fp64_rel_errors
    g64 = {n: v.double() for n, v in ref64["grads"].items()}
    assert set(got) == set(g64), sorted(set(got) ^ set(g64))
    bad = [(n, e) for n in g64 for e in [rel_l2(got[n], g64[n])] if not e <= GROSS_GRAD_TOL]
    dev, cpu = fp64_rel_errors(g64, got), fp64_rel_errors(g64, ref32["grads"])
    med = lambda v: v[len(v) // 2]
    print(f"RATIO {tag} gradients vs float64: device median {med(dev):.2e} max {dev[-1]:.2e} | float32 CPU oracle median {med(cpu):.2e} "
          f"max {cpu[-1]:.2e} | median ratio {med(dev) / max(med(cpu), 1e-30):.2f}")
    assert not bad, (tag, bad)


def check_step(got, snapshot, k, objective, fusion, tag=""):
    """All of the above for one step.  `snapshot`: {"state", "exp_avg", "exp_avg_sq"} before step k (CPU); `got`: {"parts", "logits",
    "grads", "state", "exp_avg", "exp_avg_sq"} after it.  -> (ref64, ref32)"""
    batch = inputs(k)
    ref64 = oracle_step(objective, fusion, snapshot["state"], batch, torch.float64)
    ref32 = oracle_step(objective, fusion, snapshot["state"], batch, torch.float32)
    check_losses_and_logits(got["parts"], got["logits"], ref64, ref32, tag)
    check_bn_buffers(got["state"], ref64, k, tag)
    names = list(got["grads"])
    check_adamw(({n: snapshot["state"][n] for n in names}, snapshot["exp_avg"], snapshot["exp_avg_sq"]),
                ({n: got["state"][n] for n in names}, got["exp_avg"], got["exp_avg_sq"]), got["grads"], k, snapshot["state"], tag, g64=ref64["grads"])
    check_gradients(got["grads"], ref64, ref32, tag)
    return ref64, ref32


def host_sequence(objective, fusion, dtype=torch.float32):
    """The K-step sequence with the oracle in `dtype` in the device's place: yields (k, snapshot, got) as check_step takes them."""
    state = _cast(student_state(fusion), dtype)
    names = O.trainable_keys(state)
    m = {n: torch.zeros_like(state[n]) for n in names}
    v = {n: torch.zeros_like(state[n]) for n in names}
    for k in range(1, K + 1):
        snap = {"state": O.clone_state(state), "exp_avg": O.clone_state(m), "exp_avg_sq": O.clone_state(v)}
        out = oracle_step(objective, fusion, state, inputs(k), dtype)
        state = O.clone_state(out["state"])
        O.adamw_step([state[n] for n in names], [out["grads"][n] for n in names], [m[n] for n in names], [v[n] for n in names],
                     step=k, lr=LR, betas=BETAS, weight_decay=WD)
        yield k, snap, {"parts": out["parts"], "logits": out["logits"], "grads": out["grads"], "state": O.clone_state(state),
                        "exp_avg": O.clone_state(m), "exp_avg_sq": O.clone_state(v)}
