"""The opt-in focal + Tversky hard-label loss on the GPU: kd_seg_region_loss_fwd_bwd (csrc/kd_loss_region.hip) called through the
C ABI against the float64 reference of tests/_fp64_region_loss_ref.py, every value and every dzs element within the reference's
bound with no outlier allowance, on the cases tests/test_fp64_region_loss_ref_host.py runs in plain fp32; then the layers
above it: gamma = 0 / wt = 0 against the CE kernel, the all-ignored batch, bit-for-bit determinism, the autograd objective
against the fused one, a KDStep eager / graphed, the Trainer, and the untouched default path.  Outputs start as NaN and carry
sentinel guard tails."""
import inspect
import json
import os

import pytest
import torch

import _fp64_loss_ref as L
import _fp64_region_loss_ref as R
import kd_oracle as O
from _gpu_util import build_product, load_random_state
from test_gpu_tail_kernels import Buf, _big, _check

pytestmark = pytest.mark.gpu

NVALS = 17


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _call(tensors, a, NC, grad=True, sp=None):
    """one call on guarded buffers -> (vals Buf, dzs Buf or None)"""
    lib, P, stream = _lib()
    zs, zt, y, cw = tensors
    sp = sp or a["sp"]
    nbytes = lib.kd_seg_region_loss_ws_bytes(a["npix"])
    assert nbytes == R.seg_layout(a["npix"])[0] * 64
    ws, vals = Buf(nbytes // 4), Buf(NVALS)
    dzs = Buf(a["B"], NC, a["HW"]) if grad else None
    gd = None if a["gdev"] is None else torch.tensor([a["gdev"]], device="cuda")
    lib.call("kd_seg_region_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), a["ign"], a["T"], a["alpha"], a["gscale"], P(gd),
             *(sp[k] for k in R.KEYS), P(vals.t), P(dzs.t) if grad else None, a["B"], NC, a["HW"], P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ws.guard_ok("ws"); vals.guard_ok("vals")
    if grad:
        dzs.guard_ok("dzs")
    return vals, dzs


def _run(case):
    tensors, a = R.case_setup(case, "cuda")
    vals, dzs = _call(tensors, a, case.NC, case.grad)
    ref = R.case_reference(case, tensors, a)
    what, n = R.case_id(case), 5 + case.NC
    v, e = ref["vals"]
    got = vals.t[:n].double()
    for i, name in enumerate(["hard", "kl", "sumw", "focal", "tversky"] + [f"ti{c}" for c in range(case.NC)]):
        print(f"{what} {name}: got {got[i].item():.9g} float64 {v[i].item():.9g} |d|/bound {((got[i] - v[i]).abs() / e[i].clamp_min(1e-300)).item():.3g}")
    assert bool(torch.isfinite(v).all()) and bool(v[2] > 0)
    _check(f"region vals {what}", vals.t[:n], (v, e))
    sp = a["sp"]
    if sp["wf"] == 0:
        assert vals.t[3].item() == 0.0
    if sp["wt"] == 0:
        assert vals.t[4].item() == 0.0 and bool((vals.t[5:] == 0).all())
    if not case.teacher:
        assert vals.t[1].item() == 0.0
    if case.absent and sp["wt"] > 0:
        assert 0 < vals.t[5 + case.NC - 1].item() < 1        # the absent class still counts: TI = s / (a FP + s)
    if case.grad:
        assert bool(torch.isfinite(dzs.t).all()), what
        g, eg = ref["dzs"]
        print(f"{what} dzs: worst |d|/bound {((dzs.t.double() - g).abs() / eg.clamp_min(1e-300)).max().item():.3g}")
        _check(f"region dzs {what}", dzs.t, ref["dzs"])


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_kernel_against_float64(case):
    _run(case)


def test_kernel_against_float64_x4_head_count():
    _big()
    _run(R.X4_CASE)


@pytest.mark.parametrize("size,NC,teacher", [("partial_block", 3, True), ("cap+1", 2, True), ("ragged", 4, False)])
def test_gamma0_wt0_is_the_ce_kernel(size, NC, teacher):
    """value and gradient agree with kd_seg_loss_fwd_bwd within the sum of the two kernels' bounds"""
    lib, P, stream = _lib()
    case = R.Case(size, NC, True, teacher, True, "gdev", False, 1)
    tensors, a = R.case_setup(case, "cuda")
    zs, zt, y, cw = tensors
    sp = R.spec(gamma=0.0, wt=0.0)
    vals, dzs = _call(tensors, a, NC, True, sp)
    nbytes = lib.kd_seg_loss_ws_bytes(a["npix"])
    ws, losses, dce = Buf(nbytes // 4), Buf(3), Buf(a["B"], NC, a["HW"])
    gd = torch.tensor([a["gdev"]], device="cuda")
    lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), a["ign"], a["T"], a["alpha"], a["gscale"], P(gd), P(losses.t), P(dce.t),
             a["B"], NC, a["HW"], P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    d = lambda t: None if t is None else t.double()
    r_reg = R.region_loss(d(zs), d(zt), y, d(cw), a["ign"], a["T"], a["alpha"], a["gs"], a["n_seq"], sp)
    r_ce = L.seg_loss(d(zs), d(zt), y, d(cw), a["ign"], a["T"], a["alpha"], a["gs"], a["n_seq"])
    e_v = r_reg["vals"][1][:3] + r_ce["losses"][1]
    dv = (vals.t[:3].double() - losses.t.double()).abs()
    print("values", vals.t[:3].tolist(), losses.t.tolist(), (dv / e_v.clamp_min(1e-300)).tolist())
    assert bool((dv <= e_v).all()), (dv.tolist(), e_v.tolist())
    assert vals.t[3].item() == vals.t[0].item()                  # wf = 1, wt = 0: L_hard is the focal term
    _check("dzs against the CE kernel", dzs.t, (dce.t.double(), r_reg["dzs"][1] + r_ce["dzs"][1]))


@pytest.mark.parametrize("size,NC", [("partial_block", 3), ("cap+1", 2)])
def test_all_ignored_batch(size, NC):
    case = R.Case(size, NC, True, False, True, "wf0", False, 0)
    (zs, zt, y, cw), a = R.case_setup(case, "cuda")
    y = torch.full_like(y, a["ign"])
    vals, dzs = _call((zs, None, y, cw), a, NC, True)
    ref = R.region_loss(zs.double(), None, y, cw.double(), a["ign"], a["T"], a["alpha"], a["gs"], a["n_seq"], a["sp"])
    assert ref["vals"][0][0].item() == 0.0                        # every TI is s / s: Tversky = 0
    _check("all-ignored, wf = 0", vals.t[:5 + NC], ref["vals"])
    assert vals.t[0].item() == 0.0 and vals.t[2].item() == 0.0
    assert bool((dzs.t == 0).all()), "the gradient of an all-ignored batch is exactly zero (no 0 * NaN)"
    vals, dzs = _call((zs, None, y, cw), a, NC, True, R.spec())
    assert bool(torch.isnan(vals.t[0])) and bool(torch.isnan(vals.t[3])), "wf > 0: 0/0 like the CE"
    assert vals.t[4].item() == 0.0 and bool((dzs.t == 0).all())


@pytest.mark.parametrize("size,NC", [("partial_block", 4), ("ragged", 3)])
def test_two_calls_give_identical_bytes(size, NC):
    case = R.Case(size, NC, True, True, True, "gdev", True, 3)
    tensors, a = R.case_setup(case, "cuda")
    (v0, g0), (v1, g1) = _call(tensors, a, NC), _call(tensors, a, NC)
    assert torch.equal(v0.t.view(torch.int32), v1.t.view(torch.int32))
    assert torch.equal(g0.t.view(torch.int32), g1.t.view(torch.int32))
    vf, _ = _call(tensors, a, NC, grad=False)                     # forward only: the same values
    assert torch.equal(v0.t.view(torch.int32), vf.t.view(torch.int32))


def test_region_seg_loss_function():
    """the autograd.Function: values of the direct call, gradient scaled by the upstream gradient on the device"""
    from kdrt.losses import RegionLoss, region_seg_loss
    case = R.Case("partial_block", 3, True, True, True, "default", False, 0)
    (zs, zt, y, cw), a = R.case_setup(case, "cuda")
    vals, dzs = _call((zs, zt, y, cw), a, 3)
    B, HW = a["B"], a["HW"]
    z4 = zs.view(B, 3, HW, 1).clone().requires_grad_()
    hard, kl, parts = region_seg_loss(z4, y.view(B, HW, 1), RegionLoss(), cw, a["ign"], zt.view(B, 3, HW, 1), a["T"], a["alpha"])
    assert set(parts) == {"focal", "tversky", "class_ti"} and parts["class_ti"].shape == (3,)
    got = torch.stack([hard.detach(), kl, parts["focal"], parts["tversky"]])
    assert torch.equal(got, vals.t[[0, 1, 3, 4]]) and torch.equal(parts["class_ti"], vals.t[5:8])
    hard.backward()
    assert torch.equal(z4.grad.view(B, 3, HW), dzs.t)


# ---- the KD objective, the KD step and the trainers ---------------------------------------------------------------------------

SHAPE = (2, 64, 700, 16)            # batch, image size, points, BEV grid: the smallest the unit tests of the KD objective use


def _spec():
    from kdrt.losses import RegionLoss
    return RegionLoss(gamma=2.0, wf=1.0, wt=0.8, a=0.7, b=0.3, s=1.0)


def _inputs():
    B, HW, N, G = SHAPE
    images, pts, _ = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    labels = O.make_inputs(B, HW, N, HW // 4, 4, pad_tail=40)[2]             # labels live on the logits' grid (the camera map)
    return images.cuda(), pts.cuda(), labels.cuda()


def _models():
    G = SHAPE[3]
    teacher = build_product("concat", G)
    load_random_state(teacher, "concat", 11)
    student = build_product("weighted", G)
    load_random_state(student, "weighted", 12)
    student.train()
    return student, teacher


def _kd_step(lr, steps=1, graphed=0, **kw):
    """`steps` eager KD steps (graphed: that many of them as replays after the capture's warm-up) -> (parts, flat gradient, flat parameters)"""
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    images, pts, labels = _inputs()
    student, teacher = _models()
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=0.0 if lr == 0 else 1e-3)
    step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5]).cuda(), **kw)
    if graphed:
        g = GraphedKDStep(step, images, pts, labels, warmup=steps - graphed)
        for _ in range(graphed):
            parts = g(images, pts, labels)
    else:
        for _ in range(steps):
            parts = step(images, pts, labels)
    torch.cuda.synchronize()
    flat = torch.cat([p.detach().flatten() for p in student.parameters()])
    return {k: v.clone() for k, v in parts.items() if k != "logits"}, opt.flat.grad.clone(), flat.clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_autograd_objective_and_fused_objective_give_the_same_bits():
    """kd_objective(..., hard_loss=spec)[0].backward() against kd_objective_backward(..., hard_loss=spec): lr = 0 keeps the flat
    gradient of the step for the comparison"""
    (p0, g0, _), (p1, g1, _) = _kd_step(0.0, fused_objective=False, hard_loss=_spec()), _kd_step(0.0, fused_objective=True, hard_loss=_spec())
    assert set(p0) == set(p1) == {"ce", "kl", "mse_cam", "mse_lidar", "focal", "tversky", "total"}
    for k in p0:
        assert _same_bits(p0[k], p1[k]), (k, p0[k].item(), p1[k].item())
    assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
    assert _same_bits(g0, g1), (g0 - g1).abs().max().item()
    # and the hard-label term is not the CE's: the option changes the step
    pc, gc, _ = _kd_step(0.0, fused_objective=True)
    assert set(pc) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
    assert not _same_bits(pc["ce"], p1["ce"]) and not _same_bits(gc, g1) and _same_bits(pc["kl"], p1["kl"])


def test_kd_step_with_hard_loss_eager_fused_and_graphed():
    spec = _spec()
    p_f, _, w_f = _kd_step(1e-3, fused_objective=True, hard_loss=spec)
    p_a, _, w_a = _kd_step(1e-3, fused_objective=False, hard_loss=spec)
    assert _same_bits(w_f, w_a), (w_f - w_a).abs().max().item()
    for k in ("focal", "tversky", "total"):
        assert bool(torch.isfinite(p_f[k])), k
    want = spec.wf * p_f["focal"].double() + spec.wt * p_f["tversky"].double()
    assert abs(p_f["ce"].item() - want.item()) <= 4 * L.U * abs(want.item())
    # three warm-up steps and two replays against five eager steps
    p_e, _, w_e = _kd_step(1e-3, steps=5, hard_loss=spec)
    p_g, _, w_g = _kd_step(1e-3, steps=5, graphed=2, hard_loss=spec)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    assert _same_bits(p_e["total"], p_g["total"]) and _same_bits(p_e["focal"], p_g["focal"]) and _same_bits(p_e["tversky"], p_g["tversky"])


def test_default_path_is_the_parent_commits():
    """a KDStep built with the parent commit's positional arguments only, one built by keywords without the option and one with
    hard_loss=None leave the same parameter bytes"""
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    names = list(inspect.signature(KDStep.__init__).parameters)
    assert names == ["self", "student", "teacher", "optimizer", "class_weights", "T", "alpha", "beta", "ignore_index", "reducer",
                     "teacher_storage", "fused_objective", "hard_loss"]
    images, pts, labels = _inputs()
    out = []
    for how in ("positional", "keywords", "none"):
        student, teacher = _models()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        cw = torch.tensor([0.4, 3.5]).cuda()
        if how == "positional":
            step = KDStep(student, teacher, opt, cw, 4.0, 1.0, 1.0, -1, None, "fp32", True)
        elif how == "keywords":
            step = KDStep(student, teacher, opt, class_weights=cw)
        else:
            step = KDStep(student, teacher, opt, cw, hard_loss=None)
        assert step.hard_loss is None
        for _ in range(2):
            parts = step(images, pts, labels)
        torch.cuda.synchronize()
        assert set(parts) == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"}
        out.append((torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone()))
    for w, t in out[1:]:
        assert _same_bits(w, out[0][0]) and _same_bits(t, out[0][1])


def test_trainer_with_hard_loss(tmp_path):
    from _fake_pandaset import write_tree
    from kdrt.losses import region_seg_loss
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer, Trainer
    spec = _spec()
    # no NaN points (they would poison train-mode BN) and no sweep above max_points: a longer one is cut to a random subset on
    # every pass, and the loss below is compared over two passes of the validation loader
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False)
    torch.manual_seed(0)
    model = build_product("weighted", 64)
    tr = Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"), class_weights=[0.4, 3.5], num_epochs=1, hard_loss=spec)
    assert tr.hard_loss is spec
    train_loss, tm = tr.train_epoch()
    val_loss, vm = tr.validate()
    tr.update_history(train_loss, tm["miou"], val_loss, vm["miou"], 1e-3)
    hist = json.load(open(os.path.join(tmp_path / "ck", "training_history.json")))
    assert list(hist) == ["train_loss", "train_miou", "val_loss", "val_miou", "lr"] and hist["val_loss"] == [val_loss]
    assert train_loss == train_loss and val_loss == val_loss and 0 < val_loss
    # validate() reports the loss it trains with: the region loss of the evaluated model, batch by batch
    model.eval()
    total, n = 0.0, 0
    with torch.no_grad():
        for batch in vl:
            logits = model(batch["image"].cuda(), batch["points"].cuda())
            seg = batch["segmentation"].cuda()
            total += region_seg_loss(logits, seg, spec, tr.class_weights, -1)[0].item()
            n += 1
    assert abs(val_loss - total / n) <= 1e-6 * max(1.0, abs(val_loss)), (val_loss, total / n)
    ce_loss = Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck2"), class_weights=[0.4, 3.5], num_epochs=1).validate()[0]
    assert abs(ce_loss - val_loss) > 1e-4, "the default trainer still reports the weighted CE"
    with pytest.raises(ValueError):
        Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck3"), hard_loss="focal_tversky")
    # the KD trainer hands the option to its step
    torch.manual_seed(1)
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck4"),
                   class_weights=[0.4, 3.5], num_epochs=1, hard_loss=spec)
    assert kd.kd_step.hard_loss is spec
    kd_loss, _ = kd.train_epoch()
    assert kd_loss == kd_loss and kd.validate()[0] > 0
