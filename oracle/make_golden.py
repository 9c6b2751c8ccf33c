#!/usr/bin/env python3
"""Golden-vector generator -- runs ONLY in the build container, where /root/reference exists.

Imports the real reference modules (by file path, so nothing from the reference is copied or
installed), drives them on seeded inputs and name-keyed deterministic weights
(`kd_oracle.randomize_state`), and writes small `.npz` fixtures under tests/golden/.  The
fixtures hold data only (inputs are regenerated from seeds by the tests; expected outputs and
per-tensor gradient digests are stored).  The GPU box never sees the reference.

usage:  python oracle/make_golden.py [--ref /root/reference] [--out tests/golden]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kd_oracle as O  # noqa: E402

sys.dont_write_bytecode = True
_TRN = None


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(t: torch.Tensor) -> np.ndarray:
    t = t.detach().double().reshape(-1)
    head = torch.zeros(4, dtype=torch.float64)
    head[: min(4, t.numel())] = t[:4]
    return np.concatenate([[t.sum().item(), t.norm().item(), t.abs().max().item()], head.numpy()])


PROJ_SEED = 20261016


def grad_projections(seed: int, index: int, numel: int) -> torch.Tensor:
    """[4, numel] float64 N(0, 1) directions for parameter number `index` (named_parameters order); the tests rebuild them."""
    g = torch.Generator().manual_seed(seed * 1000 + index)
    return torch.randn(4, numel, generator=g, dtype=torch.float64)


def build(ref_mods, fusion, out_ch, num_classes=2, grid=16, output_mode="same"):
    cam_m, lid_m, fus_m = ref_mods
    cam = cam_m.TwinLiteEncoder(return_multiscale=True)
    lid = lid_m.LiDAREncoder(encoder_type="spatial", grid_size=(grid, grid), use_vectorized=True)
    return fus_m.CompleteSegmentationModel(
        camera_encoder=cam, lidar_encoder=lid, num_classes=num_classes, fusion_type=fusion,
        fusion_out_channels=out_ch, camera_fpn_stages=["stage3", "stage4", "stage5"],
        camera_fpn_channels=128, output_mode=output_mode)


def calibrated_bn_stats(model, images, pts):
    """Running statistics that a train-mode forward of the REFERENCE model leaves behind when every BatchNorm's momentum
    is 1.0 for that one forward (running_mean = the batch mean, running_var = the unbiased batch variance): an eval
    forward with them has O(1) activations and O(1..10) logits, unlike `randomize_state`'s arbitrary statistics
    (|logits| up to 170), so the north-star tolerance -- abs 1e-4 on fp32 logits -- can be asserted without scaling.
    Returns {buffer key: tensor}; the model is left in eval mode with those buffers loaded."""
    bns = [m for m in model.modules() if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d))]
    old = [m.momentum for m in bns]
    for m in bns:
        m.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(images, pts)
    for m, o in zip(bns, old):
        m.momentum = o
    model.eval()
    return {k: v.clone() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}


def section_calibrated_eval(mods, out_dir):
    """8. eval forward on well-scaled activations: per fusion, B=2 / 64^2 / N=512 / grid 16."""
    B, HW, N, G = 2, 64, 512, 16
    for fusion, oc in (("concat", 256), ("minimal", 128), ("weighted", 128)):
        model = build(mods, fusion, oc, grid=G)
        model.load_state_dict(O.randomize_state(model.state_dict(), 31))
        images, pts, _ = O.make_inputs(B, HW, N, G, 31, pad_tail=40)
        stats = calibrated_bn_stats(model, images, pts)
        images2, pts2, _ = O.make_inputs(B, HW, N, G, 32, pad_tail=40)      # another batch than the calibration one
        with torch.no_grad():
            logits, mids = model(images2, pts2, return_intermediates=True)
        out = {"stat_keys": np.array(list(stats.keys()))}
        for i, v in enumerate(stats.values()):
            out[f"stat_{i}"] = v.numpy()
        out["logits"] = logits.numpy()
        out["argmax"] = logits.argmax(1).numpy()
        for k in ("camera_feat", "lidar_feat", "pre_fusion", "post_fusion"):
            out[k + "_digest"] = digest(mids[k])
            out[k + "_slice"] = mids[k][:, :8, :4, :4].contiguous().numpy()
        np.savez_compressed(os.path.join(out_dir, f"model_{fusion}_cal.npz"), **out)


def section_headline(mods, out_dir):
    """9. the BENCHMARKED workload pinned to the reference (VERDICT r3 missing #2): B=2 frames of 256^2 with N=80 000
    points, grid 64, concat teacher (eval, calibrated statistics) -> weighted student (train BN): logits, CE, the KD
    terms composed from stock torch losses over the reference modules (as section 5), per-tensor gradient digests, BN
    buffers after the forward; plus the plain CE step of the reference's trainer (trainer.py:86-90) on the same batch."""
    B, HW, N, G = 2, 256, 80000, 64
    teacher = build(mods, "concat", 256, grid=G)
    teacher.load_state_dict(O.randomize_state(teacher.state_dict(), 11))
    student = build(mods, "weighted", 128, grid=G)
    st_s = O.randomize_state(student.state_dict(), 12)
    student.load_state_dict(st_s)
    images, pts, labels = O.make_inputs(B, HW, N, G, 7, pad_tail=4000)
    pts, n_nudged = O.binning_stable_points(pts, (G, G))           # so that the float64 run below bins every point alike
    cal_im, cal_pts, _ = O.make_inputs(B, HW, N, G, 8, pad_tail=4000)
    stats = calibrated_bn_stats(teacher, cal_im, cal_pts)
    out = {"stat_keys": np.array(list(stats.keys())), "points_nudged": np.int64(n_nudged)}
    for i, v in enumerate(stats.values()):
        out[f"stat_{i}"] = v.numpy()
    T, alpha, beta = 4.0, 1.0, 1.0
    cw = torch.tensor([0.4, 3.5])
    with torch.no_grad():
        zt, mt = teacher(images, pts, return_intermediates=True)
    student.train()
    zs, ms_ = student(images, pts, return_intermediates=True)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=cw)(zs, labels)
    kl = F.kl_div(F.log_softmax(zs / T, 1), F.softmax(zt / T, 1), reduction="sum") / (B * G * G)
    mse_c = F.mse_loss(ms_["camera_feat"], mt["camera_feat"])
    mse_l = F.mse_loss(ms_["lidar_feat"], mt["lidar_feat"])
    total = ce + alpha * T * T * kl + beta * (mse_c + mse_l)
    student.zero_grad()
    total.backward()
    out.update(teacher_logits=zt.numpy(), student_logits=zs.detach().numpy(), teacher_argmax=zt.argmax(1).numpy(),
               student_argmax=zs.argmax(1).numpy(), ce=np.float64(ce.item()), kl=np.float64(kl.item()),
               mse_cam=np.float64(mse_c.item()), mse_lidar=np.float64(mse_l.item()), total=np.float64(total.item()))
    for k in ("camera_feat", "lidar_feat"):
        out[f"teacher_{k}_digest"] = digest(mt[k]); out[f"student_{k}_digest"] = digest(ms_[k])
        out[f"teacher_{k}_slice"] = mt[k][:, :8, 30:34, 30:34].contiguous().numpy()
        out[f"student_{k}_slice"] = ms_[k].detach()[:, :8, 30:34, 30:34].contiguous().numpy()
    names = [n for n, _ in student.named_parameters()]
    out["grad_keys"] = np.array(names)
    out["kd_grad_digest"] = np.stack([digest(p.grad) for _, p in student.named_parameters()])
    for tag, p in (("head_cls_w", student.head.cls.weight), ("stem_w", student.camera_encoder.stem[0].weight),
                   ("lidar_w0", student.lidar_encoder.encoder.point_mlp[0].weight),
                   ("lidar_w6", student.lidar_encoder.encoder.point_mlp[6].weight),
                   ("stage3_proj_w", student.camera_encoder.stage3.conv[6].weight)):
        out["kd_grad_" + tag] = p.grad.numpy().copy()
    bufs = {k: v for k, v in student.state_dict().items() if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    out["buf_keys"] = np.array(list(bufs.keys()))
    out["buf_digest"] = np.stack([digest(v.float()) for v in bufs.values()])
    # ground truth for the gradient comparison at this size: the SAME reference modules evaluated in float64 (the step is
    # ill-conditioned at 256^2 / 80 000 points -- BatchNorm-backward cancellations -- so two correct fp32 evaluations differ
    # by ~1e-3; a test compares its distance to this truth with the fp32 reference's own distance, stored beside it)
    g32 = {n: p.grad.detach().double().clone() for n, p in student.named_parameters()}
    t64 = build(mods, "concat", 256, grid=G)
    t64.load_state_dict(teacher.state_dict()); t64 = t64.double().eval()
    s64 = build(mods, "weighted", 128, grid=G)
    s64.load_state_dict(st_s); s64 = s64.double().train()
    i64, p64 = images.double(), pts.double()
    with torch.no_grad():
        zt64, mt64 = t64(i64, p64, return_intermediates=True)
    zs64, ms64 = s64(i64, p64, return_intermediates=True)
    ce64 = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=cw.double())(zs64, labels)
    kl64 = F.kl_div(F.log_softmax(zs64 / T, 1), F.softmax(zt64 / T, 1), reduction="sum") / (B * G * G)
    mse64 = F.mse_loss(ms64["camera_feat"], mt64["camera_feat"]) + F.mse_loss(ms64["lidar_feat"], mt64["lidar_feat"])
    tot64 = ce64 + alpha * T * T * kl64 + beta * mse64
    s64.zero_grad()
    tot64.backward()
    g64 = {n: p.grad.detach().clone() for n, p in s64.named_parameters()}
    out["total64"] = np.float64(tot64.item())
    out["student_logits64_maxdiff"] = np.float64((zs64.detach() - zs.detach().double()).abs().max().item())
    out["kd_grad_norm64"] = np.array([g64[n].norm().item() for n in names])
    out["kd_grad_relerr_fp32_reference"] = np.array([((g32[n] - g64[n]).norm() / g64[n].norm().clamp_min(1e-300)).item() for n in names])
    for tag, n in (("head_cls_w", "head.cls.weight"), ("stem_w", "camera_encoder.stem.0.weight"),
                   ("lidar_w0", "lidar_encoder.encoder.point_mlp.0.weight"), ("lidar_w6", "lidar_encoder.encoder.point_mlp.6.weight"),
                   ("stage3_proj_w", "camera_encoder.stage3.conv.6.weight")):
        out["kd_grad64_" + tag] = g64[n].numpy().copy()
    # element-wise pins for EVERY tensor at a few bytes each: four fixed Gaussian projections <g, r_k> of the float64 and of
    # the fp32 gradient (a permuted or sign-flipped gradient keeps its norm but moves each projection by ~sqrt(2)*|g|)
    out["kd_grad_proj_seed"] = np.int64(PROJ_SEED)
    r = [grad_projections(PROJ_SEED, i, g64[n].numel()) for i, n in enumerate(names)]
    out["kd_grad_proj64"] = np.stack([(rk @ g64[n].reshape(-1)).numpy() for rk, n in zip(r, names)])
    out["kd_grad_proj32_reference"] = np.stack([(rk @ g32[n].reshape(-1)).numpy() for rk, n in zip(r, names)])
    del t64, s64, zs64, ms64, zt64, mt64
    # the reference trainer's own step on the same batch (CE only), fresh statistics
    student.load_state_dict(st_s)
    student.train()
    zs2 = student(images, pts)
    ce2 = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=cw)(zs2, labels)
    student.zero_grad()
    ce2.backward()
    out["ce_step_loss"] = np.float64(ce2.item())
    out["ce_grad_digest"] = np.stack([digest(p.grad) for _, p in student.named_parameters()])
    sm = _TRN.SegmentationMetrics(num_classes=2)
    sm.update(zs2.detach(), labels)
    out["confusion"] = sm.confusion.copy()
    np.savez_compressed(os.path.join(out_dir, "headline_kd_n80k.npz"), **out)


def section_intensity255(mods, lid_m, out_dir):
    """10. unnormalised LiDAR intensity, 0..255 as in the real PandaSet sweeps (pandaset_dataset.py:119-127; SURVEY
    section 8d): the LiDAR encoder alone (train: output + parameter gradients; eval on calibrated statistics) and one
    weighted-fusion CE step."""
    G = 16
    def pts255(B, N, seed):
        _, p, _ = O.make_inputs(B, 64, N, G, seed, pad_tail=N // 12)
        g = torch.Generator().manual_seed(900 + seed)
        p[..., 3] = torch.floor(torch.rand(p.shape[:2], generator=g) * 256.0).clamp_(0, 255)
        p[:, N - N // 12:, :] = 0.0
        return p
    out = {}
    lid = lid_m.SpatialLiDAREncoder(grid_size=(G, G))
    st = O.randomize_state(lid.state_dict(), 3)
    p = pts255(2, 2048, 41)
    out["points"] = p.numpy()
    lid.load_state_dict(st); lid.train()
    y = lid(p)
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    lid.zero_grad(); (y * up).sum().backward()
    out["train_out"] = y.detach().contiguous().numpy(); out["upstream"] = up.numpy()
    for n_, p_ in lid.named_parameters():
        out["grad_" + n_] = p_.grad.numpy().copy()
    bns = [m for m in lid.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    lid.load_state_dict(st)
    for m in bns: m.momentum = 1.0
    lid.train()
    with torch.no_grad(): lid(p)
    for m in bns: m.momentum = 0.1
    lid.eval()
    for k, v in lid.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            out["cal_" + k] = v.numpy().copy()
    p2 = pts255(2, 2048, 42)
    out["points_eval"] = p2.numpy()
    with torch.no_grad():
        out["eval_out"] = lid(p2).contiguous().numpy()
    model = build(mods, "weighted", 128, grid=G)
    model.load_state_dict(O.randomize_state(model.state_dict(), 13))
    images, _, labels = O.make_inputs(2, 64, 2048, G, 41)
    model.train()
    z = model(images, p)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=torch.tensor([0.4, 3.5]))(z, labels)
    model.zero_grad(); ce.backward()
    out["model_logits"] = z.detach().numpy(); out["model_loss"] = np.float64(ce.item())
    out["model_grad_keys"] = np.array([n for n, _ in model.named_parameters()])
    out["model_grad_digest"] = np.stack([digest(q.grad) for _, q in model.named_parameters()])
    np.savez_compressed(os.path.join(out_dir, "lidar_intensity255.npz"), **out)


def section_ddp_replicas(mods, out_dir):
    """11. data-parallel semantics from REFERENCE replicas (SURVEY section 8c item vii): k in {2, 4} independent reference
    processes' worth of work -- replica r runs the trainer's step (trainer.py:86-90) on micro-batch r with its own
    BatchNorm statistics; the data-parallel gradient is the average over replicas; then one AdamW step on it."""
    B, HW, N, G = 1, 32, 96, 8
    cw = torch.tensor([0.4, 3.5])
    for k in (2, 4):
        out = {}
        model = build(mods, "weighted", 128, grid=G)
        st = O.randomize_state(model.state_dict(), 5)
        names = [n for n, _ in model.named_parameters()]
        acc = None
        for r in range(k):
            model.load_state_dict(st)
            model.train()
            images, pts, labels = O.make_inputs(B, HW, N, G, 100 + r, pad_tail=8)
            z = model(images, pts)
            loss = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=cw)(z, labels)
            model.zero_grad(); loss.backward()
            out[f"loss_{r}"] = np.float64(loss.item())
            out[f"stem_running_mean_{r}"] = model.camera_encoder.stem[1].running_mean.numpy().copy()
            out[f"lidar_bn0_running_var_{r}"] = model.lidar_encoder.encoder.point_mlp[1].running_var.numpy().copy()
            gs = [p.grad.detach().clone() for _, p in model.named_parameters()]
            acc = gs if acc is None else [a + g for a, g in zip(acc, gs)]
        mean = [a / k for a in acc]
        out["grad_keys"] = np.array(names)
        out["mean_grad_digest"] = np.stack([digest(g) for g in mean])
        out["mean_grad_flat_head"] = torch.cat([g.reshape(-1) for g in mean])[:4096].numpy()
        out["mean_grad_head_cls_w"] = mean[names.index("head.cls.weight")].numpy()
        out["mean_grad_stem_w"] = mean[names.index("camera_encoder.stem.0.weight")].numpy()
        model.load_state_dict(st)
        for (_, p), g in zip(model.named_parameters(), mean):
            p.grad = g.clone()
        torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-3).step()
        out["adamw_digest"] = np.stack([digest(p) for _, p in model.named_parameters()])
        np.savez_compressed(os.path.join(out_dir, f"ddp_replicas_k{k}.npz"), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(HERE, "..", "tests", "golden"))
    ap.add_argument("--only", default="", help="comma list of round-4 sections to (re)generate alone: cal,headline,i255,ddp")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(8)
    cam_m = _load(a.ref, "src/models/camera_encoder.py", "ref_camera_encoder")
    lid_m = _load(a.ref, "src/models/lidar_encoder.py", "ref_lidar_encoder")
    fus_m = _load(a.ref, "src/models/fusion_module.py", "ref_fusion_module")
    trn_m = _load(a.ref, "src/training/trainer.py", "ref_trainer")
    mods = (cam_m, lid_m, fus_m)
    global _TRN
    _TRN = trn_m
    r4 = {"cal": lambda: section_calibrated_eval(mods, a.out), "headline": lambda: section_headline(mods, a.out),
          "i255": lambda: section_intensity255(mods, lid_m, a.out), "ddp": lambda: section_ddp_replicas(mods, a.out)}
    if a.only:
        for name in a.only.split(","):
            r4[name]()
        return

    # ---- 1. default-init pins: registration order, param counts, seed-0 weight digests -------
    torch.manual_seed(0)
    enc = cam_m.TwinLiteEncoder()
    sd = enc.state_dict()
    pins = {"cam_keys": np.array(list(sd.keys())),
            "cam_digest": np.stack([digest(v.float()) for v in sd.values()]),
            "cam_params": np.int64(enc.count_parameters())}
    enc.eval()
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        y = enc(x)
    pins["cam_cfg1_out_digest"] = digest(y)
    pins["cam_cfg1_out_slice"] = y[0, :8, :4, :4].numpy()
    for fusion, oc in (("concat", 256), ("minimal", 128), ("weighted", 128)):
        torch.manual_seed(0)
        m = build(mods, fusion, oc, grid=64)
        s = m.get_architecture_summary()
        pins[f"{fusion}_total"] = np.int64(int(s["total_params"].replace(",", "")))
        pins[f"{fusion}_fusion"] = np.int64(int(s["fusion_params"].replace(",", "")))
        msd = m.state_dict()
        pins[f"{fusion}_keys"] = np.array(list(msd.keys()))
        pins[f"{fusion}_shapes"] = np.array([str(tuple(v.shape)) for v in msd.values()])
        pins[f"{fusion}_dtypes"] = np.array([str(v.dtype) for v in msd.values()])
        pins[f"{fusion}_digest"] = np.stack([digest(v.float()) for v in msd.values()])
    np.savez_compressed(os.path.join(a.out, "pins.npz"), **pins)

    # ---- 2. small full-model cases, eval + train(CE backward) ---------------------------------
    B, HW, N, G = 2, 64, 512, 16
    for fusion, oc in (("concat", 256), ("minimal", 128), ("weighted", 128)):
        for seed in (0, 1):
            model = build(mods, fusion, oc, grid=G)
            st = O.randomize_state(model.state_dict(), seed)
            model.load_state_dict(st)
            images, pts, labels = O.make_inputs(B, HW, N, G, seed, pad_tail=40)
            out = {}
            model.eval()
            with torch.no_grad():
                logits, mids = model(images, pts, return_intermediates=True)
                ms = model.camera_encoder(images)
            out["eval_logits"] = logits.numpy()
            out["eval_argmax"] = logits.argmax(1).numpy()
            out["eval_margin"] = np.float64((logits[:, 0] - logits[:, 1]).abs().min().item())
            if seed == 0:                      # full intermediates only for seed 0 (fixture size)
                for k in ("camera_feat", "lidar_feat", "pre_fusion", "post_fusion"):
                    out["eval_" + k] = mids[k].contiguous().numpy()
                for k, v in ms.items():
                    out["eval_" + k] = v.numpy()
            # train mode: CE loss, grads, BN buffers after one forward
            model.load_state_dict(st)
            model.train()
            cw = torch.tensor([0.4, 3.5])
            logits, mids = model(images, pts, return_intermediates=True)
            loss = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=cw)(logits, labels)
            model.zero_grad()
            loss.backward()
            out["train_logits"] = logits.detach().numpy()
            out["train_loss"] = np.float64(loss.item())
            if seed == 0:
                for k in ("camera_feat", "lidar_feat"):
                    out["train_" + k] = mids[k].detach().contiguous().numpy()
            names = [n for n, _ in model.named_parameters()]
            out["grad_keys"] = np.array(names)
            out["grad_digest"] = np.stack([digest(p.grad) for _, p in model.named_parameters()])
            out["grad_head_cls_w"] = model.head.cls.weight.grad.numpy()
            out["grad_stem_w"] = model.camera_encoder.stem[0].weight.grad.numpy()
            out["grad_lidar_w0"] = model.lidar_encoder.encoder.point_mlp[0].weight.grad.numpy()
            bufs = {k: v for k, v in model.state_dict().items()
                    if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
            out["buf_keys"] = np.array(list(bufs.keys()))
            out["buf_digest"] = np.stack([digest(v.float()) for v in bufs.values()])
            # confusion matrix through the reference's SegmentationMetrics (python loop)
            sm = trn_m.SegmentationMetrics(num_classes=2)
            sm.update(logits.detach(), labels)
            out["confusion"] = sm.confusion.copy()
            out["miou"] = np.float64(sm.compute()["miou"])
            # one AdamW step (trainer.py:56)
            opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-3)
            opt.step()
            out["adamw_digest"] = np.stack([digest(p) for _, p in model.named_parameters()])
            np.savez_compressed(os.path.join(a.out, f"model_{fusion}_s{seed}.npz"), **out)

    # ---- 3. LiDAR encoder edge cases ------------------------------------------------------------
    lid = lid_m.SpatialLiDAREncoder(grid_size=(16, 16))
    st = O.randomize_state(lid.state_dict(), 3)
    lid.load_state_dict(st)
    out = {}
    g = torch.Generator().manual_seed(77)
    cases = {}
    p = O.make_inputs(2, 8, 256, 16, 9)[1]
    p[0, :6, 0] = torch.tensor([50.0, 49.99, 0.0, -50.0, -50.01, 50.01])
    p[0, :6, 1] = torch.tensor([50.0, -50.0, 0.0, 49.99, 0.0, 0.0])
    p[1, 100:140] = p[1, 99]                      # exact duplicates -> tie gradient
    p[1, 200:] = 0.0                              # zero-padded tail
    cases["edge"] = p
    pn = p.clone()
    pn[1, 3, 0] = float("nan")                    # NaN point: invalid in eval; poisons BN stats in train
    cases["nan"] = pn
    q = torch.randn(2, 64, 4, generator=g)
    q[..., 0] = 60.0 + q[..., 0].abs()            # all outside => all zeros
    cases["outside"] = q
    for name, pts in cases.items():
        for mode in (("eval",) if name == "nan" else ("eval", "train")):
            lid.load_state_dict(st)
            lid.train(mode == "train")
            out[f"{name}_points"] = pts.numpy()
            coords, valid = lid.points_to_bev_coords(pts)
            out[f"{name}_valid"] = valid.numpy()
            y = lid(pts)
            out[f"{name}_{mode}_out"] = y.detach().contiguous().numpy()
            if mode == "train" and y.requires_grad:
                up = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
                lid.zero_grad()
                (y * up).sum().backward()
                out[f"{name}_upstream"] = up.numpy()
                for n_, p_ in lid.named_parameters():
                    out[f"{name}_grad_{n_}"] = p_.grad.numpy()
        flat, v2 = O.bev_cell_index(pts, (16, 16))
        gc = (coords * lid.grid_tensor).long()
        gc[..., 0].clamp_(0, 15); gc[..., 1].clamp_(0, 15)
        b = torch.arange(pts.shape[0]).view(-1, 1).expand(pts.shape[:2])
        out[f"{name}_flat"] = (b * 256 + gc[..., 1] * 16 + gc[..., 0]).numpy()
    np.savez_compressed(os.path.join(a.out, "lidar_edges.npz"), **out)

    # ---- 4. full-size eval (256^2, N=5000, grid 64) --------------------------------------------
    model = build(mods, "weighted", 128, grid=64)
    st = O.randomize_state(model.state_dict(), 2)
    model.load_state_dict(st)
    model.eval()
    images, pts, labels = O.make_inputs(2, 256, 5000, 64, 2, pad_tail=300)
    with torch.no_grad():
        logits, mids = model(images, pts, return_intermediates=True)
    np.savez_compressed(os.path.join(a.out, "full_weighted_eval.npz"),
                        logits=logits.numpy(), argmax=logits.argmax(1).numpy(),
                        margin=np.float64((logits[:, 0] - logits[:, 1]).abs().min().item()),
                        camera_feat_digest=digest(mids["camera_feat"]),
                        lidar_feat_digest=digest(mids["lidar_feat"]))

    # ---- 5. KD step composed from reference modules + stock torch losses -----------------------
    teacher = build(mods, "concat", 256, grid=G)
    teacher.load_state_dict(O.randomize_state(teacher.state_dict(), 11))
    teacher.eval()
    student = build(mods, "weighted", 128, grid=G)
    student.load_state_dict(O.randomize_state(student.state_dict(), 12))
    student.train()
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    T, alpha, beta = 4.0, 1.0, 1.0
    with torch.no_grad():
        zt, mt = teacher(images, pts, return_intermediates=True)
    zs, ms_ = student(images, pts, return_intermediates=True)
    ce = torch.nn.CrossEntropyLoss(ignore_index=-1, weight=torch.tensor([0.4, 3.5]))(zs, labels)
    kl = F.kl_div(F.log_softmax(zs / T, 1), F.softmax(zt / T, 1), reduction="sum") / (B * G * G)
    mse = F.mse_loss(ms_["camera_feat"], mt["camera_feat"]) + F.mse_loss(ms_["lidar_feat"], mt["lidar_feat"])
    total = ce + alpha * T * T * kl + beta * mse
    student.zero_grad()
    total.backward()
    np.savez_compressed(
        os.path.join(a.out, "kd_step.npz"), ce=np.float64(ce.item()), kl=np.float64(kl.item()),
        mse=np.float64(mse.item()), total=np.float64(total.item()),
        teacher_logits=zt.numpy(), student_logits=zs.detach().numpy(),
        grad_keys=np.array([n for n, _ in student.named_parameters()]),
        grad_digest=np.stack([digest(p.grad) for _, p in student.named_parameters()]))

    # ---- 6. x4 head (test_lidar_encoder.py:281-293) ---------------------------------------------
    m4 = build(mods, "concat", 256, num_classes=3, grid=G, output_mode="x4")
    m4.load_state_dict(O.randomize_state(m4.state_dict(), 21))
    m4.eval()
    images, pts, _ = O.make_inputs(B, HW, N, G, 6)
    with torch.no_grad():
        z4 = m4(images, pts)
    np.savez_compressed(os.path.join(a.out, "head_x4.npz"), logits=z4.numpy())
    # ---- 7. the iterative LiDAR path (use_vectorized=False, lidar_encoder.py:101-143) --------------
    # the reference's own Python double loop on the "edge" points (boundaries, 41 exact duplicates, zero-padded tail):
    # forward values in both modes and, in train mode, the parameter gradients under BOTH flags -- where backward
    # runs at all: the iterative path updates `feature_map[b, :, y, x]` in place, and autograd raises as soon as a
    # cell has received two points ("modified by an inplace operation"), i.e. that path is forward-only upstream
    lid_v = lid_m.SpatialLiDAREncoder(grid_size=(16, 16), use_vectorized=True)
    lid_i = lid_m.SpatialLiDAREncoder(grid_size=(16, 16), use_vectorized=False)
    st = O.randomize_state(lid_v.state_dict(), 3)
    pts = cases["edge"]
    out = {"points": pts.numpy()}
    up = torch.randn(2, 128, 16, 16, generator=torch.Generator().manual_seed(5))
    for mode in ("eval", "train"):
        ys = {}
        for tag, enc_ in (("vec", lid_v), ("iter", lid_i)):
            enc_.load_state_dict(st)
            enc_.train(mode == "train")
            ys[tag] = enc_(pts)
        out[f"iter_{mode}_out"] = ys["iter"].detach().contiguous().numpy()
        out[f"iter_{mode}_same_bits_as_vectorized"] = np.bool_(torch.equal(ys["iter"], ys["vec"]))
        if mode == "train":
            try:
                (ys["iter"] * up).sum().backward()
                out["iter_backward"] = np.array("ok")
            except RuntimeError as e:          # in-place map update: autograd refuses -- a forward-only path upstream
                out["iter_backward"] = np.array("RuntimeError: " + str(e).split(":")[0])
    np.savez_compressed(os.path.join(a.out, "lidar_iterative.npz"), **out)

    for fn in r4.values():
        fn()
    print("golden fixtures written to", os.path.abspath(a.out))
    for f in sorted(os.listdir(a.out)):
        print(f"  {f}: {os.path.getsize(os.path.join(a.out, f))/1024:.1f} KiB")


if __name__ == "__main__":
    main()
