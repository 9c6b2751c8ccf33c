"""The default path with 8 classes, end to end: same-resolution head, weighted CE + temperature KL, argmax and confusion matrix,
KDStep / GraphedKDStep, Trainer, and the loader with a class map.  Every case uses B = 2, a 16 x 16 map, a few hundred points.
Parity is against the CPU oracle (oracle/kd_oracle.py) on identical seeded inputs with the tolerances of tests/test_gpu_parity.py:
logits within _gpu_util.ftol, loss terms within 1e-4, gradients by grads_match with its default tolerances, class indices equal
wherever the oracle's top-two margin exceeds what the logit tolerance can move (2 * tol: each of the two logits by at most tol)."""
import numpy as np
import pytest
import torch

import data_oracle as D
import kd_oracle as O
import _fp64_multiclass_ref as MC
from _gpu_util import build_product, ftol, grads_match, max_err, oracle_run

pytestmark = pytest.mark.gpu

B, HW, N, G, NC = 2, 64, 300, 16, 8
# The input seed of the parity cases, picked on the CPU from the oracle alone.  Seeds 0..7 were scanned: the pixels whose top-two
# logit margin lies within 2 * ftol number 0 to 2 of 512 (at most 0.4 %; the cap is 2 %); seeds 1, 2 and 7 give 0 for the teacher
# and for both students, and of those 2 has the widest smallest margin (1.8e-3 against a tolerance of 1e-4).
SEED = 2
EXEMPT_CAP = 0.02
CW = [0.4, 3.5, 1.0, 2.0, 0.7, 1.5, 3.0, 0.9]


def _inputs(seed=SEED):
    images, pts, _ = O.make_inputs(B, HW, N, G, seed, pad_tail=40)
    labels = O.make_inputs(B, HW, N, HW // 4, seed, pad_tail=40, num_classes=NC)[2]      # labels live on the logits' grid
    return images, pts, labels


def _model(fusion, seed, num_classes=NC, device="cuda", **kw):
    """product model with name-keyed deterministic weights -> (model, the state the oracle runs on)"""
    m = build_product(fusion, G, num_classes=num_classes, device="cpu", **kw)
    st = O.randomize_state({k: v.detach().clone() for k, v in m.state_dict().items()}, seed)
    for k, v in m.state_dict().items():
        if k.endswith("grid_tensor"):
            st[k] = v.clone()
    m.load_state_dict(st)
    return m.to(device), st


def _margin(z):
    top = z.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("fusion", ["concat", "weighted"])
def test_kd_step_parity_with_the_oracle(fusion):
    from kdrt.losses import confusion, kd_objective
    images, pts, labels = _inputs()
    cw = torch.tensor(CW)
    teacher, t_st = _model("concat", 11)
    teacher.eval()
    student, s_st = _model(fusion, 12)
    student.train()
    with torch.no_grad():
        zt, mt = teacher(images.cuda(), pts.cuda(), return_intermediates=True)
    zs, ms = student(images.cuda(), pts.cuda(), return_intermediates=True)
    total, parts = kd_objective(zs, ms, zt, mt, labels.cuda(), cw.cuda(), T=4.0, alpha=1.0, beta=1.0)
    total.backward()
    # the oracle: the teacher's eval forward, the student's training forward, the KD objective and its gradients
    ref_t = oracle_run(t_st, "concat", images, pts, G, training=False)
    so = O.clone_state(s_st, requires_grad=True)
    zs_o, ms_o = O.complete_model(images, pts, so, fusion_type=fusion, grid=(G, G), training=True)
    total_o, parts_o = O.kd_loss(zs_o, ms_o, ref_t["logits"], {k: ref_t[k] for k in ("camera_feat", "lidar_feat")}, labels, cw,
                                 T=4.0, alpha=1.0, beta=1.0)
    total_o.backward()
    assert zs.shape == (B, NC, G, G) and zt.shape == (B, NC, G, G)
    for name, got, want in (("teacher", zt, ref_t["logits"]), ("student", zs, zs_o.detach())):
        tol = ftol(want)
        d = max_err(got, want)[0]
        print(f"{fusion} {name}: logits max |d| {d:.3g}, tolerance {tol:.3g}")
        assert d < tol, (name, d, tol)
        safe = _margin(want) > 2 * tol
        share = 1.0 - safe.float().mean().item()
        print(f"{fusion} {name}: {share * 100:.2f} % of the pixels exempt from the argmax comparison")
        assert share <= EXEMPT_CAP, (name, share)
        conf, pred = confusion(got, torch.where(safe, labels, torch.full_like(labels, -1)).cuda(), NC)
        assert torch.equal(pred.cpu()[safe], want.argmax(1)[safe]), name
        assert np.array_equal(conf.cpu().numpy(), O.confusion_matrix(want, torch.where(safe, labels, torch.full_like(labels, -1)), NC).numpy())
    for k in ("ce", "kl", "mse_cam", "mse_lidar"):
        print(f"{fusion} {k}: {parts[k].item():.7g} oracle {parts_o[k].item():.7g}")
        assert abs(parts[k].item() - parts_o[k].item()) < 1e-4, k
    bad = []
    for name, p in student.named_parameters():
        ok, msg = grads_match(p.grad, so[name].grad)
        if not ok:
            bad.append((name, msg))
    assert not bad, bad


def _kd_step(lr, steps=1, graphed=0, **kw):
    """`steps` KD steps of the 8-class weighted student (graphed: that many as replays) -> (parts, flat gradient, flat parameters)"""
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    images, pts, labels = (t.cuda() for t in _inputs())
    teacher, _ = _model("concat", 11)
    student, _ = _model("weighted", 12)
    student.train()
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=0.0 if lr == 0 else 1e-3)
    step = KDStep(student, teacher, opt, torch.tensor(CW).cuda(), **kw)
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


def test_fused_objective_and_autograd_form_give_the_same_bits():
    (p0, g0, _), (p1, g1, _) = _kd_step(0.0, fused_objective=False), _kd_step(0.0, fused_objective=True)
    assert set(p0) == set(p1) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
    for k in p0:
        assert _same_bits(p0[k], p1[k]), (k, p0[k].item(), p1[k].item())
    assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
    assert _same_bits(g0, g1), (g0 - g1).abs().max().item()


def test_graphed_replay_equals_the_eager_step():
    """three warm-up steps and two replays against five eager steps"""
    p_e, _, w_e = _kd_step(1e-3, steps=5)
    p_g, _, w_g = _kd_step(1e-3, steps=5, graphed=2)
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "ce", "kl"):
        assert _same_bits(p_e[k], p_g[k]), k


def _loaders(num_classes):
    from torch.utils.data import DataLoader
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    kw = {} if num_classes is None else {"num_classes": num_classes}
    mk = lambda seed: DataLoader(SyntheticPandaSet(n_frames=4, num_points=N, image_size=HW, bev_size=G, seed=seed, pad_tail=40, **kw),
                                 batch_size=B, shuffle=False)
    return mk(1), mk(2)


def test_trainer_reports_the_iou_of_its_eight_class_confusion_matrix(tmp_path):
    from src.training.trainer import Trainer
    model, _ = _model("weighted", 12)
    tr, va = _loaders(NC)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = Trainer(model, tr, va, dev, class_weights=CW, num_epochs=1, save_dir=str(tmp_path / "mc"), num_classes=NC)
    assert t.num_classes == NC
    for which, run in (("train", t.train_epoch), ("val", t.validate)):
        loss, m = run()
        conf = t.train_confusion if which == "train" else t.val_confusion
        assert np.isfinite(loss) and conf.shape == (NC, NC) and conf.dtype == np.int64
        assert int(conf.sum()) == 2 * B * G * G, which                      # two batches, every pixel labelled 0..7
        assert int((conf.sum(1) > 0).sum()) == NC, "every class occurs in the labels"
        assert len(m["class_iou"]) == NC and m["class_iou"] == MC.class_iou(conf)
        assert m["miou"] == float(np.mean(MC.class_iou(conf)))
    with pytest.raises(ValueError, match="class_weights"):
        Trainer(model, tr, va, dev, class_weights=[0.4, 3.5], num_epochs=1, save_dir=str(tmp_path / "bad"), num_classes=NC)


def test_trainer_without_the_argument_still_reports_two_classes(tmp_path):
    from src.training.trainer import Trainer
    model, _ = _model("weighted", 12, num_classes=2)
    tr, va = _loaders(None)
    t = Trainer(model, tr, va, torch.device("cuda", torch.cuda.current_device()), class_weights=[0.4, 3.5], num_epochs=1,
                save_dir=str(tmp_path / "two"))
    loss, m = t.train_epoch()
    assert t.num_classes is None and len(m["class_iou"]) == 2 and t.train_confusion.shape == (2, 2)
    assert m["class_iou"] == MC.class_iou(t.train_confusion)


def test_out_of_scope_paths_name_their_limit(tmp_path):
    from kdrt.bf16 import forward_bf16
    from kdrt.kd import KDStep
    from kdrt.lib import KDError
    from kdrt.losses import LovaszLoss, RegionLoss
    from kdrt.optim import FusedAdamW
    from src.training.trainer import Trainer
    images, pts, labels = (t.cuda() for t in _inputs())
    teacher, _ = _model("concat", 11)
    student, _ = _model("weighted", 12)
    student.train()
    cw = torch.tensor(CW).cuda()
    for spec in (RegionLoss(), LovaszLoss(), LovaszLoss(base=RegionLoss())):
        for fused in (True, False):
            opt = FusedAdamW(student.parameters(), lr=0.0, weight_decay=0.0)
            with pytest.raises(KDError, match="at most 4 classes"):
                KDStep(student, teacher, opt, cw, hard_loss=spec, fused_objective=fused)(images, pts, labels)
    opt = FusedAdamW(student.parameters(), lr=0.0, weight_decay=0.0)
    with pytest.raises(KDError, match="at most 4 classes"):
        KDStep(student, teacher, opt, cw, teacher_storage="bf16")
    teacher.eval()
    with pytest.raises(KDError, match="at most 4 classes"):
        forward_bf16(teacher, images, pts)
    x4, _ = _model("concat", 21, output_mode="x4")
    x4.eval()
    with pytest.raises(KDError, match="at most 4 classes"), torch.no_grad():
        x4(images, pts)
    with pytest.raises(KDError, match="at most 4 classes"):
        Trainer(student, None, None, torch.device("cuda", torch.cuda.current_device()), class_weights=CW, hard_loss=RegionLoss(),
                save_dir=str(tmp_path / "refused"), num_classes=NC)
    # and the step still runs afterwards: a refusal leaves nothing deposited
    opt = FusedAdamW(student.parameters(), lr=0.0, weight_decay=0.0)
    parts = KDStep(student, teacher, opt, cw)(images, pts, labels)
    assert bool(torch.isfinite(parts["total"]))


CLASS_MAP = {raw: (raw * 5) % NC for raw in range(2, 43)}       # raw ids 0, 1 and everything else -> background


@pytest.mark.parametrize("path", ["prepare_batch", "augmented", "staged"])
def test_loader_with_a_class_map_equals_the_rasteriser_on_the_mapped_labels(path):
    from kdrt.augment import Augment
    from src.data_loading.pandaset_dataset import StagingSet, SyntheticRawPandaSet, class_map_table
    ds = SyntheticRawPandaSet(n_frames=4, sweep_points=[400, 350, 0, 500], image_size=(HW, HW), grid_size=(G, G), max_points=600, seed=3,
                              nan_frames=(1,), class_map=CLASS_MAP)
    assert ds.num_classes == NC
    raws = [ds.load_raw(i) for i in range(4)]
    keys = [7, 8, 9, 10]
    if path == "prepare_batch":
        b = ds.prepare_batch(raws)
    elif path == "augmented":                               # an image-only setting: the points, and so the cells, keep their values
        b = ds.prepare_batch(raws, Augment(brightness=0.1), keys, 5)
    else:
        side = torch.cuda.Stream()
        b = ds.prepare_batch_staged(raws, StagingSet(), side, keys, 5)
        side.synchronize()
    torch.cuda.synchronize()
    seg = b["segmentation"].cpu().numpy()
    table = class_map_table(CLASS_MAP)
    assert seg.shape == (4, G, G) and seg.dtype == np.int64
    for i, r in enumerate(raws):
        ids = r["class"]
        mapped = np.where((ids >= 0) & (ids < table.size), table[np.clip(ids, 0, table.size - 1)], 0)
        want = D.rasterize_bev(r["x"], r["y"], mapped, (G, G), ds.pc_range)
        assert np.array_equal(seg[i], want.reshape(G, G)), (path, i)
    assert set(np.unique(seg)) <= set(range(NC)) and len(np.unique(seg)) > 4 and int(seg[2].sum()) == 0
    # without a map the same frames give the 2-class drivable mask, as before
    two = SyntheticRawPandaSet(n_frames=4, sweep_points=[400, 350, 0, 500], image_size=(HW, HW), grid_size=(G, G), max_points=600, seed=3,
                               nan_frames=(1,))
    seg2 = two.prepare_batch(raws)["segmentation"].cpu().numpy()
    for i, r in enumerate(raws):
        assert np.array_equal(seg2[i], D.rasterize_bev(r["x"], r["y"], D.remap_semantic(r["class"]), (G, G), two.pc_range).reshape(G, G))
