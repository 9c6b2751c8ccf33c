"""GPU tests of the drop-in training layer: Trainer (CE) and KDTrainer on synthetic PandaSet-shaped
batches -- loop runs, loss goes down, checkpoint dictionary keeps the reference's keys
(trainer.py:116-142) and round-trips, history JSON layout (trainer.py:144-152)."""
import json
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]


def _loaders(n=8, bs=4):
    from torch.utils.data import DataLoader
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    ds = SyntheticPandaSet(n_frames=n, num_points=1024, image_size=64, bev_size=16, seed=3, pad_tail=64)
    return DataLoader(ds, batch_size=bs, shuffle=False), DataLoader(ds, batch_size=bs, shuffle=False)


def _model(fusion, oc):
    from _gpu_util import build_product
    torch.manual_seed(0)
    return build_product(fusion, 16)


def test_trainer_ce_runs_and_checkpoints(tmp_path):
    from src.training.trainer import Trainer
    tl, vl = _loaders()
    model = _model("weighted", 128)
    tr = Trainer(model, tl, vl, torch.device("cuda"), lr=1e-3, weight_decay=1e-3, save_dir=str(tmp_path),
                 class_weights=[0.4, 3.5], num_epochs=3)
    l0, m0 = tr.train_epoch()
    for _ in range(4):
        l1, m1 = tr.train_epoch()
    assert l1 < l0, (l0, l1)
    vloss, vm = tr.validate()
    assert 0.0 <= vm["miou"] <= 1.0 and len(vm["class_iou"]) == 2
    tr.update_history(l1, m1["miou"], vloss, vm["miou"], 1e-3)
    hist = json.load(open(os.path.join(tmp_path, "training_history.json")))
    assert list(hist) == ["train_loss", "train_miou", "val_loss", "val_miou", "lr"]
    tr.save_checkpoint(0, vm["miou"], is_best=True)
    ck = torch.load(os.path.join(tmp_path, "best.pth"), map_location="cpu")
    assert set(ck) == {"epoch", "model_state", "optimizer_state", "scheduler_state", "val_miou"}
    st = ck["optimizer_state"]["state"]
    assert set(st[0]) == {"step", "exp_avg", "exp_avg_sq"}            # torch.optim.AdamW layout
    # resume into a fresh trainer: parameters, moments and step count come back
    model2 = _model("weighted", 128)
    tr2 = Trainer(model2, tl, vl, torch.device("cuda"), save_dir=str(tmp_path), class_weights=[0.4, 3.5], num_epochs=3)
    assert tr2.load_checkpoint(os.path.join(tmp_path, "best.pth")) == 1
    for (n1, p1), (n2, p2) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p1, p2), n1
    assert torch.equal(tr.optimizer.exp_avg, tr2.optimizer.exp_avg) and tr2.optimizer._step == tr.optimizer._step
    a, _ = tr.train_epoch()
    b, _ = tr2.train_epoch()
    assert abs(a - b) < 1e-5                                           # identical continuation
    # ... bit for bit: parameters, gradients, moments, device counters and every module buffer after the resumed epoch
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    for name in ("data", "grad"):
        assert torch.equal(bits(getattr(tr.optimizer.flat, name)), bits(getattr(tr2.optimizer.flat, name))), name
    for name in ("exp_avg", "exp_avg_sq", "dev_state"):
        assert torch.equal(bits(getattr(tr.optimizer, name)), bits(getattr(tr2.optimizer, name))), name
    assert tr.optimizer._step == tr2.optimizer._step == 12
    for (n1, b1), (_, b2) in zip(model.named_buffers(), model2.named_buffers()):
        assert torch.equal(bits(b1), bits(b2)), n1


def test_kd_trainer_runs(tmp_path):
    from src.training.trainer import KDTrainer
    tl, vl = _loaders()
    student, teacher = _model("weighted", 128), _model("concat", 256)
    tr = KDTrainer(student, teacher, tl, vl, torch.device("cuda"), T=4.0, alpha=1.0, beta=1.0, lr=1e-3,
                   weight_decay=1e-3, save_dir=str(tmp_path), class_weights=[0.4, 3.5], num_epochs=2)
    before = [p.detach().clone() for p in teacher.parameters()]
    l0, _ = tr.train_epoch()
    for _ in range(3):
        l1, _ = tr.train_epoch()
    assert l1 < l0
    assert all(torch.equal(a, b) for a, b in zip(before, teacher.parameters()))   # the teacher is frozen
    assert not teacher.training and student.training


def test_graphed_kd_step_matches_eager():
    """hipGraph capture of the whole KD step: N replays == N eager steps (parameters, Adam state, BN buffers)."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    B, HW, N, G = 2, 64, 512, 16
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    cw = torch.tensor([0.4, 3.5]).cuda()

    def make():
        teacher = build_product("concat", G); load_random_state(teacher, "concat", 11)
        student = build_product("weighted", G); load_random_state(student, "weighted", 12); student.train()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        return student, opt, KDStep(student, teacher, opt, cw)

    s_e, opt_e, step_e = make()
    for _ in range(6):                                   # 3 warm-up + 3: same count as the graphed run below
        out_e = step_e(images, pts, labels)
    s_g, opt_g, step_g = make()
    graphed = GraphedKDStep(step_g, images, pts, labels, warmup=3)
    for _ in range(3):
        out_g = graphed(images, pts, labels)
    torch.cuda.synchronize()
    assert opt_g._step == 6 and abs(float(opt_g.dev_state[1]) - 6.0) < 1e-6      # 3 warm-up + 3 replays, host and device agree
    assert abs(out_g["total"].item() - out_e["total"].item()) < 1e-5
    for (n1, p1), (_, p2) in zip(s_e.named_parameters(), s_g.named_parameters()):
        assert torch.allclose(p1, p2, atol=1e-6, rtol=1e-5), n1
    for (n1, b1), (_, b2) in zip(s_e.named_buffers(), s_g.named_buffers()):
        assert torch.allclose(b1.float(), b2.float(), atol=1e-6, rtol=1e-5), n1


def test_point_sort_is_shared_inside_one_kd_step_only(monkeypatch):
    """Teacher and student of one KD step sort the same point tensor ONCE; every step sorts again (nothing is carried
    over, so the bench's timed region contains the sort), and plain module calls outside a KD step never share."""
    import kd_oracle as O
    from _gpu_util import build_product, load_random_state
    from kdrt import units
    from kdrt.kd import KDStep
    from kdrt.lib import lib
    from kdrt.optim import FusedAdamW
    B, HW, N, G = 2, 64, 512, 16
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    teacher = build_product("concat", G); load_random_state(teacher, "concat", 11)
    student = build_product("weighted", G); load_random_state(student, "weighted", 12); student.train()
    opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
    step = KDStep(student, teacher.eval(), opt, torch.tensor([0.4, 3.5]).cuda())
    calls = []
    real = type(lib).call

    def counting(self, name, *a):
        calls.append(name)
        return real(self, name, *a)

    monkeypatch.setattr(type(lib), "call", counting)
    for expect in (1, 2, 3):
        step(images, pts, labels)
        assert calls.count("kd_lidar_sort_points") == expect
    assert not units._sort_cache and not units._sort_sharing
    calls.clear()
    with torch.no_grad():
        teacher(images, pts)
        teacher(images, pts)
    assert calls.count("kd_lidar_sort_points") == 2
