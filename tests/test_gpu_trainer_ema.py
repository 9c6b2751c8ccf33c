"""Trainer / KDTrainer with an EMA of the weights and parameter groups (ema_decay, no_decay_norm_bias), on the tiny PandaSet-shaped
tree of tests/_fake_pandaset.py: validation and the checkpoint's "ema_state" use the averaged weights and leave the live ones
alone bit for bit, a resumed run gets its EMA back, and with the options off the history and the checkpoint keep the
reference's layout."""
import json
import os

import pytest
import torch

import _fp64_optim_groups_ref as G
import _fp64_loss_ref as R
from _gpu_util import build_product
from test_gpu_tail_kernels import _check

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
REF_KEYS = ["train_loss", "train_miou", "val_loss", "val_miou", "lr"]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def loaders(tmp_path_factory):
    from _fake_pandaset import write_tree
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    root = str(tmp_path_factory.mktemp("data"))
    # no NaN points (they would poison train-mode BN) and no sweep above max_points (it would be cut to a random subset per pass)
    scenes = write_tree(root, n_points=(3000, 700), degenerate=False)
    return create_pandaset_dataloaders(root, scenes, scenes, batch_size=2, num_workers=0, verbose=False)


def _batches(loader):
    return [(b["image"].cuda(), b["points"].cuda(), b["segmentation"].cuda()) for b in loader]


def test_trainer_validates_and_checkpoints_the_ema(tmp_path, loaders, monkeypatch):
    from src.training.trainer import SegmentationMetrics, Trainer
    monkeypatch.delenv("KD_EMA_VALIDATE_LIVE", raising=False)
    tl, vl = loaders
    torch.manual_seed(0)
    tr = Trainer(build_product("weighted", 64), tl, vl, DEV, save_dir=str(tmp_path / "ck"), class_weights=[0.4, 3.5], num_epochs=2,
                 ema_decay=0.9, no_decay_norm_bias=True)
    opt = tr.optimizer
    assert opt.grouped and opt.ema_decay == 0.9 and [g["weight_decay"] for g in opt.param_groups] == [1e-3, 0.0]
    assert [id(q) for q in opt.flat.params] == [id(q) for q in tr.model.parameters()]
    tr.train()
    hist = json.load(open(tr.history_path))
    assert list(hist) == REF_KEYS + ["val_miou_live"] and hist["val_miou_live"] == [None, None] and len(hist["val_miou"]) == 2
    assert opt.dev_state[1].item() == 2.0 * len(tl) and not torch.equal(opt.ema, opt.flat.data)
    # validate() leaves the live weights alone, bit for bit, and reports the EMA model
    live = opt.flat.data.clone()
    ep = opt.epoch
    val_loss, vm = tr.validate()
    assert torch.equal(_bits(opt.flat.data), _bits(live)) and opt.epoch == ep + 2
    assert vm["miou"] == hist["val_miou"][-1]
    ckpt = torch.load(os.path.join(tr.save_dir, "latest.pth"), map_location=DEV)
    assert set(ckpt) == {"epoch", "model_state", "optimizer_state", "scheduler_state", "val_miou", "ema_state"}
    assert list(ckpt["ema_state"]) == list(ckpt["model_state"]) and len(ckpt["optimizer_state"]["param_groups"]) == 2
    for k, t in tr.model.state_dict().items():
        assert torch.equal(ckpt["model_state"][k], t), k             # "model_state" stays the live weights
    names = {n for n, _ in tr.model.named_parameters()}
    assert any(not torch.equal(ckpt["ema_state"][k], ckpt["model_state"][k]) for k in names)
    assert all(torch.equal(ckpt["ema_state"][k], ckpt["model_state"][k]) for k in ckpt["model_state"] if k not in names)    # buffers: copies
    # logits under swap_ema(): not the live ones, and bit for bit those of a fresh model loaded from "ema_state" (a stale eval
    # cache of the live weights would show here)
    fresh = build_product("weighted", 64)
    fresh.load_state_dict(ckpt["ema_state"])
    fresh.eval()
    tr.model.eval()
    vb = _batches(vl)
    metrics = SegmentationMetrics(num_classes=2, device=DEV)
    with torch.no_grad():
        live_logits = [tr.model(im, pts) for im, pts, _ in vb]
        with opt.swap_ema():
            ema_logits = [tr.model(im, pts) for im, pts, _ in vb]
        again = [tr.model(im, pts) for im, pts, _ in vb]
        for (im, pts, seg), a, b, c in zip(vb, live_logits, ema_logits, again):
            z = fresh(im, pts)
            assert not torch.equal(a, b), "the EMA logits equal the live ones: a stale cache, or no averaging"
            assert torch.equal(_bits(b), _bits(z)), "swap_ema() logits differ from a fresh model loaded from ema_state"
            assert torch.equal(_bits(a), _bits(c)), "the live logits did not come back after swap_ema()"
            metrics.update(z, seg)
    assert metrics.compute()["miou"] == hist["val_miou"][-1]
    assert ckpt["val_miou"] == hist["val_miou"][-1] and tr.best_miou == max(hist["val_miou"])
    # KD_EMA_VALIDATE_LIVE=1: a second pass on the live weights
    monkeypatch.setenv("KD_EMA_VALIDATE_LIVE", "1")
    tr.validate()
    live_metrics = SegmentationMetrics(num_classes=2, device=DEV)
    for (im, pts, seg), a in zip(vb, live_logits):
        live_metrics.update(a, seg)
    assert tr.last_val_miou_live == live_metrics.compute()["miou"] and torch.equal(_bits(opt.flat.data), _bits(live))
    monkeypatch.delenv("KD_EMA_VALIDATE_LIVE")
    # a resumed run gets its EMA back bit for bit; a checkpoint without "ema_state" starts the EMA from its weights
    torch.manual_seed(5)
    tr2 = Trainer(build_product("weighted", 64), tl, vl, DEV, save_dir=str(tmp_path / "ck2"), class_weights=[0.4, 3.5], num_epochs=2,
                  ema_decay=0.9, no_decay_norm_bias=True)
    assert not torch.equal(tr2.optimizer.ema, opt.ema)
    assert tr2.load_checkpoint(os.path.join(tr.save_dir, "latest.pth")) == 2
    o2 = tr2.optimizer
    assert torch.equal(_bits(o2.ema), _bits(opt.ema)) and torch.equal(_bits(o2.flat.data), _bits(live))
    assert torch.equal(o2.exp_avg, opt.exp_avg) and o2.dev_state[1].item() == opt.dev_state[1].item()
    del ckpt["ema_state"]
    torch.save(ckpt, str(tmp_path / "no_ema.pth"))
    o2.ema.fill_(7.0)
    tr2.load_checkpoint(str(tmp_path / "no_ema.pth"))
    assert torch.equal(_bits(o2.ema), _bits(live)) and torch.equal(_bits(o2.flat.data), _bits(live))


def test_kd_trainer_ema_matches_a_host_recomputation(tmp_path, loaders):
    from src.training.trainer import KDTrainer
    tl, vl = loaders
    torch.manual_seed(1)
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, DEV, save_dir=str(tmp_path / "kd"),
                   class_weights=[0.4, 3.5], num_epochs=1, ema_decay=0.9, no_decay_norm_bias=True)
    opt = kd.optimizer
    e64 = opt.ema.double()
    err = torch.zeros_like(e64)
    assert torch.equal(opt.ema, opt.flat.data)
    snaps, inner = [], kd._step

    def stepping(*a):
        out = inner(*a)
        snaps.append((opt.flat.data.clone(), opt.ema_state[0].item()))
        return out

    kd._step = stepping
    loss, _ = kd.train_epoch()
    assert loss == loss and len(snaps) == len(tl) >= 2
    for p_new, d in snaps:                                           # each step's bound, the earlier ones shrinking by d per step
        assert d == R.f32(0.9)
        e64, e_k = G.ema_update(e64, p_new.double(), d)
        err = d * err + e_k
    _check("KDTrainer EMA after one epoch", opt.ema, (e64, err))
    assert not torch.equal(opt.ema, opt.flat.data) and len(opt.param_groups) == 2
    assert kd.validate()[0] > 0


def test_options_off_keep_the_reference_layout(tmp_path, loaders):
    from src.training.trainer import Trainer
    tl, vl = loaders
    torch.manual_seed(2)
    tr = Trainer(build_product("weighted", 64), tl, vl, DEV, save_dir=str(tmp_path / "off"), class_weights=[0.4, 3.5], num_epochs=1)
    assert not tr.optimizer.grouped and tr.optimizer.ema is None and len(tr.optimizer.param_groups) == 1
    tr.train()
    assert list(json.load(open(tr.history_path))) == REF_KEYS
    ckpt = torch.load(os.path.join(tr.save_dir, "latest.pth"), map_location=DEV)
    assert set(ckpt) == {"epoch", "model_state", "optimizer_state", "scheduler_state", "val_miou"}
    with pytest.raises(RuntimeError, match="ema_decay"):
        tr.optimizer.swap_ema().__enter__()


def test_ema_starts_from_the_broadcast_weights(tmp_path, loaders, monkeypatch):
    """Data parallel: every rank's EMA must start from rank 0's weights, which arrive through the re-homed `.data` views AFTER the
    optimiser was built.  One rank, with the broadcast replaced by a write of other weights."""
    import src.training.trainer as T
    tl, vl = loaders

    def other_weights(module):
        with torch.no_grad():
            for t in list(module.parameters()) + list(module.buffers()):
                if t.is_floating_point():
                    t.data.mul_(0.5).add_(0.125)

    monkeypatch.setattr(T, "distributed", lambda: True)
    monkeypatch.setattr(T, "broadcast_module", other_weights)
    monkeypatch.setattr(T, "BucketedAllReduce", lambda *a, **k: None)
    monkeypatch.setattr(T.dist, "get_rank", lambda: 0)
    torch.manual_seed(3)
    model = build_product("weighted", 64)
    own = torch.cat([q.detach().flatten() for q in model.parameters()]).clone()
    tr = T.Trainer(model, tl, vl, DEV, save_dir=str(tmp_path / "dp"), class_weights=[0.4, 3.5], num_epochs=1, ema_decay=0.999,
                   no_decay_norm_bias=True)
    opt = tr.optimizer
    now = torch.cat([q.detach().flatten() for q in model.parameters()])
    assert torch.equal(now, own * 0.5 + 0.125), "the stand-in broadcast did not reach the parameters"
    assert torch.equal(_bits(opt.ema), _bits(opt.flat.data)), "the EMA does not start from the broadcast weights"
    sd = opt.ema_state_dict(model)
    assert all(torch.equal(sd[k], v) for k, v in model.state_dict().items())
