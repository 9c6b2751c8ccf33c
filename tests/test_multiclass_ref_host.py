"""The float64 references of the loss, metric and classifier kernels have only been exercised up to 4 classes.  Here they are
checked at 5, 9 and 16 classes against torch's own float64 operators (F.cross_entropy, F.kl_div, bincount, F.conv2d + autograd),
so that tests/test_gpu_multiclass_kernels.py may use them as they are; the table remap reference is checked against numpy.  Also
the host side of the multi-class label path: class-map validation, the synthetic frames, the entry script's environment knobs."""
import inspect
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fp64_loss_ref as L
import _fp64_multiclass_ref as MC
import _fp64_tail_ref as R

NCS = (5, 9, 16)


def _close(a, b, what, rtol=1e-11, atol=1e-13):
    assert torch.allclose(a, b, rtol=rtol, atol=atol), (what, (a - b).abs().max().item())


@pytest.mark.parametrize("teacher", [True, False])
@pytest.mark.parametrize("weights", [True, False])
@pytest.mark.parametrize("NC", NCS)
def test_seg_loss_reference_equals_torch(NC, weights, teacher):
    B, HW, ign, T, alpha, gs = 3, 61, 255, 4.0, L.f32(0.7), 1.25
    zs, zt, y, cw = L.seg_inputs(B, NC, HW, 40 + NC, "cpu", ign, 3.0, weights, teacher)
    zs = zs.double().requires_grad_()
    zt, cw = (None if t is None else t.double() for t in (zt, cw))
    ref = L.seg_loss(zs.detach(), zt, y, cw, ign, T, alpha, gs, L.seg_n_seq(B * HW))
    yt = torch.where((y >= 0) & (y < NC), y, torch.full_like(y, ign))          # torch refuses labels outside the classes
    ce = F.cross_entropy(zs, yt, weight=cw, ignore_index=ign)
    kl = zs.new_zeros(())
    if teacher:
        kl = F.kl_div(F.log_softmax(zs / T, 1), F.softmax(zt / T, 1), reduction="sum") / (B * HW)
    (gs * (ce + alpha * T * T * kl)).backward()
    keep = yt != ign
    sw = (cw[yt[keep]].sum() if weights else keep.sum().double())
    val, err = ref["losses"]
    _close(val, torch.stack([ce.detach(), kl.detach(), sw]), "losses")
    _close(ref["dzs"][0], zs.grad, "dzs")
    assert bool((err >= 0).all()) and bool(torch.isfinite(err).all()) and bool((ref["dzs"][1] >= 0).all())
    # and the error model holds at this class count: a plain fp32 evaluation lies within the bound
    f = L.seg_loss(zs.detach().float(), None if zt is None else zt.float(), y, None if cw is None else cw.float(), ign, T, alpha, gs,
                   L.seg_n_seq(B * HW))
    assert bool(((f["losses"][0].double() - val).abs() <= err).all())
    assert bool(((f["dzs"][0].double() - ref["dzs"][0]).abs() <= ref["dzs"][1]).all())


@pytest.mark.parametrize("NC,M", [(5, 5), (9, 9), (16, 16), (16, 3), (3, 16)])
def test_confusion_reference_equals_argmax_and_bincount(NC, M):
    g = torch.Generator().manual_seed(NC * 17 + M)
    z = torch.randint(-2, 3, (3, NC, 97), generator=g).float() * 0.5           # a coarse grid: many exact ties
    y = torch.randint(-2, max(NC, M) + 2, (3, 97), generator=g)
    ign = 1
    pred, conf = L.confusion(z, y, M, ign)
    want = z.argmax(1)                                                          # the first maximum, as documented
    first = (z == z.amax(1, keepdim=True)).float().argmax(1)
    assert torch.equal(want, first) and torch.equal(pred, want)
    keep = (y != ign) & (y >= 0) & (y < M) & (want < M)
    assert torch.equal(conf, torch.bincount(y[keep] * M + want[keep], minlength=M * M).view(M, M))
    assert int(conf.sum()) == int(keep.sum()) > 0


@pytest.mark.parametrize("deferred", [True, False])
@pytest.mark.parametrize("Cin,NC", [(32, 5), (64, 9), (32, 16), (4, 16)])
def test_cls_conv_references_equal_conv2d_autograd(Cin, NC, deferred):
    B, H, W = 2, 5, 7
    M = B * H * W
    g = torch.Generator().manual_seed(Cin + NC)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, w, b, dl = r(M, Cin), r(NC, Cin), r(NC), r(M, NC)
    sc, sh, mean, inv = (r(Cin).abs() + 0.5, r(Cin) * 0.2, r(Cin) * 0.1, r(Cin).abs() + 0.5) if deferred else (None,) * 4
    z = (x * sc + sh if deferred else x.clone()).requires_grad_()
    xa = torch.relu(z) if deferred else z
    wp, bp = w.clone().requires_grad_(), b.clone().requires_grad_()
    img = xa.view(B, H, W, Cin).permute(0, 3, 1, 2)
    logits = F.conv2d(img, wp.view(NC, Cin, 1, 1), bp)
    fwd = R.cls_conv_fwd(x, sc, sh, R.RELU, w, b, B)["logits"]
    _close(fwd[0], logits.detach().reshape(B, NC, H * W), "logits")
    dlog = R.nchw_from_rows(dl, B)
    logits.backward(dlog.view(B, NC, H, W))
    ref = R.cls_conv_bwd(dlog, x, sc, sh, R.RELU, mean, inv, w, n_red=10, n_part=4)
    _close(ref["gx"][0], z.grad, "gx")
    _close(ref["dw"][0], wp.grad, "dw")
    _close(ref["db"][0], bp.grad, "db")
    if deferred:
        _close(ref["s1"][0], z.grad.sum(0), "s1")
        _close(ref["s2"][0], (z.grad * (x - mean) * inv).sum(0), "s2")
    for k, (val, err) in ref.items():
        assert val.shape == err.shape and bool((err >= 0).all()), k


def test_remap_table_reference_equals_numpy():
    g = torch.Generator().manual_seed(3)
    table = torch.randint(0, 16, (43,), generator=g)
    raw = torch.randint(-5, 60, (4001,), generator=g)
    raw[:4] = torch.tensor([-(2 ** 40), 2 ** 40, 42, 43])
    got = MC.remap_table(raw, table).numpy()
    r, t = raw.numpy(), table.numpy()
    want = np.where((r >= 0) & (r < 43), t[np.clip(r, 0, 42)], 0)
    assert np.array_equal(got, want) and want[2] == t[42] and want[3] == 0 and got.dtype == np.int64


def test_class_iou_reference():
    conf = np.array([[5, 1, 0], [2, 3, 0], [0, 0, 0]])
    assert MC.class_iou(conf) == [5 / 8, 3 / 6, 0.0]


# ---- the host side of the label path ----------------------------------------------------------------------------------------

def test_class_map_table_and_its_refusals():
    from src.data_loading.pandaset_dataset import MAX_CLASSES, class_map_table
    assert MAX_CLASSES == 16
    t = class_map_table({7: 1, 13: 2, 30: 15, 0: 0})
    assert t.dtype == np.int64 and t.shape == (31,) and t[7] == 1 and t[13] == 2 and t[30] == 15 and t.sum() == 18
    assert np.array_equal(class_map_table([0, 3, 3, 1]), np.array([0, 3, 3, 1]))
    assert np.array_equal(class_map_table(np.array([0, 2], np.int64)), np.array([0, 2]))
    for bad in ({}, [], {1: 16}, {1: -1}, {-1: 1}, {"7": 1}, {7: 1.0}, {7: True}, [0, 1.5], "0123", 5, {1: None}, [[0, 1]]):
        with pytest.raises(ValueError):
            class_map_table(bad)


def test_dataset_and_loader_signatures_take_a_class_map():
    from src.data_loading.pandaset_dataset import PandaSetDataset, SyntheticRawPandaSet, create_pandaset_dataloaders
    for fn in (PandaSetDataset.__init__, SyntheticRawPandaSet.__init__, create_pandaset_dataloaders):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "class_map" and p["class_map"].default is None, fn
    ds = SyntheticRawPandaSet(n_frames=2, sweep_points=10)
    assert ds.class_table is None and ds.num_classes == 2
    ds = SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map={3: 4, 9: 7})
    assert ds.num_classes == 8 and ds.class_table.shape == (10,)
    with pytest.raises(ValueError):
        SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map={3: 16})
    with pytest.raises(ValueError):
        create_pandaset_dataloaders("/nonexistent/pandaset", ["001"], ["002"], verbose=False, class_map={3: 99})
    tr, va = create_pandaset_dataloaders("/nonexistent/pandaset", ["001"], ["002"], verbose=False, class_map={3: 4, 9: 7})
    assert tr.dataset.num_classes == va.dataset.num_classes == 8


def test_synthetic_frames_with_more_classes():
    from src.data_loading.pandaset_dataset import SyntheticPandaSet
    a, b = SyntheticPandaSet(n_frames=3, num_points=300, image_size=32, bev_size=16, seed=5), \
        SyntheticPandaSet(n_frames=3, num_points=300, image_size=32, bev_size=16, seed=5, num_classes=2)
    c = SyntheticPandaSet(n_frames=3, num_points=300, image_size=32, bev_size=16, seed=5, num_classes=8)
    seen = set()
    for i in range(3):
        fa, fb, fc = a[i], b[i], c[i]
        for k in ("image", "points", "segmentation"):
            assert torch.equal(fa[k], fb[k]), k                  # the default IS two classes
        assert torch.equal(fa["image"], fc["image"]) and torch.equal(fa["points"], fc["points"])
        assert torch.equal(fc["segmentation"] > 0, fa["segmentation"] > 0)
        assert fc["segmentation"].dtype == torch.int64 and 0 <= int(fc["segmentation"].min()) and int(fc["segmentation"].max()) <= 7
        seen |= set(fc["segmentation"].unique().tolist())
    assert len(seen) > 4
    for bad in (1, 17, 2.0, True):
        with pytest.raises(ValueError):
            SyntheticPandaSet(num_classes=bad)


def test_trainer_takes_num_classes_by_keyword_and_keeps_its_argument_list():
    from src.training.trainer import KDTrainer, Trainer
    assert list(inspect.signature(Trainer.__init__).parameters)[-1] == "hard_loss"       # pinned by the region- and Lovasz-loss tests
    assert "num_classes" in inspect.signature(type(Trainer).__call__).parameters and type(KDTrainer) is type(Trainer)
    for bad in (1, 17, 2.5, True, "8"):
        with pytest.raises(ValueError, match="num_classes"):
            Trainer(None, None, None, None, num_classes=bad)                             # refused before anything is built


def test_ablation_script_multiclass_knobs(tmp_path):
    import train_with_fusion_ablation as A
    assert A.multiclass_from_env({}) == (None, None) and A.multiclass_from_env({"KD_NUM_CLASSES": "", "KD_CLASS_MAP": ""}) == (None, None)
    assert A.multiclass_from_env({"KD_NUM_CLASSES": "8"}) == (8, None)
    path = tmp_path / "map.json"
    path.write_text(json.dumps({"7": 1, "13": 2, "30": 5}))
    assert A.multiclass_from_env({"KD_CLASS_MAP": str(path)}) == (6, {7: 1, 13: 2, 30: 5})
    assert A.multiclass_from_env({"KD_CLASS_MAP": str(path), "KD_NUM_CLASSES": "9"}) == (9, {7: 1, 13: 2, 30: 5})
    for env in ({"KD_NUM_CLASSES": "17"}, {"KD_NUM_CLASSES": "1"}, {"KD_NUM_CLASSES": "x"}, {"KD_CLASS_MAP": str(path), "KD_NUM_CLASSES": "5"}):
        with pytest.raises(ValueError):
            A.multiclass_from_env(env)
    for text in ("[1, 2]", "{}", '{"a": 1}', '{"3": 16}', '{"3": 1.5}'):
        path.write_text(text)
        with pytest.raises(ValueError):
            A.multiclass_from_env({"KD_CLASS_MAP": str(path)})
    assert "KD_NUM_CLASSES" in A.__doc__ and "KD_CLASS_MAP" in A.__doc__
