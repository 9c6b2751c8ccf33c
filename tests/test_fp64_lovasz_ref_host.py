"""CPU tests of the Lovasz-Softmax hard-label term's float64 reference (tests/_fp64_lovasz_ref.py) and of its host side: the
reference against a hand-computed case, against torch.sort + autograd on inputs whose sorted errors are separated, the
homogeneity identity, the two entries against each other; LovaszLoss validation, the ablation script's knobs, and the C ABI of
the two entry points (declared, exported, a monotone workspace query, every refusal before a launch)."""
import ctypes
import inspect
import math
import re

import pytest
import torch

import _fp64_lovasz_ref as V
from kdrt.losses import LovaszLoss, RegionLoss, lovasz_seg_loss          # ImportError without the feature


def test_reference_against_a_hand_computed_case():
    """B = 1, NC = 2, HW = 4; p_1 = (0.8, 0.6, 0.3, 0.1), labels (1, 0, 1, 0).
    Class 1: e = (0.2, 0.6, 0.7, 0.1), fg = (1, 0, 1, 0); sorted: pixel 2 (0.7, fg), 1 (0.6), 0 (0.2, fg), 3 (0.1); G = 2;
      (I, U) = (1, 2), (1, 3), (0, 3), (0, 4); J = 1/2, 2/3, 1, 1; g = 1/2, 1/6, 1/3, 0; L = 0.35 + 0.1 + 0.2/3 = 0.51666...
    Class 0: the same e, fg = (0, 1, 0, 1); sorted: pixel 2 (0.7), 1 (0.6, fg), 0 (0.2), 3 (0.1, fg); G = 2;
      (I, U) = (2, 3), (1, 3), (1, 4), (0, 4); J = 1/3, 2/3, 3/4, 1; g = 1/3, 1/3, 1/12, 1/4; L = 0.7/3 + 0.2 + 0.2/12 + 0.025 = 0.475
    L = (0.51666... + 0.475) / 2.  Pixel 2 (p = (0.7, 0.3), class 1): q_1 = -(1/2)/2, q_0 = +(1/3)/2, sum p q = 0.7/6 - 0.075 = 1/24,
    dL/dz_0 = 0.7 (1/6 - 1/24) = 0.0875 = -dL/dz_1."""
    p1 = torch.tensor([0.8, 0.6, 0.3, 0.1], dtype=torch.float64)
    zs = torch.stack([torch.log(1 - p1), torch.log(p1)]).view(1, 2, 4)
    y = torch.tensor([[1, 0, 1, 0]])
    r = V.lovasz(zs, y, -1, 1.0, 1.0)
    assert r["order"].tolist() == [[[2, 1, 0, 3], [2, 1, 0, 3]]]
    lbc = r["lbc"][0][0]
    assert abs(lbc[1].item() - (0.35 + 0.1 + 0.2 / 3)) < 1e-15 and abs(lbc[0].item() - 0.475) < 1e-15
    v = r["vals"][0]
    assert abs(v[0].item() - (0.35 + 0.1 + 0.2 / 3 + 0.475) / 2) < 1e-15
    assert abs(v[1].item() - 0.475) < 1e-15 and abs(v[2].item() - lbc[1].item()) < 1e-15
    g = r["dzs"][0]
    assert abs(g[0, 0, 2].item() - 0.0875) < 1e-15 and abs(g[0, 1, 2].item() + 0.0875) < 1e-15
    assert torch.allclose(r["dLde"][0, 1], torch.tensor([1 / 3, 1 / 6, 1 / 2, 0.0], dtype=torch.float64), atol=1e-15, rtol=0)
    assert torch.allclose(r["dLde"][0, 0], torch.tensor([1 / 12, 1 / 3, 1 / 3, 1 / 4], dtype=torch.float64), atol=1e-15, rtol=0)
    # weight, upstream gradient and the in/out hard-label term
    r2 = V.lovasz(zs, y, -1, 0.5, 3.0, hard0=0.25)
    assert abs(r2["hard"][0].item() - (0.25 + 0.5 * v[0].item())) < 1e-15
    assert torch.allclose(r2["dzs"][0], 1.5 * g, atol=1e-15, rtol=0)


def _autograd_lovasz(zs, y, ign):
    """Berman et al.'s lovasz_softmax (classes = 'present', per_image = True) with stock torch ops"""
    B, NC, HW = zs.shape
    p = torch.softmax(zs, 1)
    total = 0.0
    for b in range(B):
        keep = (y[b] != ign) & (y[b] >= 0) & (y[b] < NC)
        if not bool(keep.any()):
            continue
        losses = []
        for c in range(NC):
            fg = (y[b][keep] == c).to(zs.dtype)
            if fg.sum() == 0:
                continue
            err = (fg - p[b, c][keep]).abs()
            es, perm = torch.sort(err, descending=True)
            f = fg[perm]
            G = f.sum()
            inter = G - f.cumsum(0)
            union = G + (1 - f).cumsum(0)
            J = 1 - inter / union
            grad = torch.cat([J[:1], J[1:] - J[:-1]])
            losses.append(torch.dot(es, grad))
        total = total + sum(losses) / len(losses)
    return total / B


@pytest.mark.parametrize("B,NC,HW,seed", [(1, 2, 50, 0), (2, 3, 64, 1), (3, 4, 97, 2), (2, 2, 257, 3)])
def test_reference_against_torch_sort_and_autograd(B, NC, HW, seed):
    g = torch.Generator().manual_seed(seed)
    zs = (torch.randn(B, NC, HW, generator=g, dtype=torch.float64) * 2).requires_grad_()
    y = torch.randint(-1, NC + 1, (B, HW), generator=g)                  # -1: ignored, NC: out of range
    if B > 1:
        y[0][y[0] == NC - 1] = 0                                          # a class absent from one image
    r = V.lovasz(zs.detach(), y, -1, 1.0, 1.0)
    # the sorted errors are separated, so the order is beyond doubt
    gap = min((torch.sort(r["e"][b, c][r["order"][b, c][r["order"][b, c] >= 0]])[0].diff().min().item()
               for b in range(B) for c in range(NC) if bool(r["present"][b, c]) and int((r["order"][b, c] >= 0).sum()) > 1))
    print("smallest gap between sorted errors", gap)
    assert gap > 1e-9
    want = _autograd_lovasz(zs, y, -1)
    want.backward()
    assert abs(r["vals"][0][0].item() - want.item()) < 1e-14
    d = (r["dzs"][0] - zs.grad).abs().max().item()
    print("max |d| of the gradient", d)
    assert d < 1e-14
    keep = ((y >= 0) & (y < NC)).view(B, 1, HW)
    assert bool((r["dzs"][0][~keep.expand(B, NC, HW)] == 0).all())


def test_homogeneity_and_given_order_is_lovasz():
    zs, y = V.lovasz_inputs(3, 3, 1000, 5, "cpu", "absent")
    zs = zs.double()
    r = V.lovasz(zs, y, -1, V.f32(0.7), V.f32(2.5), hard0=0.5)
    lbc = r["lbc"][0]
    hom = (r["e"] * r["dLde"]).sum(2)                                     # L_{b,c} = sum_i e_i dL/de_i: positively homogeneous
    assert (hom - lbc).abs().max().item() < 1e-14
    assert bool((r["dLde"] >= -1e-15).all())
    s = r["dLde"].sum(2)
    assert torch.allclose(s[r["present"]], torch.ones_like(s[r["present"]]), atol=1e-12, rtol=0) and bool((s[~r["present"]] == 0).all())
    r2 = V.lovasz_given_order(zs, y, -1, V.f32(0.7), V.f32(2.5), r["order"], hard0=0.5)
    for k in ("vals", "hard", "dzs", "lbc"):
        assert torch.equal(torch.as_tensor(r[k][0]), torch.as_tensor(r2[k][0])) and torch.equal(torch.as_tensor(r[k][1]), torch.as_tensor(r2[k][1]))
    # a different order of distinct errors changes the gradient: the second entry really takes its order from the caller
    o = r["order"].clone()
    o[0, 0, :2] = o[0, 0, :2].flip(0)
    r3 = V.lovasz_given_order(zs, y, -1, V.f32(0.7), V.f32(2.5), o, hard0=0.5)
    assert not torch.equal(r3["dLde"], r["dLde"])


def test_lovasz_loss_validation():
    spec = LovaszLoss()
    assert spec.weight == 1.0 and spec.base is None
    with pytest.raises(Exception):
        spec.weight = 2.0
    assert LovaszLoss(0.5, RegionLoss(gamma=1.0)).base == RegionLoss(gamma=1.0)
    assert LovaszLoss(weight=2) == LovaszLoss(weight=2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1.0", True, None):
        with pytest.raises(ValueError):
            LovaszLoss(weight=bad)
    for bad in ("focal_tversky", LovaszLoss(), 1.0):
        with pytest.raises(ValueError):
            LovaszLoss(base=bad)
    # RegionLoss is what it was
    assert RegionLoss().args() == (2.0, 1.0, 1.0, 0.7, 0.3, 1.0)


def test_lovasz_seg_loss_refuses_cpu_tensors_and_other_specs():
    from kdrt import KDError
    z, y = torch.randn(2, 2, 4, 4, requires_grad=True), torch.zeros(2, 4, 4, dtype=torch.int64)
    with pytest.raises(KDError):
        lovasz_seg_loss(z, y, LovaszLoss())
    sig = inspect.signature(lovasz_seg_loss)
    assert list(sig.parameters) == ["logits", "target", "spec", "class_weights", "ignore_index", "teacher_logits", "T", "alpha"]
    assert [sig.parameters[k].default for k in ("class_weights", "ignore_index", "teacher_logits", "T", "alpha")] == [None, -1, None, 4.0, 1.0]


def test_ablation_script_reads_the_new_names_and_keeps_the_old():
    import train_with_fusion_ablation as S
    assert S.hard_loss_from_env({}) is None and S.hard_loss_from_env({"KD_HARD_LOSS": "ce"}) is None
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky"}) == RegionLoss()
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky", "KD_FOCAL_GAMMA": "1", "KD_LOVASZ_WEIGHT": "3"}) == RegionLoss(gamma=1.0)
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "ce_lovasz"}) == LovaszLoss(weight=1.0, base=None)
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "ce_lovasz", "KD_LOVASZ_WEIGHT": "0.25", "KD_FOCAL_GAMMA": "1"}) == LovaszLoss(weight=0.25)
    got = S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky_lovasz", "KD_LOVASZ_WEIGHT": "2", "KD_FOCAL_GAMMA": "1", "KD_TVERSKY_ALPHA": "0.5",
                                "KD_TVERSKY_BETA": "0.5"})
    assert got == LovaszLoss(weight=2.0, base=RegionLoss(gamma=1.0, a=0.5, b=0.5))
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky_lovasz"}) == LovaszLoss(base=RegionLoss())
    for bad in ({"KD_HARD_LOSS": "lovasz"}, {"KD_HARD_LOSS": "dice"}, {"KD_HARD_LOSS": "ce_lovasz", "KD_LOVASZ_WEIGHT": "0"},
                {"KD_HARD_LOSS": "focal_tversky_lovasz", "KD_FOCAL_GAMMA": "0.5"}):
        with pytest.raises(ValueError):
            S.hard_loss_from_env(bad)


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_seg_lovasz_fwd_bwd", "kd_seg_lovasz_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    V_, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert protos["kd_seg_lovasz_ws_bytes"] == (Z, [I, I, I])
    assert protos["kd_seg_lovasz_fwd_bwd"] == (I, [V_, V_, I, F, F, V_, V_, V_, V_, I, V_, I, I, I, V_, Z, V_])


def test_workspace_query_and_refusals_before_any_launch():
    from kdrt.lib import lib
    q = lib.kd_seg_lovasz_ws_bytes
    for B, NC, HW in ((1, 2, 1), (3, 4, 1000), (256, 2, 4096), (256, 2, 16384)):
        assert q(B, NC, HW) == V.ws_bytes(B, NC, HW)
        assert q(B + 1, NC, HW) > q(B, NC, HW) and q(B, NC + 1, HW) > q(B, NC, HW) and q(B, NC, HW + 1) > q(B, NC, HW)
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch

    def rc(zs=one, target=one, weight=1.0, vals=one, NC=2, HW=8, B=1, ws=one, ws_bytes=None):
        nb = q(B, NC, HW) if ws_bytes is None else ws_bytes
        return lib.kd_seg_lovasz_fwd_bwd(zs, target, -1, weight, 1.0, None, vals, None, one, 0, None, B, NC, HW, ws, nb, None)
    for kw in (dict(weight=0.0), dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(zs=None), dict(target=None),
               dict(vals=None)):
        assert rc(**kw) == -1, kw                                   # KD_ERR_ARG
        assert b"kd_seg_lovasz_fwd_bwd" in lib.kd_last_error_string()
    for kw in (dict(HW=V.MAX_HW + 1), dict(HW=1 << 20), dict(NC=1), dict(NC=5), dict(HW=0), dict(B=0)):
        assert rc(**kw) == -4, kw                                   # KD_ERR_SHAPE
        assert b"kd_seg_lovasz_fwd_bwd" in lib.kd_last_error_string()
    assert rc(ws_bytes=q(1, 2, 8) - 1) == -3 and rc(ws=None) == -3  # KD_ERR_WORKSPACE
    assert b"kd_seg_lovasz_fwd_bwd" in lib.kd_last_error_string()
    assert math.prod(V.layout(V.MAX_HW)[1:]) == V.MAX_HW and V.layout(V.MAX_HW)[0] * 8 == 128 * 1024


def test_entry_points_accept_the_type():
    from kdrt.losses import kd_objective, kd_objective_backward
    from src.training.trainer import Trainer
    for fn in (Trainer.__init__, kd_objective, kd_objective_backward):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "hard_loss" and p["hard_loss"].default is None, fn
