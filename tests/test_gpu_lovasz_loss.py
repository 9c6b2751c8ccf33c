"""The opt-in Lovasz-Softmax hard-label term on the GPU: kd_seg_lovasz_fwd_bwd (csrc/kd_loss_lovasz.hip) called through the C ABI on
guarded buffers that start as NaN, against the float64 reference of tests/_fp64_lovasz_ref.py.  Per case: the order the device
sorted by is checked on its own (a permutation of the kept pixels, float64 errors decreasing along it up to the reference's
bound on them, bit-identical pixels in ascending index), then every output is held to the reference's bound along THAT order
(the gradient is piecewise constant in the order) and the value also to the reference's own order (the value is continuous across
a swap of near-equal errors).  No outlier allowance.  Then: accumulate / forward-only / no order output, determinism, and the
layers above: the autograd objective against the fused one, a KDStep eager / graphed, the Trainer, the refusal above 128 x 128
and the untouched default path."""
import json
import os

import pytest
import torch

import _fp64_lovasz_ref as V
from _gpu_util import build_product
from test_gpu_region_loss import _inputs, _kd_step, _models, _same_bits
from test_gpu_tail_kernels import Buf, _check

pytestmark = pytest.mark.gpu

NVALS = 5
IGUARD, ISENT, IFILL = 64, 0x5A5A5A5, -7
HARD0 = 0.75                     # what hard_inout holds before the call
_CACHE = {}


class IBuf:
    """an int32 output filled with IFILL followed by a guard of sentinels"""

    def __init__(self, *shape):
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.buf = torch.full((n + IGUARD,), IFILL, device="cuda", dtype=torch.int32)
        self.buf[n:] = ISENT
        self.t = self.buf[:n].view(*shape)

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == ISENT).all()), f"{what}: written past its end"


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _call(zs, y, ign, weight, gscale=1.0, gdev=None, grad=True, accumulate=0, prefill=None, order=True, hard=True):
    """one call on guarded buffers -> (vals Buf, hard Buf or None, dzs Buf or None, order IBuf or None)"""
    lib, P, stream = _lib()
    B, NC, HW = zs.shape
    nbytes = lib.kd_seg_lovasz_ws_bytes(B, NC, HW)
    assert nbytes == V.ws_bytes(B, NC, HW)
    ws, vals = Buf(nbytes // 4), Buf(NVALS)
    hb = Buf(1) if hard else None
    if hard:
        hb.t[0] = HARD0
    dzs = Buf(B, NC, HW) if grad else None
    if prefill is not None:
        dzs.t.copy_(prefill)
    ob = IBuf(B, NC, HW) if order else None
    gd = None if gdev is None else torch.tensor([gdev], device="cuda")
    lib.call("kd_seg_lovasz_fwd_bwd", P(zs), P(y), ign, weight, gscale, P(gd), P(vals.t), P(hb.t) if hard else None,
             P(dzs.t) if grad else None, accumulate, P(ob.t) if order else None, B, NC, HW, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ws.guard_ok("ws"); vals.guard_ok("vals")
    for b, name in ((hb, "hard"), (dzs, "dzs"), (ob, "order")):
        if b is not None:
            b.guard_ok(name)
    return vals, hb, dzs, ob


def _case_inputs(case):
    """inputs and call arguments of a case, the float64 reference along its own order computed once and shared"""
    if case not in _CACHE:
        HW, B, NC, scene = case
        i = V.CASES.index(case)
        ign = (-1, 255)[i % 2]
        zs, y = V.lovasz_inputs(B, NC, HW, 100 + i, "cuda", scene, ign)
        weight = V.f32((1.0, 0.7)[i % 2])
        gscale, gdev = ((1.0, None), (2.5, 0.5))[(i // 2) % 2]
        gs = V.f32(gscale) * (1.0 if gdev is None else V.f32(gdev))
        own = V.lovasz(zs.double(), y, ign, weight, gs, HARD0)
        _CACHE[case] = (zs, y, ign, weight, gscale, gdev, gs, own)
    return _CACHE[case]


def _check_order(what, zs, y, order, ref):
    """order [B, NC, HW] int64 from the device; ref: any reference result of the same inputs (its errors do not depend on the order)"""
    B, NC, HW = zs.shape
    e, e_e, present = ref["e"], ref["e_e"], ref["present"]
    keep = (ref["e_e"][:, 0] > 0)                                   # e_e carries TINY at every kept pixel
    for b in range(B):
        kept = torch.nonzero(keep[b]).flatten()
        n = kept.numel()
        for c in range(NC):
            o = order[b, c]
            if not bool(present[b, c]):
                assert bool((o == -1).all()), f"{what}: image {b} has no pixel of class {c}, its order must be -1"
                continue
            assert bool((o[n:] == -1).all()), f"{what} ({b}, {c}): -1 past the {n} kept pixels"
            idx = o[:n]
            assert torch.equal(torch.sort(idx)[0], kept), f"{what} ({b}, {c}): not a permutation of the kept pixels"
            es, ee = e[b, c, idx], e_e[b, c, idx]
            worst = ((es[1:] - es[:-1]) / (ee[1:] + ee[:-1])).max().item() if n > 1 else 0.0
            assert worst <= 1.0, f"{what} ({b}, {c}): the float64 errors rise along the order by {worst:.3g} x the bound on them"
            # bit-identical logits and the same fg: the same error bits, so ascending pixel index
            rows = torch.cat([zs[b][:, idx].t().contiguous().view(torch.int32), (y[b, idx] == c).to(torch.int32).view(n, 1)], 1)
            inv = torch.unique(rows, dim=0, return_inverse=True)[1]
            perm = torch.sort(inv, stable=True)[1]
            gi, ii = inv[perm], idx[perm]
            same = gi[1:] == gi[:-1]
            assert bool((ii[1:][same] > ii[:-1][same]).all()), f"{what} ({b}, {c}): equal errors out of pixel order"


def _run(case):
    zs, y, ign, weight, gscale, gdev, gs, own = _case_inputs(case)
    HW, B, NC, scene = case
    what = V.case_id(case)
    vals, hb, dzs, ob = _call(zs, y, ign, weight, gscale, gdev)
    order = ob.t.long()
    _check_order(what, zs, y, order, own)
    ref = V.lovasz_given_order(zs.double(), y, ign, weight, gs, order, HARD0)
    swaps = int((order != own["order"]).sum())
    v, e = ref["vals"]
    got = vals.t[:1 + NC].double()
    for i, name in enumerate(["L"] + [f"class{c}" for c in range(NC)]):
        print(f"{what} {name}: got {got[i].item():.9g} float64 {v[i].item():.9g} |d|/bound {((got[i] - v[i]).abs() / e[i].clamp_min(1e-300)).item():.3g}")
    h, eh = ref["hard"]
    print(f"{what} hard: got {hb.t[0].item():.9g} float64 {h.item():.9g} |d|/bound {(abs(hb.t[0].item() - h.item()) / max(eh.item(), 1e-300)):.3g}; "
          f"{swaps} positions ordered differently from float64")
    g, eg = ref["dzs"]
    print(f"{what} dzs: worst |d|/bound {((dzs.t.double() - g).abs() / eg.clamp_min(1e-300)).max().item():.3g}")
    assert bool(torch.isfinite(v).all())
    _check(f"lovasz vals {what}", vals.t[:1 + NC], (v, e))
    assert bool((vals.t[1 + NC:] == 0).all()), "classes past NC read 0"
    _check(f"lovasz hard {what}", hb.t, (h.view(1), eh.view(1)))
    _check(f"lovasz dzs {what}", dzs.t, (g, eg))
    # the value along the reference's own order
    vo, eo = own["vals"]
    print(f"{what} L, float64 order: |d|/bound {((got[0] - vo[0]).abs() / eo[0].clamp_min(1e-300)).item():.3g}")
    _check(f"lovasz value, float64 order {what}", vals.t[:1 + NC], (vo, eo))
    # dropped pixels and absent classes: exactly 0
    keep = ((y != ign) & (y >= 0) & (y < NC)).view(B, 1, HW).expand(B, NC, HW)
    assert bool((dzs.t[~keep] == 0).all()), "the gradient of a dropped pixel is exactly zero"
    absent = ~ref["present"]
    assert bool((vals.t[0] >= 0)) and bool((ref["lbc"][0][absent] == 0).all())
    if scene == "ignored":
        assert bool((dzs.t[B - 1] == 0).all()) and bool((order[B - 1] == -1).all())
        if B == 1:
            assert vals.t[0].item() == 0.0 and hb.t[0].item() == HARD0


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_kernel_against_float64(case):
    _run(case)


def test_accumulate_forward_only_and_no_order_output():
    """accumulate = 1 adds the accumulate = 0 result to what dzs holds with one rounded addition: equal TO THE BIT to
    fl32(pre-fill + result); dropped pixels keep the pre-fill.  dzs null: the same vals / hard, nothing else written.  order_out
    null: no output byte changes."""
    zs, y = V.lovasz_inputs(3, 3, 1000, 77, "cuda", "absent")
    w, gsc, gd = V.f32(0.7), 2.5, 0.5
    v0, h0, g0, o0 = _call(zs, y, -1, w, gsc, gd)
    pre = torch.randn(3, 3, 1000, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda") * g0.t.abs().max()
    v1, h1, g1, o1 = _call(zs, y, -1, w, gsc, gd, accumulate=1, prefill=pre)
    assert _same_bits(g1.t, pre + g0.t), (g1.t - (pre + g0.t)).abs().max().item()
    assert _same_bits(v0.t, v1.t) and _same_bits(h0.t, h1.t) and torch.equal(o0.t, o1.t)
    vf, hf, _, of = _call(zs, y, -1, w, gsc, gd, grad=False)
    assert _same_bits(v0.t, vf.t) and _same_bits(h0.t, hf.t) and torch.equal(o0.t, of.t)
    vn, hn, gn, _ = _call(zs, y, -1, w, gsc, gd, order=False)
    assert _same_bits(v0.t, vn.t) and _same_bits(h0.t, hn.t) and _same_bits(g0.t, gn.t)
    vh, _, gh, _ = _call(zs, y, -1, w, gsc, gd, hard=False)                    # hard_inout null
    assert _same_bits(v0.t, vh.t) and _same_bits(g0.t, gh.t)


@pytest.mark.parametrize("HW,NC,scene", [(1000, 4, "dups"), (4096, 2, "const"), (16384, 3, "random")])
def test_two_calls_give_identical_bytes(HW, NC, scene):
    zs, y = V.lovasz_inputs(3, NC, HW, 9, "cuda", scene)
    a, b = _call(zs, y, -1, 1.0, 2.5, 0.5), _call(zs, y, -1, 1.0, 2.5, 0.5)
    assert _same_bits(a[0].t, b[0].t) and _same_bits(a[1].t, b[1].t) and _same_bits(a[2].t, b[2].t) and torch.equal(a[3].t, b[3].t)


def test_above_the_cap_is_refused_and_writes_nothing():
    from kdrt import KDError
    from kdrt.losses import LovaszLoss, lovasz_seg_loss
    lib, P, stream = _lib()
    HW = V.MAX_HW + 1
    zs, y = V.lovasz_inputs(1, 2, HW, 3, "cuda")
    nbytes = lib.kd_seg_lovasz_ws_bytes(1, 2, HW)
    ws, vals, hb, dzs, ob = Buf(nbytes // 4), Buf(NVALS), Buf(1), Buf(1, 2, HW), IBuf(1, 2, HW)
    rc = lib.kd_seg_lovasz_fwd_bwd(P(zs), P(y), -1, 1.0, 1.0, None, P(vals.t), P(hb.t), P(dzs.t), 0, P(ob.t), 1, 2, HW, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    assert rc == -4 and b"kd_seg_lovasz_fwd_bwd" in lib.kd_last_error_string()
    for b in (ws, vals, hb, dzs):
        assert bool(torch.isnan(b.buf[:b.n]).all())
    assert bool((ob.t == IFILL).all())
    z4 = zs.view(1, 2, HW, 1).clone().requires_grad_()
    with pytest.raises(KDError, match="128 x 128"):
        lovasz_seg_loss(z4, y.view(1, HW, 1), LovaszLoss())
    assert z4.grad is None


def test_lovasz_seg_loss_function():
    """the autograd.Function over the CE and over a RegionLoss: value = base + weight * L of the direct calls, gradient = the base
    call's with the Lovasz gradient added by one rounded addition, scaled by the upstream gradient on the device"""
    from kdrt.losses import LovaszLoss, RegionLoss, lovasz_seg_loss, region_seg_loss, seg_loss
    B, NC, HW = 3, 3, 1000
    zs, y = V.lovasz_inputs(B, NC, HW, 21, "cuda", "absent")
    zt = torch.randn(B, NC, HW, generator=torch.Generator(device="cuda").manual_seed(2), device="cuda")
    cw = torch.tensor([0.4, 3.5, 1.0], device="cuda")
    w = 0.7
    vals, _, dl, _ = _call(zs, y, -1, V.f32(w), 1.0, 2.0, hard=False)
    for base in (None, RegionLoss(wt=0.8)):
        z4 = zs.view(B, NC, HW, 1).clone().requires_grad_()
        zb = zs.view(B, NC, HW, 1).clone().requires_grad_()
        hard, kl, parts = lovasz_seg_loss(z4, y.view(B, HW, 1), LovaszLoss(w, base), cw, -1, zt.view(B, NC, HW, 1), 4.0, 0.7)
        if base is None:
            bh, bkl = seg_loss(zb, y.view(B, HW, 1), cw, -1, zt.view(B, NC, HW, 1), 4.0, 0.7)
            assert set(parts) == {"lovasz", "class_lovasz"}
        else:
            bh, bkl, bp = region_seg_loss(zb, y.view(B, HW, 1), base, cw, -1, zt.view(B, NC, HW, 1), 4.0, 0.7)
            assert set(parts) == {"lovasz", "class_lovasz", "focal", "tversky"}
            assert _same_bits(parts["focal"], bp["focal"]) and _same_bits(parts["tversky"], bp["tversky"])
        assert _same_bits(parts["lovasz"], vals.t[0]) and _same_bits(parts["class_lovasz"], vals.t[1:1 + NC]) and _same_bits(kl, bkl)
        want = (bh.detach().double() + float(V.f32(w)) * parts["lovasz"].double())
        assert abs(hard.item() - want.item()) <= 2 * 2.0 ** -24 * abs(want.item()), (hard.item(), want.item())
        (2.0 * hard).backward()
        (2.0 * bh).backward()
        assert _same_bits(z4.grad.view(B, NC, HW), zb.grad.view(B, NC, HW) + dl.t)


# ---- the KD objective, the KD step and the trainers ---------------------------------------------------------------------------

def _specs():
    from kdrt.losses import LovaszLoss, RegionLoss
    return [LovaszLoss(weight=0.7), LovaszLoss(weight=1.5, base=RegionLoss(gamma=2.0, wf=1.0, wt=0.8, a=0.7, b=0.3, s=1.0))]


BASE_PARTS = {"ce", "kl", "mse_cam", "mse_lidar", "total", "lovasz"}


@pytest.mark.parametrize("which", [0, 1], ids=["ce_base", "region_base"])
def test_autograd_objective_and_fused_objective_give_the_same_bits(which):
    spec = _specs()[which]
    (p0, g0, _), (p1, g1, _) = _kd_step(0.0, fused_objective=False, hard_loss=spec), _kd_step(0.0, fused_objective=True, hard_loss=spec)
    want = BASE_PARTS | ({"focal", "tversky"} if which else set())
    assert set(p1) == want and set(p0) == want | {"class_lovasz"}
    for k in p1:
        assert _same_bits(p0[k], p1[k]), (k, p0[k].item(), p1[k].item())
    assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
    assert _same_bits(g0, g1), (g0 - g1).abs().max().item()
    assert 0 < p1["lovasz"].item() < 1
    # the term changes the step, and leaves the KL alone
    pc, gc, _ = _kd_step(0.0, fused_objective=True, hard_loss=spec.base)
    assert not _same_bits(pc["ce"], p1["ce"]) and not _same_bits(gc, g1) and _same_bits(pc["kl"], p1["kl"])
    hard = pc["ce"].double() + float(V.f32(spec.weight)) * p1["lovasz"].double()
    assert abs(p1["ce"].item() - hard.item()) <= 2 * 2.0 ** -24 * abs(hard.item())


@pytest.mark.parametrize("which", [0, 1], ids=["ce_base", "region_base"])
def test_kd_step_eager_and_graphed(which):
    spec = _specs()[which]
    # three warm-up steps and two replays against five eager steps
    p_e, _, w_e = _kd_step(1e-3, steps=5, hard_loss=spec)
    p_g, _, w_g = _kd_step(1e-3, steps=5, graphed=2, hard_loss=spec)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "ce", "lovasz"):
        assert bool(torch.isfinite(p_e[k])) and _same_bits(p_e[k], p_g[k]), k


def test_default_path_is_untouched_by_the_option():
    """hard_loss=None and a plain RegionLoss leave the bytes they leave without a Lovasz step having run in between (its
    workspace and LDS opt-in leave no state behind), and the bytes of the positional construction of the parent commit"""
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    from kdrt.losses import RegionLoss
    images, pts, labels = _inputs()

    def run(how):
        student, teacher = _models()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        cw = torch.tensor([0.4, 3.5]).cuda()
        if how == "positional":
            step = KDStep(student, teacher, opt, cw, 4.0, 1.0, 1.0, -1, None, "fp32", True)
        else:
            step = KDStep(student, teacher, opt, cw, hard_loss=how)
        for _ in range(2):
            parts = step(images, pts, labels)
        torch.cuda.synchronize()
        return torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone(), set(parts)

    region = RegionLoss(wt=0.8)
    before, before_r = run(None), run(region)
    for spec in _specs():
        run(spec)
    after, after_r, pos = run(None), run(region), run("positional")
    assert before[2] == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"}
    for a, b in ((before, after), (before, pos), (before_r, after_r)):
        assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and a[2] == b[2]


def test_trainer_with_lovasz_loss(tmp_path):
    from _fake_pandaset import write_tree
    from kdrt.losses import LovaszLoss, lovasz_seg_loss
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer, Trainer
    spec = _specs()[0]
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
    assert hist["val_loss"] == [val_loss]
    assert train_loss == train_loss and abs(train_loss) < float("inf") and val_loss == val_loss and 0 < val_loss < float("inf")
    # validate() reports the loss it trains with, batch by batch
    model.eval()
    total, n = 0.0, 0
    with torch.no_grad():
        for batch in vl:
            logits = model(batch["image"].cuda(), batch["points"].cuda())
            total += lovasz_seg_loss(logits, batch["segmentation"].cuda(), spec, tr.class_weights, -1)[0].item()
            n += 1
    assert abs(val_loss - total / n) <= 1e-6 * max(1.0, abs(val_loss)), (val_loss, total / n)
    for bad in ("ce_lovasz", 1.0, LovaszLoss):
        with pytest.raises(ValueError):
            Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck3"), hard_loss=bad)
    torch.manual_seed(1)
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck4"),
                   class_weights=[0.4, 3.5], num_epochs=1, hard_loss=_specs()[1])
    assert kd.kd_step.hard_loss == _specs()[1]
    kd_loss, _ = kd.train_epoch()
    assert kd_loss == kd_loss and abs(kd_loss) < float("inf") and kd.validate()[0] > 0
