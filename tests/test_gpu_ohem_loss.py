"""The opt-in OHEM cross-entropy on the GPU: kd_seg_ohem_fwd_bwd (csrc/kd_loss_ohem.hip) called through the C ABI on guarded buffers
that start as NaN / sentinels, against tests/_ohem_ref.py.  Per case of _ohem_ref.CASES:
  1. the selection is exact given the device's own l: select(nll_out, ...) reproduces counts_out, the bits of theta and keep_out
     byte for byte -- in every scene;
  2. nll_out lies within the per-pixel bound e_lp of the float64 l;
  3. vals[0..3] and dzs lie within the bounds of the float64 reference evaluated over the DEVICE's kept set (the gradient is
     piecewise constant in the set), with no outlier allowance; dzs is exactly 0 at valid pixels outside S without a teacher;
  4. continuous and dropped-label scenes only: keep_out equals the float64-chosen set except at pixels inside the margin
     tests/test_ohem_ref_host.py bounds (at most 2 % of the valid pixels, asserted here again on the same numbers).
The tie, narrow-band, identical and all-ignored scenes are NOT part of check 4 -- fp32 and float64 legitimately split a tie group or
a band of a few ulps differently -- they are covered by checks 1 to 3 and by their known answers (|S| == n for identical pixels,
|S| > m for a rank inside a tie group, nothing kept and a NaN value for an all-ignored batch, one second-digit bucket for the
narrow band).  Then: keep-all parameters against kd_seg_loss_fwd_bwd, determinism, forward only, refusals, and the layers above:
ohem_seg_loss, the autograd objective against the fused one, a KDStep eager / graphed at 2 and 9 classes, the untouched default
path, and the Trainer."""
import json
import os

import numpy as np
import pytest
import torch

import _fp64_loss_ref as L
import _ohem_ref as R
import kd_oracle as O
from _gpu_util import build_product
from test_gpu_tail_kernels import Buf, _check

pytestmark = pytest.mark.gpu

IGUARD = 64
_CACHE = {}


class IBuf:
    """an integer output filled with a sentinel value followed by a guard of the same"""

    def __init__(self, n, dtype, fill):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + IGUARD,), fill, device="cuda", dtype=dtype)
        self.t = self.buf[:n]

    def guard_ok(self, what):
        assert bool((self.buf[self.n:] == self.fill).all()), f"{what}: written past its end"

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _call(tensors, a, grad=True, optional=True, rc_only=False, NC=None, ws_short=0, **over):
    """one call on guarded buffers -> dict of the buffers (vals, counts, dzs, nll, keep, ws); rc_only: the raw status instead of a raise"""
    lib, P, stream = _lib()
    zs, zt, y, cw = tensors
    a = {**a, **over}
    B, HW, npix = a["B"], a["HW"], a["npix"]
    NC = zs.shape[1] if NC is None else NC
    nbytes = lib.kd_seg_ohem_ws_bytes(npix)
    assert nbytes == R.ws_bytes(npix)
    o = {"ws": Buf(nbytes // 4), "vals": Buf(R.NVALS), "dzs": Buf(B, zs.shape[1], HW) if grad else None,
         "counts": IBuf(3, torch.int64, -77) if optional else None, "nll": Buf(npix) if optional else None,
         "keep": IBuf(npix, torch.uint8, 0x5A) if optional else None}
    gd = None if a["gdev"] is None else torch.tensor([a["gdev"]], device="cuda")
    p = lambda k: None if o[k] is None else P(o[k].t)
    args = (P(zs), P(zt), P(y), P(cw), a["ign"], a["T"], a["alpha"], a["gscale"], P(gd), a["lam"], a["min_kept"], a["min_divisor"],
            p("vals"), p("counts"), p("dzs"), p("nll"), p("keep"), B, NC, HW, p("ws"), nbytes - ws_short, stream())
    if rc_only:
        o["rc"] = lib.kd_seg_ohem_fwd_bwd(*args)
    else:
        lib.call("kd_seg_ohem_fwd_bwd", *args)
    torch.cuda.synchronize()
    for k, b in o.items():
        if k != "rc" and b is not None:
            b.guard_ok(k)
    return o


def _case(case):
    """inputs, scalars and the float64 per-pixel l of a case, computed once and shared"""
    if case not in _CACHE:
        tensors, a = R.case_setup(case, "cuda")
        zs, zt, y, cw = tensors
        valid, l64, e_l = R.per_pixel(zs.double(), y, a["ign"])
        _CACHE[case] = (tensors, a, valid, l64, e_l)
    return _CACHE[case]


def _d(t):
    return None if t is None else t.double()


def _run(case):
    (zs, zt, y, cw), a, valid, l64, e_l = _case(case)
    shape, NC, scene, teacher, weights, par = case
    what = R.case_id(case)
    B, HW = a["B"], a["HW"]
    o = _call((zs, zt, y, cw), a)
    vals, counts, dzs = o["vals"].t, o["counts"].t.tolist(), o["dzs"].t
    nll, keep_dev = o["nll"].t.view(B, HW), o["keep"].t.view(B, HW)
    n = int(valid.sum())

    # 1. the selection, exact on the device's own l
    assert bool((nll[~valid] == -1).all()) and bool((nll[valid] >= 0).all())
    assert bool((nll.view(torch.int32)[valid] >= 0).all()), "a kept l is stored with the sign bit clear"
    m, tau, theta, keep = R.select(nll, valid, a["lam"], a["min_kept"], a["min_divisor"])
    nkept = int(keep.sum())
    print(f"{what}: n {n} m {m} |S| {nkept} theta {float(theta):.9g} (tau {None if tau is None else float(tau)}, lambda {a['lam']:.9g}); device {counts}")
    assert counts == [n, m, nkept], (counts, [n, m, nkept])
    assert vals[4:5].view(torch.int32).item() == int(np.array([theta], np.float32).view(np.int32)[0]), (vals[4].item(), float(theta))
    assert np.array_equal(keep_dev.cpu().numpy().reshape(-1), keep.astype(np.uint8)), "keep_out is not the selection on nll_out"
    keep_t = keep_dev.bool()

    # 2. l against float64
    worst = ((nll.double() - l64).abs() / e_l)[valid].max().item() if n else 0.0
    print(f"{what} nll: worst |d|/bound {worst:.3g}")
    assert worst <= 1.0

    # 3. value and gradient over the device's S
    ref = R.ohem(zs.double(), _d(zt), y, _d(cw), a["ign"], a["T"], a["alpha"], a["gs"], keep_t, a["n_seq"])
    v, e = ref["vals"]
    for i, name in enumerate(("L", "kl", "sum_S w", "ce_all")):
        print(f"{what} {name}: got {vals[i].item():.9g} float64 {v[i].item():.9g} |d|/bound {((vals[i].double() - v[i]).abs() / e[i].clamp_min(1e-300)).item():.3g}")
    if n == 0:
        assert bool(torch.isnan(vals[0])) and bool(torch.isnan(vals[3])) and bool(torch.isnan(vals[5])), "0/0 like the CE"
        assert vals[2].item() == 0.0 and bool(torch.isnan(v[0]))
        _check(f"ohem kl {what}", vals[1:2], (v[1:2], e[1:2]))
    else:
        assert bool(torch.isfinite(v).all())
        _check(f"ohem vals {what}", vals[:4], (v, e))
        share = torch.tensor([nkept / n], dtype=torch.float64, device="cuda")
        _check(f"ohem kept share {what}", vals[5:6], (share, L._bound(1, share)))
    if not teacher:
        assert vals[1].item() == 0.0
    assert bool((vals[6:] == 0).all())
    g, eg = ref["dzs"]
    print(f"{what} dzs: worst |d|/bound {((dzs.double() - g).abs() / eg.clamp_min(1e-300)).max().item():.3g}")
    _check(f"ohem dzs {what}", dzs, (g, eg))
    if not teacher:
        off = (~keep_t).view(B, 1, HW).expand(B, NC, HW)
        assert bool((dzs[off] == 0).all()), "no teacher: the gradient outside S is exactly zero"
        if nkept:
            assert bool((dzs[~off] != 0).any())

    # 4. the kept set against float64's
    if scene in R.SET_SCENES:
        s = R.select64(l64, e_l, valid, a["lam"], a["min_kept"], a["min_divisor"])
        differ = keep_t.reshape(-1) != s["keep"]
        print(f"{what} set: {int(differ.sum())} pixels differ from float64's, {int(s['margin'].sum())} inside the margin ({s['share'] * 100:.3f} %)")
        assert s["share"] <= R.MARGIN_CAP
        assert not bool((differ & ~s["margin"]).any()), "a pixel outside the margin is kept by one of fp32 / float64 only"
        assert m == s["m"]

    # known answers
    if scene == "identical":
        assert nkept == n
    if scene == "ties":
        assert nkept > m and len(torch.unique(nll[valid])) <= 5 * NC
    if scene == "narrow":
        assert len(torch.unique(nll.view(torch.int32)[valid] >> 10)) == 1 and len(torch.unique(nll[valid])) > 1 and m <= nkept < n
    if scene == "ignored":
        assert counts == [0, 0, 0] and not bool(keep_t.any()) and vals[4].item() == np.float32(a["lam"])
    if par in R.KEEP_ALL:
        assert nkept == n and _same_bits(vals[3:4], vals[0:1])
    if par == "m1" and n:
        assert m == 1 and nkept >= 1 and bool((nll[valid].max() == nll[keep_t]).all())
    if par == "kept_cap":
        assert m == n
    if par == "mid" and scene in R.SET_SCENES:
        assert float(theta) == np.float32(a["lam"]) and nkept >= m, "the threshold decides"
    if par in ("rank", "third") and n:
        assert float(theta) == float(tau) < a["lam"], "the rank decides"
    return o


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_kernel_against_the_references(case):
    _run(case)


@pytest.mark.parametrize("case", [c for c in R.CASES if c[5] in R.KEEP_ALL] + [("ragged", 9, "dropped", True, True, "thresh1")], ids=R.case_id)
def test_keep_all_parameters_are_the_ce_call(case):
    """value, KL and gradient agree with kd_seg_loss_fwd_bwd within twice that call's float64 bound; the CE over K is the mined term"""
    lib, P, stream = _lib()
    if case in R.CASES:
        (zs, zt, y, cw), a = _case(case)[:2]
    else:                                                        # the same at the grid cap: the inputs of a ragged case, lambda = 0
        (zs, zt, y, cw), a = R.case_setup(("ragged", 16, "dropped", True, True, "rank"), "cuda")
        zs, zt, cw = zs[:, :9].contiguous(), zt[:, :9].contiguous(), cw[:9].contiguous()
        a = {**a, "lam": 0.0}
    B, NC, HW = zs.shape
    o = _call((zs, zt, y, cw), a)
    nbytes = lib.kd_seg_loss_ws_bytes(a["npix"])
    ws, losses, dce = Buf(nbytes // 4), Buf(3), Buf(B, NC, HW)
    gd = None if a["gdev"] is None else torch.tensor([a["gdev"]], device="cuda")
    lib.call("kd_seg_loss_fwd_bwd", P(zs), P(zt), P(y), P(cw), a["ign"], a["T"], a["alpha"], a["gscale"], P(gd), P(losses.t), P(dce.t),
             B, NC, HW, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    r = L.seg_loss(zs.double(), _d(zt), y, _d(cw), a["ign"], a["T"], a["alpha"], a["gs"], a["n_seq"])
    v, e = r["losses"]
    dv = (o["vals"].t[:3].double() - losses.t.double()).abs()
    print("values", o["vals"].t[:4].tolist(), losses.t.tolist(), (dv / e.clamp_min(1e-300)).tolist())
    assert bool((dv <= 2 * e).all()), (dv.tolist(), e.tolist())
    assert _same_bits(o["vals"].t[3:4], o["vals"].t[0:1])
    assert _same_bits(o["vals"].t[1:2], losses.t[1:2]), "the KL keeps the bits of the CE call"
    _check("dzs against the CE kernel", o["dzs"].t, (dce.t.double(), 2 * r["dzs"][1]))
    cnt = o["counts"].t.tolist()
    assert cnt[0] == cnt[2] == int(((y != a["ign"]) & (y >= 0) & (y < NC)).sum())


@pytest.mark.parametrize("case", [R.CASES[6], R.CASES[13], R.CASES[15]], ids=R.case_id)
def test_two_calls_give_identical_bytes_and_forward_only(case):
    tensors, a = _case(case)[:2]
    p, q = _call(tensors, a), _call(tensors, a)
    for k in ("vals", "dzs", "nll"):
        assert _same_bits(p[k].t, q[k].t), k
    assert torch.equal(p["counts"].t, q["counts"].t) and torch.equal(p["keep"].t, q["keep"].t)
    f = _call(tensors, a, grad=False)                             # dzs NULL: the same values, the same optional outputs
    assert _same_bits(p["vals"].t, f["vals"].t) and torch.equal(p["counts"].t, f["counts"].t) and torch.equal(p["keep"].t, f["keep"].t)
    b = _call(tensors, a, grad=False, optional=False)             # every optional output NULL
    assert _same_bits(p["vals"].t, b["vals"].t)
    g = _call(tensors, a, optional=False)
    assert _same_bits(p["vals"].t, g["vals"].t) and _same_bits(p["dzs"].t, g["dzs"].t)


def test_refusals_return_their_code_and_write_nothing():
    lib = _lib()[0]
    tensors, a = R.case_setup(R.CASES[3], "cuda")
    zs, zt, y, cw = tensors
    z17 = torch.randn(a["B"], 17, a["HW"], device="cuda")
    cw17 = torch.ones(17, device="cuda")
    for what, code, kw in (("NC = 17", -4, dict(tensors=(z17, None, y, cw17))), ("NC = 1", -4, dict(NC=1)),
                           ("min_divisor = 0", -1, dict(min_divisor=0)), ("min_kept = 0", -1, dict(min_kept=0)),
                           ("negative lambda", -1, dict(lam=-0.5)), ("infinite lambda", -1, dict(lam=float("inf"))),
                           ("NaN lambda", -1, dict(lam=float("nan"))), ("short workspace", -3, dict(ws_short=4))):
        t = kw.pop("tensors", tensors)
        o = _call(t, a, rc_only=True, **kw)
        assert o["rc"] == code and b"kd_seg_ohem_fwd_bwd" in lib.kd_last_error_string(), (what, o["rc"])
        for k in ("ws", "vals", "dzs", "nll"):
            assert bool(torch.isnan(o[k].buf[:o[k].n]).all()), (what, k)
        assert o["counts"].untouched() and o["keep"].untouched(), what


@pytest.mark.parametrize("NC", [2, 16])
def test_ohem_seg_loss_function(NC):
    """the autograd.Function: values of the direct call, gradient scaled by the upstream gradient on the device"""
    from kdrt import KDError
    from kdrt.losses import OhemCE, ohem_seg_loss
    B, HW, ign = 3, 1000, -1
    zs, zt, y, cw = R.ohem_inputs(B, NC, HW, 31 + NC, "cuda", "dropped", ign)
    spec = OhemCE(thresh=0.6, min_divisor=8, min_kept=5)
    a = {"B": B, "HW": HW, "npix": B * HW, "ign": ign, "T": 4.0, "alpha": 0.7, "gscale": 1.0, "gdev": 2.0, "lam": spec.lam(),
         "min_kept": 5, "min_divisor": 8}
    o = _call((zs, zt, y, cw), a)
    z4 = zs.view(B, NC, HW, 1).clone().requires_grad_()
    hard, kl, parts = ohem_seg_loss(z4, y.view(B, HW, 1), spec, cw, ign, zt.view(B, NC, HW, 1), 4.0, 0.7)
    assert set(parts) == {"ce_all", "theta", "kept"} and not any(p.requires_grad for p in parts.values()) and not kl.requires_grad
    got = torch.stack([hard.detach(), kl, parts["ce_all"], parts["theta"], parts["kept"]])
    assert _same_bits(got, o["vals"].t[[0, 1, 3, 4, 5]])
    assert parts["theta"].item() == np.float32(spec.lam()) and 0 < parts["kept"].item() < 1 and hard.item() > parts["ce_all"].item()
    (2.0 * hard).backward()
    assert _same_bits(z4.grad.view(B, NC, HW), o["dzs"].t)
    # without a teacher alpha is 0: no KL value, and the gradient is zero outside S
    z4 = zs.view(B, NC, HW, 1).clone().requires_grad_()
    hard2, kl2, _ = ohem_seg_loss(z4, y.view(B, HW, 1), spec, cw, ign)
    hard2.backward()
    assert _same_bits(hard2.detach(), hard.detach()) and kl2.item() == 0.0
    off = ~o["keep"].t.bool().view(B, 1, HW).expand(B, NC, HW)
    assert bool((z4.grad.view(B, NC, HW)[off] == 0).all())
    with pytest.raises(KDError, match="OhemCE"):
        ohem_seg_loss(z4, y.view(B, HW, 1), "ohem")


# ---- the KD objective, the KD step and the trainers ---------------------------------------------------------------------------

SHAPE = (2, 64, 700, 16)            # batch, image size, points, BEV grid: the smallest the unit tests of the KD objective use
CW9 = [0.4, 3.5, 1.0, 2.0, 0.7, 1.5, 3.0, 0.9, 1.2]


def _spec():
    from kdrt.losses import OhemCE
    return OhemCE(thresh=0.7, min_divisor=4, min_kept=8)


def _inputs(nc=2):
    B, HW, N, G = SHAPE
    images, pts, _ = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    labels = O.make_inputs(B, HW, N, HW // 4, 4, pad_tail=40, num_classes=nc)[2]          # labels live on the logits' grid
    return images.cuda(), pts.cuda(), labels.cuda()


def _models(nc=2):
    """teacher and student with name-keyed deterministic weights"""
    out = []
    for fusion, seed in (("concat", 11), ("weighted", 12)):
        m = build_product(fusion, SHAPE[3], num_classes=nc, device="cpu")
        st = O.randomize_state({k: v.detach().clone() for k, v in m.state_dict().items()}, seed)
        for k, v in m.state_dict().items():
            if k.endswith("grid_tensor"):
                st[k] = v.clone()
        m.load_state_dict(st)
        out.append(m.cuda())
    teacher, student = out
    student.train()
    return student, teacher


def _weights(nc):
    return torch.tensor([0.4, 3.5] if nc == 2 else CW9).cuda()


def _kd_step(lr, steps=1, graphed=0, nc=2, **kw):
    """`steps` eager KD steps (graphed: that many of them as replays after the capture's warm-up) -> (parts, flat gradient, flat parameters)"""
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    images, pts, labels = _inputs(nc)
    student, teacher = _models(nc)
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=0.0 if lr == 0 else 1e-3)
    step = KDStep(student, teacher, opt, _weights(nc), **kw)
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


PARTS = {"ce", "kl", "mse_cam", "mse_lidar", "total", "ce_all", "ohem_theta", "ohem_kept"}


@pytest.mark.parametrize("nc", [2, 9])
def test_autograd_objective_and_fused_objective_give_the_same_bits(nc):
    spec = _spec()
    (p0, g0, _), (p1, g1, _) = _kd_step(0.0, nc=nc, fused_objective=False, hard_loss=spec), _kd_step(0.0, nc=nc, fused_objective=True, hard_loss=spec)
    assert set(p0) == set(p1) == PARTS
    for k in p1:
        assert _same_bits(p0[k], p1[k]), (k, p0[k].item(), p1[k].item())
    assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
    assert _same_bits(g0, g1), (g0 - g1).abs().max().item()
    assert 0 < p1["ohem_kept"].item() < 1 and p1["ce"].item() > p1["ce_all"].item() > 0
    # the mined term changes the step and leaves the KL alone; the CE over every labelled pixel is the CE step's
    pc, gc, _ = _kd_step(0.0, nc=nc, fused_objective=True)
    assert set(pc) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
    assert not _same_bits(pc["ce"], p1["ce"]) and not _same_bits(gc, g1) and _same_bits(pc["kl"], p1["kl"])
    assert abs(pc["ce"].item() - p1["ce_all"].item()) <= 1e-5 * pc["ce"].item()


@pytest.mark.parametrize("nc", [2, 9])
def test_kd_step_eager_and_graphed(nc):
    spec = _spec()
    # three warm-up steps and two replays against five eager steps
    p_e, _, w_e = _kd_step(1e-3, steps=5, nc=nc, hard_loss=spec)
    p_g, _, w_g = _kd_step(1e-3, steps=5, graphed=2, nc=nc, hard_loss=spec)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "ce", "kl", "ce_all", "ohem_theta", "ohem_kept"):
        assert bool(torch.isfinite(p_e[k])) and _same_bits(p_e[k], p_g[k]), k


def test_default_path_is_untouched_by_the_option():
    """hard_loss=None, a plain RegionLoss and the positional construction of the parent commit leave the same bytes and the same
    parts before and after OHEM steps have run in between (the workspace and the histograms leave no state behind)"""
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    from kdrt.losses import RegionLoss
    images, pts, labels = _inputs()

    def run(how):
        student, teacher = _models()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        cw = _weights(2)
        if how == "positional":
            step = KDStep(student, teacher, opt, cw, 4.0, 1.0, 1.0, -1, None, "fp32", True)
        else:
            step = KDStep(student, teacher, opt, cw, hard_loss=how)
        for _ in range(2):
            parts = step(images, pts, labels)
        torch.cuda.synchronize()
        return torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone(), set(parts)

    region = RegionLoss(wt=0.8)
    before, before_r, before_p = run(None), run(region), run("positional")
    ohem = run(_spec())
    after, after_r, after_p = run(None), run(region), run("positional")
    assert before[2] == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"}
    assert before_r[2] == before[2] | {"focal", "tversky"} and ohem[2] == PARTS | {"logits"}
    for x, y in ((before, after), (before, before_p), (before, after_p), (before_r, after_r)):
        assert _same_bits(x[0], y[0]) and _same_bits(x[1], y[1]) and x[2] == y[2]
    assert not _same_bits(before[0], ohem[0])
    for bad in ("ohem", 0.7, type(_spec())):
        student, teacher = _models()
        with pytest.raises(ValueError, match="RegionLoss.*LovaszLoss.*OhemCE"):
            KDStep(student, teacher, FusedAdamW(student.parameters(), lr=1e-3), _weights(2), hard_loss=bad)


@pytest.mark.parametrize("nc", [2, 9])
def test_trainer_with_ohem(tmp_path, nc):
    from _fake_pandaset import write_tree
    from kdrt.losses import seg_loss
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer, Trainer
    spec = _spec()
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)
    mc = {} if nc == 2 else {"class_map": {raw: raw % nc for raw in range(2, 43)}}
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False, **mc)
    cw = [0.4, 3.5] if nc == 2 else CW9
    kw = {} if nc == 2 else {"num_classes": nc}
    torch.manual_seed(0)
    model = build_product("weighted", 64, num_classes=nc)
    tr = Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"), class_weights=cw, num_epochs=1, hard_loss=spec, **kw)
    assert tr.hard_loss is spec and tr.num_classes == (None if nc == 2 else nc)
    train_loss, tm = tr.train_epoch()
    val_loss, vm = tr.validate()
    tr.update_history(train_loss, tm["miou"], val_loss, vm["miou"], 1e-3)
    hist = json.load(open(os.path.join(tmp_path / "ck", "training_history.json")))
    assert hist["val_loss"] == [val_loss] and hist["train_loss"] == [train_loss]
    assert train_loss == train_loss and 0 < train_loss < float("inf") and 0 < val_loss < float("inf")
    # validate() reports the plain weighted CE of the evaluated weights, batch by batch: mining is a training device
    model.eval()
    total, n = 0.0, 0
    with torch.no_grad():
        for batch in vl:
            logits = model(batch["image"].cuda(), batch["points"].cuda())
            total += seg_loss(logits, batch["segmentation"].cuda(), tr.class_weights, -1)[0].item()
            n += 1
    assert abs(val_loss - total / n) <= 1e-6 * max(1.0, abs(val_loss)), (val_loss, total / n)
    for bad in ("ohem", 0.7, type(spec)):
        with pytest.raises(ValueError, match="RegionLoss.*LovaszLoss.*OhemCE"):
            Trainer(model, tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck3"), hard_loss=bad)
    # the KD trainer hands the option to its step; the epoch's loss is the objective with the mined term
    torch.manual_seed(1)
    kd = KDTrainer(build_product("weighted", 64, num_classes=nc), build_product("concat", 64, num_classes=nc), tl, vl, torch.device("cuda"),
                   save_dir=str(tmp_path / "ck4"), class_weights=cw, num_epochs=1, hard_loss=spec, **kw)
    assert kd.kd_step.hard_loss is spec
    kd_loss, _ = kd.train_epoch()
    assert kd_loss == kd_loss and abs(kd_loss) < float("inf") and kd.validate()[0] > 0
