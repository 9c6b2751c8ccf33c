"""The opt-in channel-wise distillation feature term on the GPU: kd_feat_cwd_fwd_bwd (csrc/kd_loss_cwd.hip) called through the C ABI on
guarded buffers that start as NaN, against the float64 reference of tests/_fp64_cwd_ref.py: the column statistics, the value and
every gradient element within the reference's bound, no outlier allowance.  Then what the bound cannot show: exact zeros for
identical maps, uniform probabilities of constant columns, an image's bits independent of its batch, two calls with the same
bytes, every refusal before a launch; and the layers above: the autograd objective against the fused one, a KDStep eager /
graphed, the Lovasz combination, the KD trainer and the untouched default path."""
import pytest
import torch

import _fp64_cwd_ref as V
from _gpu_util import build_product
from test_gpu_region_loss import _inputs, _kd_step, _models, _same_bits
from test_gpu_tail_kernels import Buf, _check

pytestmark = pytest.mark.gpu

_CACHE = {}


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _call(s, t, tau, gcoef, gdev=None, grad=True, stats=True):
    """one call on guarded buffers -> (val Buf, ds Buf or None, stats Buf or None)"""
    lib, P, stream = _lib()
    B, HW, C = s.shape
    nbytes = lib.kd_feat_cwd_ws_bytes(B, HW, C)
    assert nbytes == V.ws_bytes(B, HW, C)
    ws, val = Buf(nbytes // 4), Buf(1)
    ds = Buf(B, HW, C) if grad else None
    sb = Buf(B, C, 4) if stats else None
    gd = None if gdev is None else torch.tensor([gdev], device="cuda")
    lib.call("kd_feat_cwd_fwd_bwd", P(s), P(t), B, HW, C, tau, gcoef, P(gd), P(val.t), P(ds.t) if grad else None,
             P(sb.t) if stats else None, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ws.guard_ok("ws"); val.guard_ok("val")
    for b, name in ((ds, "ds"), (sb, "stats")):
        if b is not None:
            b.guard_ok(name)
    return val, ds, sb


def _case(case):
    """inputs, call arguments and the float64 reference of a case, computed once and shared"""
    if case not in _CACHE:
        s, t, tau, gcoef, gdev, k = V.case_setup(case, "cuda")
        _CACHE[case] = (s, t, tau, gcoef, gdev, k, V.cwd(s.double(), t.double(), tau, k))
    return _CACHE[case]


def _report(what, name, got, ref):
    v, e = ref
    d = (got.double().reshape(v.shape) - v).abs()
    r = torch.where(d > 0, d / e.clamp_min(1e-300), torch.zeros_like(d))
    print(f"{what} {name}: worst |d|/bound {r.max().item():.3g}")


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_kernel_against_float64(case):
    s, t, tau, gcoef, gdev, k, ref = _case(case)
    what = V.case_id(case)
    val, ds, sb = _call(s, t, tau, gcoef, gdev)
    v, e = ref["val"]
    print(f"{what} val: got {val.t[0].item():.9g} float64 {v.item():.9g} |d|/bound {abs(val.t[0].item() - v.item()) / max(e.item(), 1e-300):.3g}")
    _report(what, "stats", sb.t, ref["stats"])
    _report(what, "ds", ds.t, ref["ds"])
    assert bool(torch.isfinite(v)) and bool(torch.isfinite(ref["ds"][0]).all())
    _check(f"cwd stats {what}", sb.t, ref["stats"])
    _check(f"cwd val {what}", val.t, (v.view(1), e.view(1)))
    _check(f"cwd ds {what}", ds.t, ref["ds"])
    assert bool(torch.isfinite(ds.t).all()) and val.t[0].item() >= 0.0
    if case[1] == 1:                                             # one position: phi = 1 on both sides
        assert val.t[0].item() == 0.0 and bool((ds.t == 0).all()) and bool((sb.t[..., 1::2] == 0).all())
    if case[4] == "spikes":
        assert bool((ref["phi_t"].float() == 0).any()), "the scene is there for teacher probabilities that underflow in fp32"


@pytest.mark.parametrize("case", [V.CASES[2], V.CASES[3]], ids=V.case_id)
def test_forward_only_no_stats_and_device_scale(case):
    """ds null: the same value and statistics; stats_out null: the same value and gradient; k = gcoef * gscale_dev[0] is ONE fp32
    product, so passing part of the coefficient on the device and folding it on the host give the same bits whenever the folded
    coefficient is that product (within the bound a fortiori: the folded call is checked against the reference as well)"""
    s, t, tau, gcoef, gdev, k, ref = _case(case)
    v0, g0, s0 = _call(s, t, tau, gcoef, gdev)
    vf, _, sf = _call(s, t, tau, gcoef, gdev, grad=False)
    assert _same_bits(v0.t, vf.t) and _same_bits(s0.t, sf.t)
    vn, gn, _ = _call(s, t, tau, gcoef, gdev, stats=False)
    assert _same_bits(v0.t, vn.t) and _same_bits(g0.t, gn.t)
    if gdev is None:
        v1, g1, _ = _call(s, t, tau, V.f32(gcoef * 4.0), 0.25)   # split by a power of two: the same fp32 product
    else:
        v1, g1, _ = _call(s, t, tau, V.f32(k), None)             # folded on the host
    _check("cwd ds, the coefficient passed the other way", g1.t, V.cwd(s.double(), t.double(), tau, V.f32(k))["ds"])
    assert _same_bits(g0.t, g1.t)
    assert _same_bits(v0.t, v1.t), "val is not scaled by the gradient coefficient"


@pytest.mark.parametrize("case", [V.CASES[0], V.CASES[2], V.CASES[3], V.CASES[4]], ids=V.case_id)
def test_identical_maps_give_exact_zeros(case):
    s, _, tau, gcoef, gdev, _, _ = _case(case)
    for t in (s.clone(), s):                                     # a bit-identical copy, and the same pointer
        val, ds, sb = _call(s, t, tau, gcoef, gdev)
        assert val.t[0].item() == 0.0 and bool((ds.t == 0).all())
        assert _same_bits(sb.t[..., :2].contiguous(), sb.t[..., 2:].contiguous())


def test_constant_columns_are_uniform():
    case = V.CASES[4]
    s, t, tau, gcoef, gdev, k, ref = _case(case)
    B, HW, C = s.shape
    _, _, sb = _call(s, t, tau, gcoef, gdev)
    logHW = torch.log(torch.tensor(float(HW), dtype=torch.float64))
    for c, x in ((0, 0.0), (1, 1.5 / tau)):
        for q in (0, 2):
            assert bool((sb.t[:, c, q] == x).all())
            d = (sb.t[:, c, q + 1].double() - logHW).abs()
            assert bool((d <= ref["stats"][1][:, c, q + 1]).all()), (d.tolist(), ref["stats"][1][:, c, q + 1].tolist())
    # a uniform phi on both sides: the gradient of such a column is exactly zero wherever the teacher's column is constant too
    _, ds, _ = _call(s, t, tau, gcoef, gdev)
    assert bool((ds.t[:, :, :2] == 0).all())
    # against a teacher column whose probabilities underflow everywhere but in row 0, k = 1: ds = phi(s) there, 1 / HW to the bit
    t2 = t.clone()
    t2[:, :, 0] = 0.0
    t2[:, 0, 0] = 1000.0
    _, ds2, _ = _call(s, t2, tau, 1.0, None)
    assert HW == 4096 and bool((ds2.t[:, 1:, 0] == 1.0 / HW).all()) and bool((ds2.t[:, 0, 0] == 1.0 / HW - 1.0).all())


@pytest.mark.parametrize("case", [V.CASES[2], V.CASES[6]], ids=V.case_id)
def test_an_image_alone_reproduces_its_bits(case):
    s, t, tau, gcoef, gdev, _, _ = _case(case)
    _, ds, sb = _call(s, t, tau, gcoef, gdev)
    for b in range(s.shape[0]):
        _, d1, s1 = _call(s[b:b + 1], t[b:b + 1], tau, gcoef, gdev)          # views into the batch: no copy, the same gcoef
        assert _same_bits(d1.t[0], ds.t[b]) and _same_bits(s1.t[0], sb.t[b]), b
        _, d2, s2 = _call(s[b:b + 1].clone(), t[b:b + 1].clone(), tau, gcoef, gdev)
        assert _same_bits(d2.t[0], ds.t[b]) and _same_bits(s2.t[0], sb.t[b]), b


@pytest.mark.parametrize("case", [V.CASES[1], V.CASES[3], V.CASES[4], V.CASES[5]], ids=V.case_id)
def test_two_calls_give_identical_bytes(case):
    s, t, tau, gcoef, gdev, _, _ = _case(case)
    a, b = _call(s, t, tau, gcoef, gdev), _call(s, t, tau, gcoef, gdev)
    for x, y in zip(a, b):
        assert _same_bits(x.t, y.t)


def test_refusals_return_before_a_launch_and_write_nothing():
    lib, P, stream = _lib()
    B, HW, C = 2, 16, 8
    s, t = V.cwd_inputs(B, HW, C, 1, "cuda")
    big = V.ws_bytes(B, HW, 516)
    ws, val, ds, sb = Buf(big // 4), Buf(1), Buf(B * HW * 516), Buf(B * 516 * 4)

    def rc(HW=HW, C=C, tau=1.0, nbytes=None):
        nb = V.ws_bytes(B, max(HW, 1), 8) if nbytes is None else nbytes
        r = lib.kd_feat_cwd_fwd_bwd(P(s), P(t), B, HW, C, tau, 1.0, None, P(val.t), P(ds.t), P(sb.t), P(ws.t), nb, stream())
        assert r == 0 or b"kd_feat_cwd_fwd_bwd" in lib.kd_last_error_string()
        return r
    assert rc(C=6) == -4 and rc(C=516, nbytes=big) == -4 and rc(HW=0) == -4                  # KD_ERR_SHAPE
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        assert rc(tau=tau) == -1, tau                                                        # KD_ERR_ARG
    assert rc(nbytes=V.ws_bytes(B, HW, C) - 1) == -3                                         # KD_ERR_WORKSPACE
    torch.cuda.synchronize()
    for b in (ws, val, ds, sb):
        assert bool(torch.isnan(b.buf[:b.n]).all())
        b.guard_ok("refused call")
    from kdrt import KDError
    from kdrt.losses import channel_kd
    a = torch.randn(1, 6, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(KDError, match="channels"):
        channel_kd(a, a.detach())
    with pytest.raises(KDError):
        channel_kd(torch.randn(1, 8, 4, 4, device="cuda"), torch.randn(1, 8, 4, 4))
    assert a.grad is None


def test_channel_kd_function():
    """the autograd.Function on NCHW maps: the value of the direct call, the gradient of a second call scaled by the upstream
    gradient on the device, as a channels-last view of the NHWC matrix"""
    from kdrt.losses import channel_kd
    B, HW, C, tau = 3, 60, 36, 2.0
    s, t = V.cwd_inputs(B, HW, C, 9, "cuda", "normal")
    val, ds, _ = _call(s, t, tau, V.f32(tau / (B * C)), 3.0)
    a = s.view(B, 6, 10, C).permute(0, 3, 1, 2).contiguous().requires_grad_()     # a contiguous NCHW copy
    b = t.view(B, 6, 10, C).permute(0, 3, 1, 2)                                   # channels-last: used in place
    loss = channel_kd(a, b, tau)
    assert _same_bits(loss.detach().view(1), val.t)
    (3.0 * loss).backward()
    assert _same_bits(a.grad.permute(0, 2, 3, 1).reshape(B, HW, C).contiguous(), ds.t)


# ---- the KD objective, the KD step and the trainer ----------------------------------------------------------------------------

PARTS = {"ce", "kl", "cwd_cam", "cwd_lidar", "total"}


def test_autograd_objective_and_fused_objective_give_the_same_bits():
    from kdrt.losses import ChannelKD
    spec = ChannelKD(2.0)
    (p0, g0, _), (p1, g1, _) = _kd_step(0.0, fused_objective=False, feature_loss=spec), _kd_step(0.0, fused_objective=True, feature_loss=spec)
    assert set(p0) == set(p1) == PARTS
    for k in p1:
        assert _same_bits(p0[k], p1[k]), (k, p0[k].item(), p1[k].item())
    assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
    assert _same_bits(g0, g1), (g0 - g1).abs().max().item()
    assert p1["cwd_cam"].item() > 0 and p1["cwd_lidar"].item() > 0
    # the term changes the step and leaves the logit terms alone; a beta that is no power of two keeps the same agreement
    pm, gm, _ = _kd_step(0.0, fused_objective=True)
    assert set(pm) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
    assert not _same_bits(gm, g1) and _same_bits(pm["ce"], p1["ce"]) and _same_bits(pm["kl"], p1["kl"])
    (p2, g2, _), (p3, g3, _) = _kd_step(0.0, fused_objective=False, feature_loss=ChannelKD(3.0), beta=0.7), _kd_step(0.0, fused_objective=True, feature_loss=ChannelKD(3.0), beta=0.7)
    assert _same_bits(g2, g3) and all(_same_bits(p2[k], p3[k]) for k in PARTS)
    want = p3["ce"].double() + 16.0 * p3["kl"].double() + float(V.f32(0.7)) * (p3["cwd_cam"].double() + p3["cwd_lidar"].double())
    assert abs(p3["total"].item() - want.item()) <= 4 * V.U * abs(want.item())


def test_kd_step_eager_and_graphed():
    from kdrt.losses import ChannelKD
    spec = ChannelKD()
    # three warm-up steps and three replays against six eager steps
    p_e, _, w_e = _kd_step(1e-3, steps=6, feature_loss=spec)
    p_g, _, w_g = _kd_step(1e-3, steps=6, graphed=3, feature_loss=spec)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "cwd_cam", "cwd_lidar"):
        assert bool(torch.isfinite(p_e[k])) and _same_bits(p_e[k], p_g[k]), k


def test_default_path_is_untouched_by_the_option(monkeypatch):
    """feature_loss=None and no argument at all leave the same parameter bytes, before and after a channel-KD step has run in
    the process, and make the library calls of the MSE objective: no channel-KD entry point, the parent commit's loss calls"""
    from kdrt.kd import KDStep
    from kdrt.lib import lib
    from kdrt.losses import ChannelKD
    from kdrt.optim import FusedAdamW
    images, pts, labels = _inputs()
    calls = []
    real = type(lib).call

    def spy(self, name, *a):
        calls.append(name)
        return real(self, name, *a)
    monkeypatch.setattr(type(lib), "call", spy)

    def run(how):
        student, teacher = _models()
        opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
        cw = torch.tensor([0.4, 3.5]).cuda()
        if how == "positional":
            step = KDStep(student, teacher, opt, cw, 4.0, 1.0, 1.0, -1, None, "fp32", True)
        elif how == "absent":
            step = KDStep(student, teacher, opt, cw)
        else:
            step = KDStep(student, teacher, opt, cw, feature_loss=how)
        assert step.feature_loss is (how if isinstance(how, ChannelKD) else None)
        del calls[:]
        for _ in range(2):
            parts = step(images, pts, labels)
        torch.cuda.synchronize()
        return torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone(), set(parts), list(calls)

    before, absent = run(None), run("absent")
    cwd = run(ChannelKD())
    after, pos = run(None), run("positional")
    assert before[2] == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"}
    for b in (absent, after, pos):
        assert _same_bits(before[0], b[0]) and _same_bits(before[1], b[1]) and before[2] == b[2] and before[3] == b[3]
    loss_calls = [c for c in before[3] if c in ("kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_kd_objective_final", "kd_kd_total", "kd_mse_fwd_bwd")]
    assert loss_calls == ["kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_mse_partial", "kd_kd_objective_final"] * 2
    assert not any("cwd" in c for c in before[3])
    # the option swaps exactly those calls
    assert [c for c in cwd[3] if c not in before[3]] == ["kd_feat_cwd_fwd_bwd", "kd_feat_cwd_fwd_bwd", "kd_kd_total"] * 2
    assert [c for c in cwd[3] if c in before[3]] == [c for c in before[3] if c not in ("kd_mse_partial", "kd_kd_objective_final")]
    assert not _same_bits(before[0], cwd[0])


def test_kd_trainer_with_channel_kd(tmp_path):
    from _fake_pandaset import write_tree
    from kdrt.losses import ChannelKD
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False)
    torch.manual_seed(1)
    spec = ChannelKD()
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"),
                   class_weights=[0.4, 3.5], num_epochs=1, feature_loss=spec)
    assert kd.kd_step.feature_loss is spec and kd.kd_step.hard_loss is None
    loss, _ = kd.train_epoch()
    assert loss == loss and abs(loss) < float("inf")
    assert kd.validate()[0] > 0                                   # validation is the hard-label loss, as before
