"""The opt-in pair-wise distillation feature term on the GPU: kd_feat_pair_fwd_bwd (csrc/kd_loss_pair.hip) called through the C ABI on
guarded buffers that start as NaN, against the float64 direct form of tests/_fp64_pair_ref.py (explicit n x n affinities) with the
float32 Gram form as the yardstick of what fp32 costs.  Then what a bound cannot show: exact inputs bit for bit, exact zeros for
identical maps, the same bytes from two calls and from a graph replay, every refusal before a launch; and the layers above: the
autograd function, the autograd objective against the fused one, a KDStep eager / graphed, the KD trainer and the untouched
default path.

Measured on an MI355X (profiles/pair_kd_error.txt): the kernel's error against float64 stays below 4 x gram32's on every shape."""
import pytest
import torch

import _fp64_pair_ref as V
from _gpu_util import build_product
from test_gpu_region_loss import _inputs, _kd_step, _models, _same_bits
from test_gpu_tail_kernels import Buf

pytestmark = pytest.mark.gpu

# (B, H, W, Cs, Ct)
SHAPES = [(1, 1, 1, 4, 4), (1, 1, 2, 8, 8), (2, 8, 8, 8, 8), (3, 24, 24, 36, 36), (2, 24, 24, 128, 64), (2, 17, 9, 132, 256),
          (1, 64, 64, 128, 128)]
MANY_SLICES, ONE_SLICE = SHAPES[4], SHAPES[2]
_CACHE = {}


def _id(shape):
    return "B%d_%dx%d_Cs%d_Ct%d" % shape


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _call(s, t, gcoef, gdev=None, grad=True, img=True):
    """one call on guarded buffers -> (val Buf, ds Buf or None, img Buf or None)"""
    lib, P, stream = _lib()
    (B, HW, Cs), Ct = s.shape, t.shape[2]
    nbytes = lib.kd_feat_pair_ws_bytes(B, HW, Cs, Ct)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, val = Buf(nbytes // 4), Buf(1)
    ds = Buf(B, HW, Cs) if grad else None
    ib = Buf(B) if img else None
    gd = None if gdev is None else torch.tensor([gdev], device="cuda")
    lib.call("kd_feat_pair_fwd_bwd", P(s), P(t), B, HW, Cs, Ct, gcoef, P(gd), P(val.t), P(ds.t) if grad else None,
             P(ib.t) if img else None, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ws.guard_ok("ws"); val.guard_ok("val")
    for b, name in ((ds, "ds"), (ib, "img_vals_out")):
        if b is not None:
            b.guard_ok(name)
    return val, ds, ib


def _case(shape):
    """the maps, the float64 direct form and the float32 Gram form of a shape, computed once and shared"""
    if shape not in _CACHE:
        B, H, W, Cs, Ct = shape
        s, t = V.relu_maps(B, H * W, Cs, Ct, 1000 + H * W + Cs, "cuda")
        ref = V.direct(s.double(), t.double())
        g32 = {k: v.cuda() for k, v in V.gram32(s, t).items()}
        _CACHE[shape] = (s, t, ref, g32)
    return _CACHE[shape]


def _bounds(ref, f32):
    """(value, per-image values, gradient elements): 4 x the float32 Gram form's own distance from float64 + 8 U x the magnitude that
    cancels (tests/test_gpu_objective_matrix.py applies the same bounds to the term inside the KD objective)"""
    ev32, ei32, eg32 = (f32["val"] - ref["val"]).abs().item(), (f32["img"] - ref["img"]).abs(), (f32["grad"] - ref["grad"]).abs().max().item()
    return 4 * ev32 + 8 * V.U * ref["Sv"].item(), 4 * ei32 + 8 * V.U * ref["Sv_img"], 4 * eg32 + 8 * V.U * ref["M"]


def _float64_shape(shape):
    """-> the list of what is outside its bound for one shape (empty: inside), after printing every figure"""
    lib, _, _ = _lib()
    B, H, W, Cs, Ct = shape
    n = H * W
    if shape == MANY_SLICES:
        assert lib.kd_feat_pair_slices(B, n) > 1
    if shape == ONE_SLICE:
        assert lib.kd_feat_pair_slices(B, n) == 1
    s, t, ref, g32 = _case(shape)
    assert bool((s[:, n // 3] == 0).all()) and bool((t[:, (2 * n) // 3] == 0).all())
    val, ds, ib = _call(s, t, 4.0 / (B * float(n) * n))
    v64, g64 = ref["val"], ref["grad"]
    ev32, ei32, eg32 = (g32["val"] - v64).abs().item(), (g32["img"] - ref["img"]).abs(), (g32["grad"] - g64).abs().max().item()
    ev, ei, eg = abs(val.t[0].double().item() - v64.item()), (ib.t.double() - ref["img"]).abs(), (ds.t.double() - g64).abs()
    bound_v, bound_i, bound_g = _bounds(ref, g32)
    gmax = g64.abs().max().item()
    print(f"pair {_id(shape)}: val {val.t[0].item():.9g} float64 {v64.item():.9g} |d| {ev:.3g} gram32 {ev32:.3g} |d|/bound {ev / max(bound_v, 1e-300):.3g}"
          f" | img worst |d|/bound {(ei / bound_i.clamp_min(1e-300)).max().item():.3g}"
          f" | ds max |d| {eg.max().item():.3g} gram32 {eg32:.3g} ratio {eg.max().item() / max(eg32, 1e-300):.3g} worst |d|/bound "
          f"{(eg / bound_g.clamp_min(1e-300)).max().item():.3g} (largest entry {gmax:.3g})")
    bad = []
    if not (bool(torch.isfinite(ds.t).all()) and bool(torch.isfinite(val.t).all()) and bool(torch.isfinite(ib.t).all())):
        bad.append("not finite")
    if not ev <= bound_v:
        bad.append(("val", ev, bound_v))
    if not bool((ei <= bound_i).all()):
        bad.append(("img", ei.tolist(), bound_i.tolist()))
    if bool((eg > bound_g).any()):
        bad.append(("ds", int((eg > bound_g).sum()), (eg / bound_g.clamp_min(1e-300)).max().item()))
    if not bool((ds.t[:, n // 3] == 0).all()):
        bad.append("a zeroed row received a gradient")
    if n > 2 and not (val.t[0].item() > 0 and gmax > 0):
        bad.append("degenerate case")
    return bad


def test_float64():
    """every shape of SHAPES: value, per-image values and every gradient element inside the bound; all shapes are run and printed before
    the assertion, which names each shape that is outside"""
    bad = {_id(shape): b for shape in SHAPES for b in [_float64_shape(shape)] if b}
    assert not bad, bad


def test_exact_bits():
    """rows of one entry or of four equal ones, power-of-two norms, B, n and the coefficients powers of two: every normalised entry is
    +-1 or +-0.5 and every sum is exact in fp32, so the outputs are the float64 results rounded once -- which here is not at all"""
    lib, _, _ = _lib()
    for B, n, Cs, Ct, seed in ((2, 256, 8, 12, 3), (1, 64, 36, 36, 4), (4, 128, 128, 128, 5)):
        s, t = V.exact_maps(B, n, Cs, seed, "cuda"), V.exact_maps(B, n, Ct, seed + 50, "cuda")
        assert bool((s < 0).any()) and bool((s > 0).any())
        ref = V.direct(s.double(), t.double())
        gcoef, gscale = 4.0 / (B * n * n), 0.5
        assert V.f32(gcoef) == gcoef
        val, ds, ib = _call(s, t, gcoef, gscale)
        want = ref["grad"] * gscale
        assert torch.equal(want.float().double(), want) and ref["val"].item() > 0 and want.abs().max() > 0
        assert val.t[0].item() == ref["val"].float().item(), (val.t[0].item(), ref["val"].item())
        assert torch.equal(ib.t, ref["img"].float())
        assert torch.equal(ds.t, want.float()), (ds.t.double() - want).abs().max().item()
    assert lib.kd_feat_pair_slices(2, 256) > 1


def test_identical_zeros():
    lib, _, _ = _lib()
    for shape in (SHAPES[2], SHAPES[3], (2, 24, 24, 128, 128), (1, 17, 9, 256, 256)):
        B, H, W, Cs, Ct = shape
        s, _ = V.relu_maps(B, H * W, Cs, Ct, 77, "cuda")
        assert bool((s[:, (H * W) // 3] == 0).all())
        if H * W == 576:
            assert lib.kd_feat_pair_slices(B, H * W) > 1
        for t in (s.clone(), s):                                     # a bit-identical copy, and the same pointer
            val, ds, ib = _call(s, t, 1.0, 3.0)
            assert val.t[0].item() == 0.0 and bool((ib.t == 0).all()) and bool((ds.t == 0).all()), _id(shape)


def test_same_bytes():
    """two calls, a forward-only call, the coefficient folded on the host and a graph replay, on three shapes"""
    for shape in (SHAPES[3], SHAPES[4], SHAPES[5]):
        _same_bytes(shape)


def _same_bytes(shape):
    lib, P, stream = _lib()
    s, t, _, _ = _case(shape)
    (B, HW, Cs), Ct = s.shape, t.shape[2]
    a, b = _call(s, t, 0.37, 1.5), _call(s, t, 0.37, 1.5)
    for x, y in zip(a, b):
        assert _same_bits(x.t, y.t)
    vf, _, jf = _call(s, t, 0.37, 1.5, grad=False)
    assert _same_bits(a[0].t, vf.t) and _same_bits(a[2].t, jf.t)
    vn, dn, _ = _call(s, t, 0.37, 1.5, img=False)
    assert _same_bits(a[0].t, vn.t) and _same_bits(a[1].t, dn.t)
    v1, d1, _ = _call(s, t, V.f32(V.f32(0.37) * 1.5), None)      # k is ONE fp32 product: folded on the host it is the same coefficient
    assert _same_bits(a[0].t, v1.t) and _same_bits(a[1].t, d1.t)
    # a captured call, replayed on other inputs and then on these
    nbytes = lib.kd_feat_pair_ws_bytes(B, HW, Cs, Ct)
    ws, val, ds = Buf(nbytes // 4), Buf(1), Buf(B, HW, Cs)
    ss, ts, gd = s.clone(), t.clone(), torch.tensor([1.5], device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.call("kd_feat_pair_fwd_bwd", P(ss), P(ts), B, HW, Cs, Ct, 0.37, P(gd), P(val.t), P(ds.t), None, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(val.t).all()) and bool(torch.isnan(ds.t).all()), "capture must not execute"
    ss.copy_(s.flip(0) * 0.5 + 0.25)
    graph.replay()
    torch.cuda.synchronize()
    assert not _same_bits(ds.t, a[1].t)
    ss.copy_(s)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(val.t, a[0].t) and _same_bits(ds.t, a[1].t)
    for bf in (ws, val, ds):
        bf.guard_ok("replay")


def test_refusals():
    lib, P, stream = _lib()
    B, HW, C = 2, 16, 8
    s, t = V.relu_maps(B, HW, C, C, 1, "cuda")
    big = lib.kd_feat_pair_ws_bytes(B, HW, 256, 256)
    ws, val, ds, ib = Buf(big // 4), Buf(1), Buf(B * HW * 260), Buf(B)

    def rc(HW=HW, Cs=C, Ct=C, gcoef=1.0, nbytes=big, s_=s, ds_=None):
        r = lib.kd_feat_pair_fwd_bwd(P(s_), P(t), B, HW, Cs, Ct, gcoef, None, P(val.t), P(ds.t) if ds_ is None else ds_, P(ib.t), P(ws.t),
                                     nbytes, stream())
        assert r == 0 or b"kd_feat_pair_fwd_bwd" in lib.kd_last_error_string()
        return r
    assert rc(Cs=6) == -4 and rc(Ct=260) == -4 and rc(Cs=0) == -4 and rc(HW=0) == -4                  # KD_ERR_SHAPE
    for g in (float("nan"), float("inf")):
        assert rc(gcoef=g) == -1, g                                                                    # KD_ERR_ARG
    assert rc(nbytes=lib.kd_feat_pair_ws_bytes(B, HW, C, C) - 1) == -3                                 # KD_ERR_WORKSPACE
    assert rc(s_=s.view(-1)[1:]) == -2 and rc(ds_=P(ds.t.view(-1)[1:])) == -2                         # KD_ERR_ALIGN
    torch.cuda.synchronize()
    for b in (ws, val, ds, ib):
        assert bool(torch.isnan(b.buf[:b.n]).all())
        b.guard_ok("refused call")
    from kdrt import KDError
    from kdrt.losses import pair_kd
    a = torch.randn(1, 6, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(KDError, match="channels"):
        pair_kd(a, a.detach())
    with pytest.raises(KDError):
        pair_kd(torch.randn(1, 8, 4, 4, device="cuda"), torch.randn(1, 8, 4, 4))
    with pytest.raises(KDError):
        pair_kd(torch.randn(1, 8, 4, 4, device="cuda"), torch.randn(1, 8, 4, 5, device="cuda"))
    assert a.grad is None


def test_pair_kd():
    """the autograd.Function on NCHW maps of unequal widths: the value of the direct call, the gradient of a second call scaled by the
    upstream gradient on the device, as a channels-last view of the NHWC matrix; and both against the float64 direct form"""
    from kdrt.losses import pair_kd
    B, H, W, Cs, Ct = SHAPES[4]
    s, t, ref, g32 = _case(SHAPES[4])
    n = H * W
    val, ds, _ = _call(s, t, 4.0 / (B * n * n), 3.0)
    a = s.view(B, H, W, Cs).permute(0, 3, 1, 2).contiguous().requires_grad_()     # a contiguous NCHW copy
    b = t.view(B, H, W, Ct).permute(0, 3, 1, 2)                                   # channels-last: used in place
    loss = pair_kd(a, b)
    assert _same_bits(loss.detach().view(1), val.t)
    (3.0 * loss).backward()
    got = a.grad.permute(0, 2, 3, 1).reshape(B, n, Cs).contiguous()
    assert _same_bits(got, ds.t)
    eg32 = (g32["grad"] - ref["grad"]).abs().max().item()
    assert bool(((got.double() - 3.0 * ref["grad"]).abs() <= 3.0 * (4 * eg32 + 8 * V.U * ref["M"])).all())
    assert abs(loss.item() - ref["val"].item()) <= 4 * (g32["val"] - ref["val"]).abs().item() + 8 * V.U * ref["Sv"].item()


# ---- the KD objective, the KD step and the trainer ----------------------------------------------------------------------------

PARTS = {"ce", "kl", "pair_cam", "pair_lidar", "total"}


def test_objective_forms():
    """kd_objective(...).backward() against kd_objective_backward: the same parts and the same gradient bits, with beta = 0.7 and 0"""
    from kdrt.losses import PairKD
    for beta in (0.7, 0.0):
        (p0, g0, _), (p1, g1, _) = _kd_step(0.0, fused_objective=False, feature_loss=PairKD(), beta=beta), _kd_step(0.0, fused_objective=True, feature_loss=PairKD(), beta=beta)
        assert set(p0) == set(p1) == PARTS
        for k in p1:
            assert _same_bits(p0[k], p1[k]), (beta, k, p0[k].item(), p1[k].item())
        assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
        assert _same_bits(g0, g1), (beta, (g0 - g1).abs().max().item())
        assert p1["pair_cam"].item() > 0 and p1["pair_lidar"].item() > 0
        want = p1["ce"].double() + 16.0 * p1["kl"].double() + float(V.f32(beta)) * (p1["pair_cam"].double() + p1["pair_lidar"].double())
        assert abs(p1["total"].item() - want.item()) <= 4 * V.U * abs(want.item())
        # the term changes the step (with a beta that weighs it) and leaves the logit terms alone
        pm, gm, _ = _kd_step(0.0, fused_objective=True, beta=beta)
        assert set(pm) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
        assert _same_bits(pm["ce"], p1["ce"]) and _same_bits(pm["kl"], p1["kl"])
        assert _same_bits(gm, g1) == (beta == 0.0)


def test_step_graphed():
    from kdrt.losses import PairKD
    # three warm-up steps and three replays against six eager steps; beta large enough for the term to move the weights
    p_e, _, w_e = _kd_step(1e-3, steps=6, feature_loss=PairKD(), beta=50.0)
    p_g, _, w_g = _kd_step(1e-3, steps=6, graphed=3, feature_loss=PairKD(), beta=50.0)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "pair_cam", "pair_lidar"):
        assert bool(torch.isfinite(p_e[k])) and _same_bits(p_e[k], p_g[k]), k


def test_default_path(monkeypatch):
    """feature_loss=None leaves the same parameter bytes and makes the same library calls before and after a pair step has run in the
    process; the option swaps exactly the feature-term calls"""
    from kdrt.kd import KDStep
    from kdrt.lib import lib
    from kdrt.losses import PairKD
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
        step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5]).cuda(), feature_loss=how)
        assert step.feature_loss is how
        del calls[:]
        for _ in range(2):
            parts = step(images, pts, labels)
        torch.cuda.synchronize()
        return torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone(), set(parts), list(calls)

    before = run(None)
    pair = run(PairKD())
    after = run(None)
    assert before[2] == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"} and pair[2] == PARTS | {"logits"}
    assert _same_bits(before[0], after[0]) and _same_bits(before[1], after[1]) and before[2] == after[2] and before[3] == after[3]
    loss_calls = [c for c in before[3] if c in ("kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_kd_objective_final", "kd_kd_total", "kd_mse_fwd_bwd")]
    assert loss_calls == ["kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_mse_partial", "kd_kd_objective_final"] * 2
    assert not any("pair" in c or "cwd" in c for c in before[3])
    assert [c for c in pair[3] if c not in before[3]] == ["kd_feat_pair_fwd_bwd", "kd_feat_pair_fwd_bwd", "kd_kd_total"] * 2
    assert [c for c in pair[3] if c in before[3]] == [c for c in before[3] if c not in ("kd_mse_partial", "kd_kd_objective_final")]
    assert not _same_bits(before[0], pair[0])


def test_trainer(tmp_path):
    from _fake_pandaset import write_tree
    from kdrt.losses import PairKD
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False)
    torch.manual_seed(1)
    spec = PairKD()
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"),
                   class_weights=[0.4, 3.5], num_epochs=1, feature_loss=spec)
    assert kd.kd_step.feature_loss is spec and kd.kd_step.hard_loss is None
    loss, _ = kd.train_epoch()
    assert loss == loss and abs(loss) < float("inf")
    assert kd.validate()[0] > 0                                   # validation is the hard-label loss, as before
