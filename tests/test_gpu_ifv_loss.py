"""The opt-in intra-class feature variation distillation feature term on the GPU: kd_feat_ifv_fwd_bwd (csrc/kd_loss_ifv.hip) called
through the C ABI on guarded buffers that start as NaN, against the float64 direct form of tests/_fp64_ifv_ref.py with its plain
float32 evaluation (sums in pixel order) as the yardstick of what fp32 costs.  Then what a bound cannot show: exact inputs bit for
bit, exact zeros for identical maps, the same bytes from two calls and from a graph replay, every refusal before a launch; and the
layers above: the autograd function, the autograd objective against the fused one, a 5-class KDStep eager / graphed, the KD trainer
and the untouched default and PairKD paths.

Measured on an MI355X: profiles/ifv_kd_error.txt."""
import gc

import pytest
import torch

import _fp64_ifv_ref as V
import kd_oracle as O
from _gpu_util import build_product
from test_gpu_multiclass_step import B as MB, G as MG, HW as MHW, N as MN, _model
from test_gpu_region_loss import _inputs, _models, _same_bits
from test_gpu_tail_kernels import Buf

pytestmark = pytest.mark.gpu

# (B, H, W, Cs, Ct, NC)
SHAPES = [(1, 1, 1, 4, 4, 2), (1, 1, 2, 8, 8, 2), (2, 8, 8, 8, 8, 3), (3, 24, 24, 36, 36, 5), (2, 24, 24, 128, 64, 16),
          (2, 17, 9, 132, 256, 9), (1, 64, 64, 128, 128, 4)]
MANY_SLICES, ONE_SLICE = SHAPES[4], SHAPES[2]
_CACHE = {}


def _id(shape):
    return "B%d_%dx%d_Cs%d_Ct%d_NC%d" % shape


def _lib():
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    return lib, P, stream


def _call(s, t, y, NC, gcoef, gdev=None, grad=True, img=True, ignore=-1):
    """one call on guarded buffers -> (val Buf, ds Buf or None, img Buf or None)"""
    lib, P, stream = _lib()
    (B, HW, Cs), Ct = s.shape, t.shape[2]
    nbytes = lib.kd_feat_ifv_ws_bytes(B, HW, Cs, Ct, NC)
    assert nbytes > 0 and nbytes % 4 == 0
    ws, val = Buf(nbytes // 4), Buf(1)
    ds = Buf(B, HW, Cs) if grad else None
    ib = Buf(B) if img else None
    gd = None if gdev is None else torch.tensor([gdev], device="cuda")
    lib.call("kd_feat_ifv_fwd_bwd", P(s), P(t), P(y), ignore, B, HW, Cs, Ct, NC, gcoef, P(gd), P(val.t), P(ds.t) if grad else None,
             P(ib.t) if img else None, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    ws.guard_ok("ws"); val.guard_ok("val")
    for b, name in ((ds, "ds"), (ib, "img_vals_out")):
        if b is not None:
            b.guard_ok(name)
    return val, ds, ib


def _case(shape):
    """the maps, the labels, the float64 direct form and the float32 evaluation of a shape, computed once and shared"""
    if shape not in _CACHE:
        B, H, W, Cs, Ct, NC = shape
        s, t, y, plants = V.planted(B, H * W, Cs, Ct, NC, 1000 + H * W + Cs)
        ref = {k: v.cuda() for k, v in V.direct(s.double(), t.double(), y, NC).items()}
        y32 = {k: v.cuda() for k, v in V.ifv32(s, t, y, NC).items()}
        _CACHE[shape] = (s.cuda(), t.cuda(), y.cuda(), plants, ref, y32)
    return _CACHE[shape]


def _bounds(ref, f32):
    """(value, per-image values, gradient elements): 4 x the float32 evaluation's own distance from float64 + 8 U x the magnitude that
    cancels (tests/test_gpu_objective_matrix.py applies the same bounds to the term inside the KD objective)"""
    ev32, ei32, eg32 = (f32["val"] - ref["val"]).abs().item(), (f32["img"] - ref["img"]).abs(), (f32["grad"] - ref["grad"]).abs().max().item()
    return 4 * ev32 + 8 * V.U * ref["Sv"].item(), 4 * ei32 + 8 * V.U * ref["Sv_img"], 4 * eg32 + 8 * V.U * ref["M"]


def _float64_shape(shape):
    """-> the list of what is outside its bound for one shape (empty: inside), after printing every figure"""
    lib, _, _ = _lib()
    B, H, W, Cs, Ct, NC = shape
    n = H * W
    if shape == MANY_SLICES:
        assert lib.kd_feat_ifv_slices(B, n) > 1
    if shape == ONE_SLICE:
        assert lib.kd_feat_ifv_slices(B, n) == 1
    assert lib.kd_feat_ifv_slices(B, n) == V.slices(B, n)
    s, t, y, plants, ref, y32 = _case(shape)
    kept = V.kept_mask(y, NC)
    if n >= 64:                                                      # the planted cases are in the inputs
        assert {"zero", "single"} <= set(plants) and bool((y == -1).any()) and bool((y == NC).any())
        assert int((y[0] == plants["single"]).sum()) == 1 and bool((s[0, list(V.ZERO_ROWS)] == 0).all())
        assert ("absent" in plants and int((y[0] == plants["absent"]).sum()) == 0) or NC < 4
        assert B == 1 or not bool(kept[1].any())
        if shape == MANY_SLICES:
            lo, hi = plants["straddle"]
            assert hi == V.slice_rows(B, n) and y[0, lo] == y[0, hi] and bool(kept[0, lo])
    val, ds, ib = _call(s, t, y, NC, 2.0 / B)
    v64, g64 = ref["val"], ref["grad"]
    ev32, ei32, eg32 = (y32["val"] - v64).abs().item(), (y32["img"] - ref["img"]).abs(), (y32["grad"] - g64).abs().max().item()
    ev, ei, eg = abs(val.t[0].double().item() - v64.item()), (ib.t.double() - ref["img"]).abs(), (ds.t.double() - g64).abs()
    bound_v, bound_i, bound_g = _bounds(ref, y32)
    gmax = g64.abs().max().item()
    line = (f"ifv {_id(shape)}: val {val.t[0].item():.9g} float64 {v64.item():.9g} |d| {ev:.3g} ifv32 {ev32:.3g} |d|/bound {ev / max(bound_v, 1e-300):.3g}"
            f" | img worst |d|/bound {(ei / bound_i.clamp_min(1e-300)).max().item():.3g}"
            f" | ds max |d| {eg.max().item():.3g} ifv32 {eg32:.3g} ratio {eg.max().item() / max(eg32, 1e-300):.3g} worst |d|/bound "
            f"{(eg / bound_g.clamp_min(1e-300)).max().item():.3g} (largest entry {gmax:.3g})")
    print(line)
    bad = []
    if not (bool(torch.isfinite(ds.t).all()) and bool(torch.isfinite(val.t).all()) and bool(torch.isfinite(ib.t).all())):
        bad.append("not finite")
    if not ev <= bound_v:
        bad.append(("val", ev, bound_v))
    if not bool((ei <= bound_i).all()):
        bad.append(("img", ei.tolist(), bound_i.tolist()))
    if bool((eg > bound_g).any()):
        bad.append(("ds", int((eg > bound_g).sum()), (eg / bound_g.clamp_min(1e-300)).max().item()))
    if not bool((ds.t[~kept] == 0).all()):
        bad.append("a row that is not kept received a gradient")
    if n > 2 and not (val.t[0].item() > 0 and gmax > 0 and ds.t.abs().max().item() > 0):
        bad.append("degenerate case")
    return bad


def _part_float64():
    """every shape of SHAPES: value, per-image values and every gradient element inside the bound; all shapes are run and printed before
    the assertion, which names each shape that is outside"""
    bad = {_id(shape): b for shape in SHAPES for b in [_float64_shape(shape)] if b}
    assert not bad, bad


def _part_exact_bits():
    """tests/_fp64_ifv_ref.exact_inputs: prototypes that are unit vectors, similarities 0 or 1, counts and coefficients powers of two;
    the float64 result survives rounding to fp32 unchanged and the device must give it bit for bit"""
    lib, _, _ = _lib()
    for B, NC, N, extra, Cs, Ct, seed in ((2, 4, 16, 16, 8, 12, 3), (1, 2, 8, 0, 36, 36, 4), (4, 16, 64, 128, 128, 64, 5)):
        s, t, y = V.exact_inputs(B, NC, N, extra, Cs, Ct, seed, "cuda")
        ref = V.direct(s.double(), t.double(), y, NC)
        gcoef, gscale = 2.0 / B, 0.5
        assert V.f32(gcoef) == gcoef
        val, ds, ib = _call(s, t, y, NC, gcoef, gscale)
        want = ref["grad"] * gscale
        assert torch.equal(want.float().double(), want) and ref["val"].item() > 0 and want.abs().max() > 0
        assert ref["val"].float().double().item() == ref["val"].item()
        assert val.t[0].item() == ref["val"].item(), (val.t[0].item(), ref["val"].item())
        assert torch.equal(ib.t, ref["img"].float())
        assert torch.equal(ds.t, want.float()), (ds.t.double() - want).abs().max().item()
    assert lib.kd_feat_ifv_slices(4, 16 * 64 + 128) > 1


def _part_identical_zeros():
    lib, _, _ = _lib()
    for shape in (SHAPES[2], SHAPES[3], (2, 24, 24, 128, 128, 16), (1, 17, 9, 256, 256, 9)):
        B, H, W, Cs, Ct, NC = shape
        s, _, y, _ = V.planted(B, H * W, Cs, Ct, NC, 77, "cuda")
        if H * W == 576:
            assert lib.kd_feat_ifv_slices(B, H * W) > 1
        for t in (s.clone(), s):                                     # a bit-identical copy, and the same pointer
            val, ds, ib = _call(s, t, y, NC, 1.0, 3.0)
            assert val.t[0].item() == 0.0 and bool((ib.t == 0).all()) and bool((ds.t == 0).all()), _id(shape)


def _part_same_bytes():
    """two calls, a forward-only call, the coefficient folded on the host and a graph replay, on three shapes"""
    for shape in (SHAPES[3], SHAPES[4], SHAPES[5]):
        _same_bytes(shape)


def _same_bytes(shape):
    lib, P, stream = _lib()
    s, t, y, _, _, _ = _case(shape)
    (B, HW, Cs), Ct, NC = s.shape, t.shape[2], shape[5]
    a, b = _call(s, t, y, NC, 0.37, 1.5), _call(s, t, y, NC, 0.37, 1.5)
    for x, z in zip(a, b):
        assert _same_bits(x.t, z.t)
    vf, _, jf = _call(s, t, y, NC, 0.37, 1.5, grad=False)             # the value-only call
    assert _same_bits(a[0].t, vf.t) and _same_bits(a[2].t, jf.t)
    vn, dn, _ = _call(s, t, y, NC, 0.37, 1.5, img=False)
    assert _same_bits(a[0].t, vn.t) and _same_bits(a[1].t, dn.t)
    v1, d1, _ = _call(s, t, y, NC, V.f32(V.f32(0.37) * 1.5), None)     # k is ONE fp32 product: folded on the host it is the same coefficient
    assert _same_bits(a[0].t, v1.t) and _same_bits(a[1].t, d1.t)
    # a captured call, replayed on other inputs and then on these
    nbytes = lib.kd_feat_ifv_ws_bytes(B, HW, Cs, Ct, NC)
    ws, val, ds = Buf(nbytes // 4), Buf(1), Buf(B, HW, Cs)
    ss, ts, gd = s.clone(), t.clone(), torch.tensor([1.5], device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.call("kd_feat_ifv_fwd_bwd", P(ss), P(ts), P(y), -1, B, HW, Cs, Ct, NC, 0.37, P(gd), P(val.t), P(ds.t), None, P(ws.t), nbytes, stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(val.t).all()) and bool(torch.isnan(ds.t).all()), "capture must not execute"
    ss.copy_(s.flip(1) * 0.5 + 0.25)
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


def _part_refusals():
    lib, P, stream = _lib()
    B, HW, C, NC = 2, 16, 8, 3
    s, t, y, _ = V.planted(B, HW, C, C, NC, 1, "cuda")
    big = lib.kd_feat_ifv_ws_bytes(B, HW, 256, 256, 16)
    ws, val, ds, ib = Buf(big // 4), Buf(1), Buf(B * HW * 260), Buf(B)

    def rc(HW=HW, Cs=C, Ct=C, NC=NC, gcoef=1.0, nbytes=big, s_=s, ds_=None):
        r = lib.kd_feat_ifv_fwd_bwd(P(s_), P(t), P(y), -1, B, HW, Cs, Ct, NC, gcoef, None, P(val.t), P(ds.t) if ds_ is None else ds_, P(ib.t),
                                    P(ws.t), nbytes, stream())
        assert r == 0 or b"kd_feat_ifv_fwd_bwd" in lib.kd_last_error_string()
        return r
    assert rc(Cs=6) == -4 and rc(Ct=260) == -4 and rc(NC=1) == -4 and rc(NC=17) == -4 and rc(Cs=0) == -4 and rc(HW=0) == -4    # KD_ERR_SHAPE
    for g in (float("nan"), float("inf")):
        assert rc(gcoef=g) == -1, g                                                                    # KD_ERR_ARG
    assert rc(nbytes=lib.kd_feat_ifv_ws_bytes(B, HW, C, C, NC) - 1) == -3                              # KD_ERR_WORKSPACE
    assert rc(s_=s.view(-1)[1:]) == -2 and rc(ds_=P(ds.t.view(-1)[1:])) == -2                         # KD_ERR_ALIGN
    torch.cuda.synchronize()
    for b in (ws, val, ds, ib):
        assert bool(torch.isnan(b.buf[:b.n]).all())
        b.guard_ok("refused call")
    from kdrt import KDError
    from kdrt.losses import intra_class_kd
    a = torch.randn(1, 6, 4, 4, device="cuda", requires_grad=True)
    y4 = torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    with pytest.raises(KDError, match="channels"):
        intra_class_kd(a, a.detach(), y4, 3)
    a8 = torch.randn(1, 8, 4, 4, device="cuda", requires_grad=True)
    with pytest.raises(KDError):
        intra_class_kd(a8, torch.randn(1, 8, 4, 4), y4, 3)                                           # a CPU teacher
    with pytest.raises(KDError):
        intra_class_kd(a8, a8.detach().double(), y4, 3)
    with pytest.raises(KDError, match="label map"):
        intra_class_kd(a8, a8.detach(), torch.zeros(1, 16, 16, dtype=torch.int64, device="cuda"), 3)    # labels of an x4 head
    with pytest.raises(KDError, match="int64"):
        intra_class_kd(a8, a8.detach(), y4.int(), 3)
    for nc in (1, 17):
        with pytest.raises(KDError, match="classes"):
            intra_class_kd(a8, a8.detach(), y4, nc)
    assert a.grad is None and a8.grad is None


def _part_intra_class_kd():
    """the autograd.Function on NCHW maps of unequal widths: the value of the direct call, the gradient of a second call scaled by the
    upstream gradient on the device, as a channels-last view of the NHWC matrix; and both against the float64 direct form"""
    from kdrt.losses import intra_class_kd
    B, H, W, Cs, Ct, NC = SHAPES[4]
    s, t, y, _, ref, y32 = _case(SHAPES[4])
    n = H * W
    val, ds, _ = _call(s, t, y, NC, 2.0 / B, 3.0)
    a = s.view(B, H, W, Cs).permute(0, 3, 1, 2).contiguous().requires_grad_()     # a contiguous NCHW copy
    b = t.view(B, H, W, Ct).permute(0, 3, 1, 2)                                   # channels-last: used in place
    loss = intra_class_kd(a, b, y.view(B, H, W), NC)
    assert _same_bits(loss.detach().view(1), val.t)
    (3.0 * loss).backward()
    got = a.grad.permute(0, 2, 3, 1).reshape(B, n, Cs).contiguous()
    assert _same_bits(got, ds.t)
    eg32 = (y32["grad"] - ref["grad"]).abs().max().item()
    assert bool(((got.double() - 3.0 * ref["grad"]).abs() <= 3.0 * (4 * eg32 + 8 * V.U * ref["M"])).all())
    assert abs(loss.item() - ref["val"].item()) <= 4 * (y32["val"] - ref["val"]).abs().item() + 8 * V.U * ref["Sv"].item()
    # another ignore_index: the pixels labelled 0 leave, the pixels labelled -1 stay out of range
    v0, _, _ = _call(s, t, y, NC, 2.0 / B, 3.0, ignore=0)
    l0 = intra_class_kd(a.detach(), b, y.view(B, H, W), NC, ignore_index=0)
    assert _same_bits(l0.view(1), v0.t) and not _same_bits(v0.t, val.t)


# ---- the KD objective, the KD step and the trainer ----------------------------------------------------------------------------

PARTS = {"ce", "kl", "ifv_cam", "ifv_lidar", "total"}
NC5 = 5
CW5 = [0.4, 3.5, 1.0, 2.0, 0.7]


def _kd_step5(lr, steps=1, graphed=0, labels=None, **kw):
    """`steps` KD steps of the 5-class weighted student under the 5-class concat teacher (the small models of
    tests/test_gpu_multiclass_step.py) -> (parts, flat gradient, flat parameters)"""
    from kdrt.kd import GraphedKDStep, KDStep
    from kdrt.optim import FusedAdamW
    images, pts, _ = O.make_inputs(MB, MHW, MN, MG, 2, pad_tail=40)
    if labels is None:
        labels = O.make_inputs(MB, MHW, MN, MHW // 4, 2, pad_tail=40, num_classes=NC5)[2]
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    teacher, _ = _model("concat", 11, num_classes=NC5)
    student, _ = _model("weighted", 12, num_classes=NC5)
    student.train()
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=0.0 if lr == 0 else 1e-3)
    step = KDStep(student, teacher, opt, torch.tensor(CW5).cuda(), **kw)
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


def _part_objective_forms():
    """kd_objective(...).backward() against kd_objective_backward with 5 classes: the same parts and the same gradient bits, with
    beta = 0.7 and 0"""
    from kdrt.losses import IntraClassKD
    for beta in (0.7, 0.0):
        (p0, g0, _), (p1, g1, _) = (_kd_step5(0.0, fused_objective=False, feature_loss=IntraClassKD(), beta=beta),
                                    _kd_step5(0.0, fused_objective=True, feature_loss=IntraClassKD(), beta=beta))
        assert set(p0) == set(p1) == PARTS
        for k in p1:
            assert _same_bits(p0[k], p1[k]), (beta, k, p0[k].item(), p1[k].item())
        assert bool(torch.isfinite(g1).all()) and g1.abs().max() > 0
        assert _same_bits(g0, g1), (beta, (g0 - g1).abs().max().item())
        assert p1["ifv_cam"].item() > 0 and p1["ifv_lidar"].item() > 0
        want = p1["ce"].double() + 16.0 * p1["kl"].double() + float(V.f32(beta)) * (p1["ifv_cam"].double() + p1["ifv_lidar"].double())
        assert abs(p1["total"].item() - want.item()) <= 4 * V.U * abs(want.item())
        # the term changes the step (with a beta that weighs it) and leaves the logit terms alone
        pm, gm, _ = _kd_step5(0.0, fused_objective=True, beta=beta)
        assert set(pm) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
        assert _same_bits(pm["ce"], p1["ce"]) and _same_bits(pm["kl"], p1["kl"])
        assert _same_bits(gm, g1) == (beta == 0.0)


def _part_step_graphed():
    from kdrt.losses import IntraClassKD
    # three warm-up steps and three replays against six eager steps; beta large enough for the term to move the weights
    p_e, _, w_e = _kd_step5(1e-3, steps=6, feature_loss=IntraClassKD(), beta=5.0)
    p_g, _, w_g = _kd_step5(1e-3, steps=6, graphed=3, feature_loss=IntraClassKD(), beta=5.0)
    print("graphed vs eager: max |d| of the parameters", (w_e - w_g).abs().max().item(), "total", p_e["total"].item(), p_g["total"].item())
    assert _same_bits(w_e, w_g), (w_e - w_g).abs().max().item()
    for k in ("total", "ifv_cam", "ifv_lidar"):
        assert bool(torch.isfinite(p_e[k])) and _same_bits(p_e[k], p_g[k]), k
    _, _, w_m = _kd_step5(1e-3, steps=6, beta=5.0)
    assert not _same_bits(w_e, w_m)


def _part_mismatched_label_size(monkeypatch):
    """labels at the resolution of an x4 head's logits, not of the feature maps: a KDError before any launch, in both forms"""
    from kdrt import KDError
    from kdrt.lib import lib
    from kdrt.losses import IntraClassKD, kd_objective, kd_objective_backward
    calls = []
    with monkeypatch.context() as mp:
        mp.setattr(type(lib), "call", lambda self, name, *a: calls.append(name))
        g = torch.Generator().manual_seed(3)
        zs = torch.randn(2, 3, 32, 32, generator=g).cuda().requires_grad_()
        zt = torch.randn(2, 3, 32, 32, generator=g).cuda()
        y = torch.randint(-1, 3, (2, 32, 32), generator=g).cuda()
        ms = {k: torch.randn(2, 8, 8, 8, generator=g).cuda().requires_grad_() for k in ("camera_feat", "lidar_feat")}
        mt = {k: torch.randn(2, 12, 8, 8, generator=g).cuda() for k in ("camera_feat", "lidar_feat")}
        for fn in (kd_objective, kd_objective_backward):
            with pytest.raises(KDError, match="label map"):
                fn(zs, ms, zt, mt, y, feature_loss=IntraClassKD())
            assert calls == [] and zs.grad is None and ms["camera_feat"].grad is None


def _part_default_and_pair_paths(monkeypatch):
    """feature_loss=None and PairKD leave the same parameter bytes and make the same library calls before and after an IntraClassKD
    step has run in the process; the option swaps exactly the feature-term calls"""
    from kdrt.kd import KDStep
    from kdrt.lib import lib
    from kdrt.losses import IntraClassKD, PairKD
    from kdrt.optim import FusedAdamW
    images, pts, labels = _inputs()
    calls = []
    real = type(lib).call

    def spy(self, name, *a):
        calls.append(name)
        return real(self, name, *a)
    with monkeypatch.context() as mp:
        mp.setattr(type(lib), "call", spy)

        def run(how):
            gc.collect()                                                 # the models of the run before are gone, and with them their entries in
            student, teacher = _models()                                 # the process-wide W^T cache: every run starts from the same state
            opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
            step = KDStep(student, teacher, opt, torch.tensor([0.4, 3.5]).cuda(), feature_loss=how)
            assert step.feature_loss is how
            del calls[:]
            for _ in range(2):
                parts = step(images, pts, labels)
            torch.cuda.synchronize()
            return torch.cat([p.detach().flatten() for p in student.parameters()]).clone(), parts["total"].clone(), set(parts), list(calls)

        before, ifv, after = run(None), run(IntraClassKD()), run(None)
        pair_before, ifv2, pair_after = run(PairKD()), run(IntraClassKD()), run(PairKD())
        assert before[2] == {"ce", "kl", "mse_cam", "mse_lidar", "total", "logits"} and ifv[2] == PARTS | {"logits"}
        for x, z in ((before, after), (pair_before, pair_after), (ifv, ifv2)):
            assert _same_bits(x[0], z[0]) and _same_bits(x[1], z[1]) and x[2] == z[2]
            assert x[3] == z[3], [(i, a, b) for i, (a, b) in enumerate(zip(x[3], z[3])) if a != b][:3] + [len(x[3]), len(z[3])]
        loss_calls = [c for c in before[3] if c in ("kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_kd_objective_final", "kd_kd_total", "kd_mse_fwd_bwd")]
        assert loss_calls == ["kd_seg_loss_fwd_bwd", "kd_mse_partial", "kd_mse_partial", "kd_kd_objective_final"] * 2
        assert not any("pair" in c or "cwd" in c or "ifv" in c for c in before[3])
        assert [c for c in pair_before[3] if c not in before[3]] == ["kd_feat_pair_fwd_bwd", "kd_feat_pair_fwd_bwd", "kd_kd_total"] * 2
        assert not any("ifv" in c for c in pair_before[3])
        assert [c for c in ifv[3] if c not in before[3]] == ["kd_feat_ifv_fwd_bwd", "kd_feat_ifv_fwd_bwd", "kd_kd_total"] * 2
        assert [c for c in ifv[3] if c in before[3]] == [c for c in before[3] if c not in ("kd_mse_partial", "kd_kd_objective_final")]
        assert not _same_bits(before[0], ifv[0]) and not _same_bits(pair_before[0], ifv[0])


def _part_trainer(tmp_path):
    from _fake_pandaset import write_tree
    from kdrt.losses import IntraClassKD
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import KDTrainer
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False)
    torch.manual_seed(1)
    spec = IntraClassKD()
    kd = KDTrainer(build_product("weighted", 64), build_product("concat", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"),
                   class_weights=[0.4, 3.5], num_epochs=1, feature_loss=spec)
    assert kd.kd_step.feature_loss is spec and kd.kd_step.hard_loss is None
    loss, _ = kd.train_epoch()
    assert loss == loss and abs(loss) < float("inf")
    assert kd.validate()[0] > 0                                   # validation is the hard-label loss, as before


# The parts above run as two tests: one process-wide library, one set of shared references, and the whole suite's test count stays
# nearly what it was.  Each part asserts on its own; a failure names the part in its traceback.

def test_kernel():
    """kd_feat_ifv_fwd_bwd through the C ABI and intra_class_kd: float64 bounds on every shape, exact bits, exact zeros, the same
    bytes (two calls, value-only call, graph replay), every refusal before a launch, the autograd function"""
    for part in (_part_float64, _part_exact_bits, _part_identical_zeros, _part_same_bytes, _part_refusals, _part_intra_class_kd):
        part()


def test_layers_above(monkeypatch, tmp_path):
    """the KD objective in both forms, a 5-class KDStep eager / graphed, a mismatched label size, the untouched default and PairKD
    call logs, a KDTrainer epoch"""
    _part_objective_forms()
    _part_step_graphed()
    _part_mismatched_label_size(monkeypatch)
    _part_default_and_pair_paths(monkeypatch)
    _part_trainer(tmp_path)
