"""Lightweight KD students on the GPU: TwinLiteEncoder(base_channels=b) for b in {8, 16, 24, 40} (32 is the rest of the suite)
through every layer -- the stem kernels' COUT instances, the fp32 GEMM / depthwise / weight-gradient kernels at the narrow
shapes (K, N of 8 .. 240), the masked bf16 GEMM tile -- against the CPU oracle (width-generic: every shape comes from the
weights) and float64 references.  FPN width and LiDAR feature_dim stay 128, so a b-wide student distils from the 32-wide
teacher with the unchanged objective."""
import pytest
import torch
import torch.nn.functional as F

import kd_oracle as O
from _gpu_util import ftol, grads_match, max_err

pytestmark = pytest.mark.gpu

WIDTHS = (8, 16, 24, 40)
FUSIONS = {"concat": 256, "minimal": 128, "weighted": 128}
LOGIT_TOL = 1e-4


def build(fusion, grid, b, device="cuda"):
    from src.models.camera_encoder import TwinLiteEncoder
    from src.models.fusion_module import CompleteSegmentationModel
    from src.models.lidar_encoder import LiDAREncoder
    cam = TwinLiteEncoder(base_channels=b, return_multiscale=True)
    lid = LiDAREncoder(encoder_type="spatial", grid_size=(grid, grid), use_vectorized=True)
    m = CompleteSegmentationModel(cam, lid, num_classes=2, fusion_type=fusion, fusion_out_channels=FUSIONS[fusion],
                                  camera_fpn_stages=["stage3", "stage4", "stage5"], camera_fpn_channels=128, output_mode="same")
    return m.to(device)


def load_state(model, seed):
    """kd_oracle.randomize_state over the model's own state_dict shapes (name-keyed, as tests/_gpu_util.load_random_state)."""
    sd = model.state_dict()
    st = O.randomize_state({k: v.cpu() for k, v in sd.items()}, seed)
    for k in sd:
        if k.endswith("grid_tensor"):
            st[k] = sd[k].cpu()
    model.load_state_dict(st)
    return st


# Model-level gradients at B = 2 with training-mode BatchNorm are sensitive to ReLU / ReLU6 / scatter-max kinks (see
# _gpu_util.grads_match): a pre-activation within fp32 rounding of a kink moves whole upstream tensors by ~1e-2.  The seed of each
# (b, fusion, image size) is the first one whose fp32 CPU oracle gradients agree with the float64 oracle's to 2.5e-3 relative L2
# (no kink within rounding); where none of seeds 1-11 meets that, seed 1.
SEEDS = {(8, "concat", 256): 5, (8, "minimal", 64): 2, (8, "weighted", 256): 2, (16, "concat", 256): 6, (16, "minimal", 256): 2,
         (16, "weighted", 256): 3, (24, "weighted", 256): 4, (40, "minimal", 64): 2}

_ORACLE = {}


def oracle_train(st, key, fusion, images, pts, labels, cw, G):
    """Oracle training forward + CE backward, cached across the two GEMM arithmetics (the oracle does not depend on them)."""
    if key not in _ORACLE:
        s = O.clone_state(st, requires_grad=True)
        logits, _ = O.complete_model(images, pts, s, fusion_type=fusion, grid=(G, G), training=True)
        loss = O.weighted_ce(logits, labels, cw)
        loss.backward()
        _ORACLE[key] = (logits.detach(), loss.detach(), {k: v.grad for k, v in s.items() if v.grad is not None},
                        {k: v.detach() for k, v in s.items()})
    return _ORACLE[key]


# ---------------------------------------------------------------------------------------------------------------------------
# 1. training step (forward, CE, backward, BatchNorm running statistics) against the oracle
@pytest.mark.parametrize("shape", ((2, 64, 700, 16), (2, 256, 5000, 64)))
@pytest.mark.parametrize("fusion", list(FUSIONS))
@pytest.mark.parametrize("b", WIDTHS)
def test_train_step_vs_oracle(b, fusion, shape, gemm_arith):
    from kdrt.losses import seg_loss
    B, HW, N, G = shape
    seed = SEEDS.get((b, fusion, HW), 1)
    model = build(fusion, G, b)
    st = load_state(model, seed)
    model.train()
    images, pts, labels = O.make_inputs(B, HW, N, G, seed, pad_tail=40)
    cw = torch.tensor([0.4, 3.5])
    logits = model(images.cuda(), pts.cuda())
    ce, _ = seg_loss(logits, labels.cuda(), cw.cuda())
    ce.backward()
    zr, lr, grads, state = oracle_train(st, (b, fusion, shape), fusion, images, pts, labels, cw, G)
    assert max_err(logits, zr)[0] < LOGIT_TOL
    assert abs(ce.item() - lr.item()) < LOGIT_TOL
    bad = []
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        ok, msg = grads_match(p.grad, grads[name])
        if not ok:
            bad.append((name, msg))
    assert not bad, bad
    sd = model.state_dict()
    for k, v in state.items():
        if k.endswith(("running_mean", "running_var")):
            assert max_err(sd[k], v)[0] < 1e-4 * max(1.0, v.abs().max().item()), k
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(v) == 1, k


# ---------------------------------------------------------------------------------------------------------------------------
# 2. eval forward against the oracle (the suite's eval criterion: 1e-4, scaled where random BatchNorm statistics make the
#    activations large -- tests/_gpu_util.ftol)
@pytest.mark.parametrize("fusion", list(FUSIONS))
@pytest.mark.parametrize("b", WIDTHS)
def test_eval_forward_vs_oracle(b, fusion, gemm_arith):
    B, HW, N, G = 2, 64, 700, 16
    model = build(fusion, G, b)
    st = load_state(model, 0)
    model.eval()
    images, pts, _ = O.make_inputs(B, HW, N, G, 0, pad_tail=40)
    with torch.no_grad():
        logits, mids = model(images.cuda(), pts.cuda(), return_intermediates=True)
        ms = model.camera_encoder(images.cuda())
    zr, ref = O.complete_model(images, pts, O.clone_state(st), fusion_type=fusion, grid=(G, G), training=False)
    assert max_err(logits, zr)[0] < ftol(zr)
    for k in ("camera_feat", "lidar_feat"):
        assert max_err(mids[k], ref[k])[0] < ftol(ref[k]), k
    enc = O.twinlite_encoder(images, O.clone_state(st), "camera_encoder.", False, True)
    for k, v in ms.items():
        assert v.shape[1] == {"stage2": 2, "stage3": 2, "stage4": 4, "stage5": 4}[k] * b
        assert max_err(v, enc[k])[0] < ftol(enc[k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 3. KD: a concat b = 32 teacher distils into a weighted b-wide student (fused objective, feature-gradient deposits)
def _kd_setup(b, G, storage="fp32", lr=0.0):
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    teacher = build("concat", G, 32)
    t_st = load_state(teacher, 11)
    teacher.eval()
    student = build("weighted", G, b)
    s_st = load_state(student, 12)
    student.train()
    opt = FusedAdamW(student.parameters(), lr=lr, weight_decay=0.0 if lr == 0.0 else 1e-3)
    cw = torch.tensor([0.4, 3.5])
    step = KDStep(student, teacher, opt, cw.cuda(), T=4.0, alpha=1.0, beta=1.0, teacher_storage=storage)
    return teacher, t_st, student, s_st, opt, step, cw


@pytest.mark.parametrize("b", (8, 16, 40))
def test_kd_step_small_student_vs_oracle(b):
    from kdrt import gradsink
    B, HW, N, G = 2, 64, 700, 16
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    try:
        _, t_st, student, s_st, opt, step, cw = _kd_setup(b, G)
        parts = step(images.cuda(), pts.cuda(), labels.cuda())
        torch.cuda.synchronize()
        so = O.clone_state(s_st, requires_grad=True)
        with torch.no_grad():
            zt, mt = O.complete_model(images, pts, O.clone_state(t_st), fusion_type="concat", grid=(G, G), training=False)
        zs, ms = O.complete_model(images, pts, so, fusion_type="weighted", grid=(G, G), training=True)
        assert ms["camera_feat"].shape == mt["camera_feat"].shape
        total, p_o = O.kd_loss(zs, ms, zt, mt, labels, cw, 4.0, 1.0, 1.0)
        total.backward()
        for k in ("ce", "kl", "mse_cam", "mse_lidar"):
            assert abs(parts[k].item() - p_o[k].item()) < LOGIT_TOL * max(1.0, abs(p_o[k].item())), (k, parts[k].item(), p_o[k].item())
        assert abs(parts["total"].item() - total.item()) < 2e-4 * max(1.0, abs(total.item()))
        assert max_err(parts["logits"], zs)[0] < LOGIT_TOL
        bad = []
        for name, p in student.named_parameters():
            ok, msg = grads_match(p.grad, so[name].grad)
            if not ok:
                bad.append((name, msg))
        assert not bad, bad
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()


def test_graphed_kd_step_b16_student_matches_eager():
    from kdrt import gradsink
    from kdrt.kd import GraphedKDStep
    B, HW, N, G = 2, 64, 512, 16
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    try:
        _, _, s_e, _, opt_e, step_e, _ = _kd_setup(16, G, lr=1e-3)
        for _ in range(6):                                   # 3 warm-up + 3: same count as the graphed run below
            out_e = step_e(images, pts, labels)
        _, _, s_g, _, opt_g, step_g, _ = _kd_setup(16, G, lr=1e-3)
        graphed = GraphedKDStep(step_g, images, pts, labels, warmup=3)
        for _ in range(3):
            out_g = graphed(images, pts, labels)
        torch.cuda.synchronize()
        assert opt_g._step == 6
        assert abs(out_g["total"].item() - out_e["total"].item()) < 1e-5
        for (n1, p1), (_, p2) in zip(s_e.named_parameters(), s_g.named_parameters()):
            assert torch.equal(p1, p2), n1
        for (n1, b1), (_, b2) in zip(s_e.named_buffers(), s_g.named_buffers()):
            assert torch.equal(b1, b2), n1
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. bf16 inference at width b (tolerances of tests/test_gpu_bf16.py)
LOGIT_TOL_REL, LOGIT_TOL_REL_WEIGHTED, ARGMAX_MIN = 1.5e-2, 5e-2, 0.99


@pytest.mark.parametrize("fusion", list(FUSIONS))
@pytest.mark.parametrize("b", WIDTHS)
def test_bf16_forward_small_student(b, fusion):
    from kdrt.bf16 import forward_bf16
    B, HW, N, G = 2, 64, 700, 16
    images, pts, _ = O.make_inputs(B, HW, N, G, 5, pad_tail=60)
    model = build(fusion, G, b)
    st = load_state(model, 21)
    model.eval()
    with torch.no_grad():
        z32 = model(images.cuda(), pts.cuda())
    z16 = forward_bf16(model, images.cuda(), pts.cuda())
    assert z16.shape == z32.shape
    rng = (z32.max() - z32.min()).item()
    tol = LOGIT_TOL_REL_WEIGHTED if fusion == "weighted" else LOGIT_TOL_REL
    err = (z16 - z32).abs().max().item()
    agree = (z16.argmax(1) == z32.argmax(1)).float().mean().item()
    print(f"bf16 vs fp32 HIP [b={b} {fusion}]: {err / rng:.2%} of the logit range, argmax agreement {agree:.2%}")
    assert err <= tol * rng and agree >= ARGMAX_MIN, (err, rng, agree)
    with torch.no_grad():
        zo, _ = O.complete_model(images, pts, O.clone_state(st), fusion_type=fusion, grid=(G, G), training=False)
    err_o = (z16.cpu() - zo).abs().max().item()
    agree_o = (z16.cpu().argmax(1) == zo.argmax(1)).float().mean().item()
    assert err_o <= tol * rng and agree_o >= ARGMAX_MIN, (err_o, agree_o)


def test_kd_step_bf16_teacher_b16_student():
    from kdrt import gradsink
    B, HW, N, G = 2, 64, 700, 16
    images, pts, labels = (t.cuda() for t in O.make_inputs(B, HW, N, G, 4, pad_tail=40))
    res = {}
    try:
        for storage in ("fp32", "bf16"):
            _, _, _, _, opt, step, _ = _kd_setup(16, G, storage=storage)
            parts = step(images, pts, labels)
            torch.cuda.synchronize()
            res[storage] = ({k: parts[k].item() for k in ("ce", "kl", "mse_cam", "mse_lidar", "total")}, opt.flat.grad.clone())
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()
    (p32, g32), (p16, g16) = res["fp32"], res["bf16"]
    assert p16["ce"] == p32["ce"]
    for k in ("kl", "mse_cam", "mse_lidar", "total"):
        assert abs(p16[k] - p32[k]) <= 5e-2 * max(abs(p32[k]), 1e-6), (k, p32[k], p16[k])
    cos = F.cosine_similarity(g16.double().view(1, -1), g32.double().view(1, -1)).item()
    assert cos >= 0.995, cos


# ---------------------------------------------------------------------------------------------------------------------------
# 5. kernel units
@pytest.mark.parametrize("cin", (3, 4))
@pytest.mark.parametrize("cout", (8, 16, 24, 32, 40))
def test_stem_kernels_against_float64(cout, cin):
    """kd_stem_conv_fwd (raw output + BatchNorm statistics slab) and kd_stem_conv_fwd_infer (conv + BN + ReLU6) at every stem
    width, against float64 F.conv2d on the same inputs.  Odd H / W: a ragged last 256-pixel batch."""
    from kdrt.lib import lib
    from kdrt.ops import ACT_RELU6, P, stream
    B, H, W = 3, 45, 37
    g = torch.Generator().manual_seed(cout * 10 + cin)
    x = torch.rand(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.4
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    ref = F.conv2d(x.double(), w.double(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    rows = lib.kd_stem_stat_rows(B * Ho * Wo)
    y = torch.full((B * Ho * Wo + 64, cout), 3.0, device="cuda")            # rows past the output stay untouched
    part = torch.empty(rows * 2 * cout, device="cuda")
    xc, wc = x.cuda(), w.cuda()
    lib.call("kd_stem_conv_fwd", P(xc), P(wc), P(y), P(part), B, cin, H, W, cout, stream())
    torch.cuda.synchronize()
    assert bool((y[B * Ho * Wo:] == 3.0).all())
    assert (y[: B * Ho * Wo].double().cpu() - ref).abs().max().item() < 1e-5
    s = part.view(rows, 2, cout).double().sum(0).cpu()
    assert (s[0] - ref.sum(0)).abs().max().item() < 1e-5 * ref.abs().sum(0).max().item()
    assert (s[1] - (ref * ref).sum(0)).abs().max().item() < 1e-5 * (ref * ref).sum(0).max().item()
    if cin == 3:
        yi = torch.full((B * Ho * Wo + 64, cout), 3.0, device="cuda")
        scc, shc = sc.cuda(), sh.cuda()                                       # (kept alive until the launch has run)
        lib.call("kd_stem_conv_fwd_infer", P(xc), P(wc), P(scc), P(shc), ACT_RELU6, P(yi), B, cin, H, W, cout, stream())
        torch.cuda.synchronize()
        want = torch.clamp(ref * sc.double() + sh.double(), 0.0, 6.0)
        assert bool((yi[B * Ho * Wo:] == 3.0).all())
        assert (yi[: B * Ho * Wo].double().cpu() - want).abs().max().item() < 1e-5


@pytest.mark.parametrize("cout", (8, 16, 24, 40))
def test_bf16_stem_against_float64(cout):
    from kdrt.lib import lib
    from kdrt.ops import ACT_RELU6, P, stream
    B, H, W = 2, 45, 37
    g = torch.Generator().manual_seed(cout)
    x = torch.rand(B, 3, H, W, generator=g)
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.4
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.2
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.full((B * Ho * Wo + 64, cout), 3.0, device="cuda", dtype=torch.bfloat16)
    xc, wc, scc, shc = x.cuda(), w.cuda(), sc.cuda(), sh.cuda()
    lib.call("kd_bf16_stem", P(xc), P(wc), P(scc), P(shc), ACT_RELU6, P(y), B, 3, H, W, cout, stream())
    torch.cuda.synchronize()
    ref = F.conv2d(x.double(), w.double(), stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, cout)
    want = torch.clamp(ref * sc.double() + sh.double(), 0.0, 6.0)
    assert bool((y[B * Ho * Wo:].float() == 3.0).all())
    err = (y[: B * Ho * Wo].double().cpu() - want).abs()
    assert bool((err <= 2.0 ** -8 * want.abs() + 1e-5).all()), err.max().item()


KN = (8, 16, 24, 40, 48, 144)


@pytest.mark.parametrize("N", KN)
@pytest.mark.parametrize("K", KN)
def test_bf16_pwconv_narrow_shapes_against_float64(K, N):
    """kd_bf16_pwconv at K, N multiples of 8 (the masked, zero-padded tile): bf16 output with and without a residual, as a column
    slice of a wider buffer (the columns past N are not written), and the epi 4 scatter-max into an fp32 grid."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    M, pad = 777, 8
    g = torch.Generator().manual_seed(K * 1000 + N)
    A = torch.randn(M, K, generator=g).bfloat16()
    W, bias = torch.randn(N, K, generator=g) * 0.3, torch.randn(N, generator=g) * 0.2
    sc, sh = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.3
    R = torch.randn(M, N, generator=g).bfloat16()
    z = (A.double() @ W.bfloat16().double().t() + bias.double()) * sc.double() + sh.double()
    Ac, Wc, bc, scc, shc = A.cuda(), W.cuda(), bias.cuda(), sc.cuda(), sh.cuda()
    for act, res in ((2, None), (0, R)):
        want = (torch.clamp(z, 0.0, 6.0) if act == 2 else z) + (res.double() if res is not None else 0.0)
        wide = torch.full((M, N + pad), 7.0, dtype=torch.bfloat16).cuda()
        Rc = res.cuda() if res is not None else None
        lib.call("kd_bf16_pwconv", P(Ac), K, 0, P(Wc), P(bc), P(scc), P(shc), act, P(wide), N + pad,
                 P(Rc), N if res is not None else 0, 0, M, K, N, None, None, None, None, None, 0, None, None, 0, stream())
        torch.cuda.synchronize()
        out = wide.cpu()
        assert bool((out[:, N:] == 7.0).all())
        err = (out[:, :N].double() - want).abs()
        assert bool((err <= 2.0 ** -8 * want.abs() + 1e-4 * max(1.0, want.abs().max().item())).all()), err.max().item()
    # epi 4: rows sorted by cell, grid rows padded past N (must stay 0), a few rows skipped (cell -1)
    ncell = 97
    cell = torch.sort(torch.randint(0, ncell, (M,), generator=g)).values.to(torch.int32)
    cell[:5] = -1
    grid = torch.zeros(ncell, N + pad, device="cuda")
    cc = cell.cuda()
    lib.call("kd_bf16_pwconv", P(Ac), K, 0, P(Wc), P(bc), P(scc), P(shc), 1, None, 0, None, 0, 4, M, K, N,
             None, None, None, None, None, 0, P(cc), P(grid), N + pad, stream())
    torch.cuda.synchronize()
    v = torch.clamp(z, min=0.0)
    ref = torch.zeros(ncell, N, dtype=torch.float64)
    ok = cell >= 0
    ref.index_reduce_(0, cell[ok].long(), v[ok], "amax", include_self=True)
    got = grid.cpu().double()
    assert bool((got[:, N:] == 0).all())
    assert (got[:, :N] - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("C", (8, 24, 40, 48, 144))
@pytest.mark.parametrize("stride", (1, 2))
def test_bf16_depthwise_at_student_widths(C, stride):
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    B, H, W = 2, 32, 19
    g = torch.Generator().manual_seed(C * 10 + stride)
    x = torch.randn(B, H, W, C, generator=g).bfloat16()
    w, sc, sh = torch.randn(C, 1, 3, 3, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, C), 9.0, device="cuda", dtype=torch.bfloat16)
    xc, wc, scc, shc = x.cuda(), w.cuda(), sc.cuda(), sh.cuda()
    lib.call("kd_bf16_dwconv3x3", P(xc), P(wc), P(scc), P(shc), 2, P(y), B, H, W, C, stride, stream())
    torch.cuda.synchronize()
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride, padding=1, groups=C)
    ref = torch.clamp(ref * sc.double().view(1, C, 1, 1) + sh.double().view(1, C, 1, 1), 0.0, 6.0).permute(0, 2, 3, 1)
    err = (y.cpu().double() - ref).abs()
    assert bool((err <= 2.0 ** -7 * ref.abs() + 1e-5).all()), err.max().item()


@pytest.mark.parametrize("b", (12, 48))
def test_unsupported_width_raises(b):
    from kdrt import KDError
    from kdrt.bf16 import forward_bf16
    images, pts, _ = O.make_inputs(2, 64, 256, 16, 3)
    model = build("weighted", 16, b)
    load_state(model, 1)
    for training in (True, False):
        model.train(training)
        with pytest.raises(KDError, match="8, 16, 24, 32, 40"):
            model(images.cuda(), pts.cuda())
    with pytest.raises(KDError, match="8, 16, 24, 32, 40"):
        forward_bf16(model.eval(), images.cuda(), pts.cuda())
