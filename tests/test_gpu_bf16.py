"""bf16-storage inference mode (BASELINE.json configs[1]: camera + LiDAR concat-fusion forward in bf16) -- a second mode with
its OWN stated tolerance, never a substitute for the fp32 parity contract.  Checked against the fp32 HIP path and the CPU
oracle on the same weights / inputs: max-abs logit error relative to the logit range, and the argmax agreement rate."""
import pytest
import torch

import _bf16_ref as BR
import kd_oracle as O
from _gpu_util import build_product, load_random_state

pytestmark = pytest.mark.gpu

# measured on an MI355X (seeded random weights with non-trivial BatchNorm statistics): max |logit error| 0.55-0.98 % of the
# logit range, argmax agreement 99.41-99.88 %; bf16 keeps 8 mantissa bits per stored activation through ~25 layers
LOGIT_TOL_REL = 1.5e-2
ARGMAX_MIN = 0.99
# Weighted fusion has its own logit bound.  Its two attention logits go through a softmax, and with the seeded random weights
# the logit DIFFERENCE has a standard deviation of ~30 (a trained block is far milder), so wherever the two are close the
# weights w = softmax(a) move by up to |da| / 4 per unit of logit error: the bf16 rounding of the projected maps alone
# (|da| <= 0.35; fp32 `h` and fp32 attention weights do not lower it -- emulated on the CPU oracle) moves single pixels by
# 2-4 % of the logit range.  Measured: 1.32 / 3.50 / 1.34 % at the three shapes, argmax agreement 99.41-100 % (same bound).
LOGIT_TOL_REL_WEIGHTED = 5e-2


# the third shape has an 8 x 8 BEV grid under a 16 x 16 camera map: the bilinear LiDAR resize of fusion_module.py:239-240
@pytest.mark.parametrize("fusion", ("concat", "minimal", "weighted"))
@pytest.mark.parametrize("shape", ((2, 64, 700, 16), (2, 256, 5000, 64), (2, 64, 700, 8)))
def test_bf16_forward_against_fp32_and_oracle(fusion, shape):
    from kdrt.bf16 import forward_bf16
    B, HW, N, G = shape
    images, pts, _ = O.make_inputs(B, HW, N, G, 5, pad_tail=60)
    model = build_product(fusion, G)
    st = load_random_state(model, fusion, 21)
    model.eval()
    with torch.no_grad():
        z32 = model(images.cuda(), pts.cuda())
    z16 = forward_bf16(model, images.cuda(), pts.cuda())
    assert z16.dtype == torch.float32 and z16.shape == z32.shape
    rng = (z32.max() - z32.min()).item()
    err = (z16 - z32).abs().max().item()
    agree = (z16.argmax(1) == z32.argmax(1)).float().mean().item()
    print(f"bf16 vs fp32 HIP [{fusion} {shape}]: max|dlogit| {err:.4f} = {err / rng:.2%} of range {rng:.2f}, argmax agreement {agree:.4%}")
    tol = LOGIT_TOL_REL_WEIGHTED if fusion == "weighted" else LOGIT_TOL_REL
    assert err <= tol * rng, (err, rng)
    assert agree >= ARGMAX_MIN, agree
    if True:                                         # the CPU oracle too, at both shapes (eval forward of 2 frames: < 1 s)
        with torch.no_grad():
            zo, _ = O.complete_model(images, pts, O.clone_state(st), fusion_type=fusion, grid=(G, G), training=False)
        err_o = (z16.cpu() - zo).abs().max().item()
        agree_o = (z16.cpu().argmax(1) == zo.argmax(1)).float().mean().item()
        assert err_o <= tol * rng and agree_o >= ARGMAX_MIN, (err_o, agree_o)


def test_bf16_mode_is_gated():
    from kdrt import KDError
    from kdrt.bf16 import forward_bf16
    images, pts, _ = O.make_inputs(2, 64, 256, 16, 3)
    m = build_product("concat", 16, output_mode="x4")
    m.eval()
    with pytest.raises(KDError):                     # no bf16 kernels for the transposed-convolution head: loud, no fallback
        forward_bf16(m, images.cuda(), pts.cuda())
    m2 = build_product("concat", 16)
    m2.train()
    with pytest.raises(KDError):                     # inference only
        forward_bf16(m2, images.cuda(), pts.cuda())
    with pytest.raises(KDError):                     # MI355X only
        forward_bf16(m2.eval(), images, pts)


# KD step with the frozen teacher on the bf16 path.  Measured on an MI355X (below): the teacher's targets move by
# the bf16 forward error above, so KL and the two feature MSEs move by at most a few per cent and the student's
# gradient keeps its direction (cosine > 0.999); CE does not involve the teacher and stays bit-identical.
KD_LOSS_TOL_REL = 5e-2
KD_GRAD_COS_MIN = 0.995


@pytest.mark.parametrize("teacher_fusion", ("concat", "weighted"))
def test_kd_step_with_bf16_teacher(teacher_fusion):
    from kdrt.kd import KDStep
    from kdrt.optim import FusedAdamW
    B, HW, N, G = 2, 256, 5000, 64
    images, pts, labels = O.make_inputs(B, HW, N, G, 4, pad_tail=40)
    images, pts, labels = images.cuda(), pts.cuda(), labels.cuda()
    cw = torch.tensor([0.4, 3.5]).cuda()
    res = {}
    for storage in ("fp32", "bf16"):
        teacher = build_product(teacher_fusion, G)
        load_random_state(teacher, teacher_fusion, 11)
        student = build_product("weighted", G)
        load_random_state(student, "weighted", 12)
        student.train()
        opt = FusedAdamW(student.parameters(), lr=0.0, weight_decay=0.0)     # lr 0: the flat gradient survives the step
        step = KDStep(student, teacher, opt, cw, T=4.0, alpha=1.0, beta=1.0, teacher_storage=storage)
        parts = step(images, pts, labels)
        torch.cuda.synchronize()
        res[storage] = ({k: parts[k].item() for k in ("ce", "kl", "mse_cam", "mse_lidar", "total")}, opt.flat.grad.clone())
    (p32, g32), (p16, g16) = res["fp32"], res["bf16"]
    assert p16["ce"] == p32["ce"]                                            # no teacher in CE
    for k in ("kl", "mse_cam", "mse_lidar", "total"):
        rel = abs(p16[k] - p32[k]) / max(abs(p32[k]), 1e-6)
        print(f"bf16 teacher: {k} {p32[k]:.6f} -> {p16[k]:.6f} ({rel:.2%})")
        assert rel <= KD_LOSS_TOL_REL, (k, p32[k], p16[k])
    cos = torch.nn.functional.cosine_similarity(g16.double().view(1, -1), g32.double().view(1, -1)).item()
    nrm = (g16.double().norm() / g32.double().norm()).item()
    print(f"bf16 teacher: student gradient cosine {cos:.6f}, norm ratio {nrm:.4f}")
    assert cos >= KD_GRAD_COS_MIN and abs(nrm - 1) < 5e-2
    with pytest.raises(ValueError):
        KDStep(student, teacher, opt, cw, teacher_storage="fp16")


def test_bf16_one_kernel_lidar_encoder_against_the_two_launches(monkeypatch):
    """kd_bf16_lidar_mlp_scatter (point MLP + scatter-max in one kernel, nothing between the layers in HBM) against the two
    kd_bf16_pwconv launches it replaces: the same roundings (operands to bf16 once, fp32 accumulation); only the order of the
    sums inside a dot product differs, which can move a layer-1 activation by one bf16 step (2^-8 relative) before layer 2."""
    from kdrt import bf16
    B, HW, N, G = 2, 256, 5000, 64
    images, pts, _ = O.make_inputs(B, HW, N, G, 5, pad_tail=60)
    model = build_product("concat", G)
    load_random_state(model, "concat", 21)
    model.eval()
    _, one = bf16.forward_bf16(model, images.cuda(), pts.cuda(), return_intermediates=True)
    monkeypatch.setattr(bf16, "_LIDAR_ONE_KERNEL", False)
    _, two = bf16.forward_bf16(model, images.cuda(), pts.cuda(), return_intermediates=True)
    a, b = one["lidar_feat"], two["lidar_feat"]
    assert a.shape == b.shape and (a > 0).any()
    assert torch.equal(a == 0, b == 0)                                   # the same cells / channels are occupied
    err = (a - b).abs().max().item() / b.abs().max().item()
    print(f"one-kernel bf16 LiDAR encoder vs two launches: max |diff| = {err:.2e} of the map's maximum")
    assert err <= 4e-3
    assert (one["logits"] - two["logits"]).abs().max().item() <= 1e-2 * (two["logits"].max() - two["logits"].min()).item()


@pytest.mark.parametrize("M,K,N,res,sliced", [(4096, 32, 32, True, False), (4100, 32, 192, False, False), (1000, 64, 384, False, False),
                                              (777, 64, 64, True, False), (5000, 128, 128, True, True), (3001, 192, 64, False, False),
                                              (2049, 256, 128, False, True), (1111, 384, 64, True, False), (2500, 384, 128, False, False),
                                              (900, 512, 128, False, False), (1300, 768, 128, True, False), (31, 128, 768, False, False),
                                              (130, 32, 32, True, False), (64, 64, 96, False, False)])
def test_bf16_gemm_second_form_same_bits_as_the_first(M, K, N, res, sliced):
    """kd_bf16_pwconv has two kernels for bf16 in / bf16 out: the round-4 form (K static, prefetch across slabs, residual tile requested
    first, 16-byte stores through an LDS tile) and the first form, which still serves fp32 inputs, the LiDAR layers and any launch given a
    device-side row count.  Same products, same accumulation order, one rounding: the outputs must be bit-identical -- on every K the
    second form has an instance for, ragged M (partial units), residuals, and C as a column slice of a wider buffer."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    A = rnd(M, K).bfloat16()
    W, b, sc, sh = rnd(N, K) * 0.2, rnd(N), rnd(N).abs() + 0.5, rnd(N) * 0.3
    R = rnd(M, N).bfloat16() if res else None
    outs = []
    for first_form in (False, True):
        wide = torch.full((M, 2 * N if sliced else N), 7.0, device="cuda", dtype=torch.bfloat16)
        out = wide[:, N:] if sliced else wide
        mdev = torch.tensor([M], device="cuda", dtype=torch.int32) if first_form else None     # a device-side M selects the first form
        lib.call("kd_bf16_pwconv", P(A), K, 0, P(W), P(b), P(sc), P(sh), 2, P(out), out.stride(0), P(R), N if res else 0, 0, M, K, N,
                 P(mdev), None, None, None, None, 0, None, None, 0, stream())
        torch.cuda.synchronize()
        if sliced:
            assert bool((wide[:, :N] == 7.0).all())                    # the neighbouring columns are untouched
        outs.append(out.float().clone())
    assert torch.equal(outs[0], outs[1])
    # the float64 value of the same bf16 operands within the fp32 accumulation bound, rounded to bf16 once (tests/_bf16_ref.py)
    ok, lo, hi = BR.accept(outs[0], *BR.pwconv(A, W, b, sc, sh, R), 2, R)
    assert bool(ok.all()), int((~ok).sum())


@pytest.mark.parametrize("B,H,W,C,stride", [(2, 16, 9, 32, 1), (3, 48, 20, 8, 1), (1, 24, 7, 384, 1), (2, 20, 11, 64, 1), (1, 64, 64, 192, 1),
                                            (2, 8, 5, 768, 1), (2, 32, 18, 32, 2), (1, 17, 9, 64, 2)])
def test_bf16_depthwise_forms_against_torch(B, H, W, C, stride):
    """kd_bf16_dwconv3x3: stride 1 runs as one software pipeline over a thread's column segments where Ho is a multiple of 16 or 8 (one,
    several and many segments per column here), otherwise -- and for stride 2 -- segment by segment.  Against F.conv2d on the same bf16
    input in fp32: the result is rounded to bf16 once, so the two may differ by one bf16 ulp where the fp32 sums differ in the last bits."""
    import torch.nn.functional as F
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H * 10 + C)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    x = rnd(B, H, W, C).bfloat16()
    w, sc, sh = rnd(C, 1, 3, 3) * 0.3, rnd(C).abs() + 0.5, rnd(C) * 0.2
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.full((B, Ho, Wo, C), 9.0, device="cuda", dtype=torch.bfloat16)
    lib.call("kd_bf16_dwconv3x3", P(x), P(w), P(sc), P(sh), 2, P(y), B, H, W, C, stride, stream())
    torch.cuda.synchronize()
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w, stride=stride, padding=1, groups=C)
    ref = torch.clamp(ref * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1), 0.0, 6.0).permute(0, 2, 3, 1)
    z, e = BR.dwconv(x, w, sc, sh, stride)
    assert bool(((ref.double() - BR.act(z, 2)).abs() <= e).all())            # F.conv2d in fp32 meets the same bound
    ok, lo, hi = BR.accept(y, z, e, 2)
    assert bool(ok.all()), int((~ok).sum())
