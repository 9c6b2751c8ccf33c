"""Unit-level GPU parity: each reference module on its own, forward AND every gradient, against the
CPU oracle at rounding-level tolerance (these problems are too small to land on a ReLU kink).
Shapes include the awkward ones: M not a multiple of the 128-row GEMM tile, N=192 / K=32 tiles,
odd spatial sizes under stride 2, 28x28 maps (config-1's 224^2 input)."""
import numpy as np
import pytest
import torch

import kd_oracle as O
from _gpu_util import max_err

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_arith")]
TOL = 2e-5          # relative to each tensor's max magnitude


def _rand_state(module, seed):
    st = O.randomize_state({k: v.detach().clone() for k, v in module.state_dict().items()}, seed)
    for k, v in module.state_dict().items():
        if k.endswith("grid_tensor"):
            st[k] = v.clone()
    module.load_state_dict(st)
    return st


def _compare(module, oracle_fn, x, seed, training=True, x_grad=True):
    st = _rand_state(module, seed)
    module = module.cuda().train(training)
    g = torch.Generator().manual_seed(100 + seed)
    xg = x.clone().cuda().requires_grad_(x_grad)
    y = module(xg)
    so = O.clone_state(st, requires_grad=True)
    xc = x.clone().requires_grad_(x_grad)
    yo = oracle_fn(xc, so)
    ys = y if isinstance(y, dict) else {"out": y}
    yos = yo if isinstance(yo, dict) else {"out": yo}
    loss = loss_o = 0.0
    for k in yos:
        assert ys[k].shape == yos[k].shape, k
        d, r = max_err(ys[k], yos[k])
        assert r < TOL, (k, d, r)
        up = torch.randn(yos[k].shape, generator=g)
        loss = loss + (ys[k] * up.cuda()).sum()
        loss_o = loss_o + (yos[k] * up).sum()
    loss.backward()
    loss_o.backward()
    if x_grad:
        assert max_err(xg.grad, xc.grad)[1] < TOL, "input grad"
    for name, p in module.named_parameters():
        want = so[name].grad
        assert p.grad is not None, name
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "bias" and want.abs().max() < 1e-4 * max(1.0, float(loss_o.detach().abs()) ** 0.5):
            assert p.grad.abs().max().item() < 1e-3, name     # zero-gradient conv bias in front of a BN: noise
            continue
        d, r = max_err(p.grad, want)
        assert r < 5 * TOL, (name, d, r)
    for k, v in so.items():
        if k.endswith(("running_mean", "running_var")):
            assert max_err(module.state_dict()[k], v)[1] < 1e-5, k


@pytest.mark.parametrize("cin,cout,stride,exp,hw", [(32, 32, 1, 1, 16), (32, 64, 2, 6, 14), (64, 64, 1, 6, 7),
                                                     (64, 128, 2, 6, 7), (128, 128, 1, 6, 4)])
@pytest.mark.parametrize("training", (True, False))
def test_inverted_residual(cin, cout, stride, exp, hw, training):
    from src.models.camera_encoder import InvertedResidual
    torch.manual_seed(0)
    m = InvertedResidual(cin, cout, stride=stride, expansion_ratio=exp)
    x = torch.randn(3, cin, hw, hw, generator=torch.Generator().manual_seed(1))
    _compare(m, lambda xx, st: O.inverted_residual(xx, st, "", cin, cout, stride, exp, training)
             if False else O.inverted_residual(xx, {("." + k): v for k, v in st.items()}, "", cin, cout, stride, exp, training),
             x, seed=cin + stride, training=training)


@pytest.mark.parametrize("hw", (32, 28))
def test_twinlite_encoder_multiscale(hw):
    from src.models.camera_encoder import TwinLiteEncoder
    m = TwinLiteEncoder(return_multiscale=True)
    x = torch.rand(2, 3, hw, hw, generator=torch.Generator().manual_seed(2))
    _compare(m, lambda xx, st: O.twinlite_encoder(xx, st, "", True, True), x, seed=5, x_grad=False)


def test_twinlite_config1_shape_and_eval():
    """BASELINE configs[0]: TwinLiteEncoder() on a 4x3x224x224 batch (shape pin test_camera_encoder.py:24-40)."""
    from src.models.camera_encoder import TwinLiteEncoder
    m = TwinLiteEncoder()
    st = _rand_state(m, 9)
    m = m.cuda().eval()
    x = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        y = m(x.cuda())
        yo = O.twinlite_encoder(x, O.clone_state(st), "", False, False)
    assert y.shape == (4, 128, 28, 28)
    assert max_err(y, yo)[1] < TOL


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 128), (256, 64)])
def test_conv1x1_and_dwsep(cin, cout):
    from src.models.fusion_module import Conv1x1, DWSeparableConv
    x = torch.randn(2, cin, 12, 12, generator=torch.Generator().manual_seed(3))
    _compare(Conv1x1(cin, cout), lambda xx, st: O.conv1x1_block(xx, {("m." + k): v for k, v in st.items()}, "m", True), x, 11)
    _compare(DWSeparableConv(cin, cout), lambda xx, st: O.dwsep_block(xx, {("m." + k): v for k, v in st.items()}, "m", True), x, 12)


def test_camera_fpn():
    from src.models.fusion_module import CameraFPNLite
    stages = ["stage3", "stage4", "stage5"]
    fpn = CameraFPNLite({"stage2": 64, "stage3": 64, "stage4": 128, "stage5": 128}, 128, stages)
    st = _rand_state(fpn, 21)
    fpn = fpn.cuda().train()
    g = torch.Generator().manual_seed(4)
    feats = {"stage3": torch.randn(2, 64, 12, 12, generator=g), "stage4": torch.randn(2, 128, 6, 6, generator=g),
             "stage5": torch.randn(2, 128, 6, 6, generator=g)}
    fg = {k: v.clone().cuda().requires_grad_(True) for k, v in feats.items()}
    fc = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
    y = fpn(fg)
    so = O.clone_state(st, requires_grad=True)
    yo = O.camera_fpn(fc, {("f." + k): v for k, v in so.items()}, "f", stages, True)
    assert max_err(y, yo)[1] < TOL
    up = torch.randn(yo.shape, generator=g)
    (y * up.cuda()).sum().backward()
    (yo * up).sum().backward()
    for k in feats:
        assert max_err(fg[k].grad, fc[k].grad)[1] < 5 * TOL, k
    for name, p in fpn.named_parameters():
        assert max_err(p.grad, so[name].grad)[1] < 5 * TOL, name


@pytest.mark.parametrize("n,grid,pad", [(300, 8, 0), (1000, 16, 200)])
def test_lidar_encoder(n, grid, pad):
    from src.models.lidar_encoder import LiDAREncoder
    enc = LiDAREncoder(encoder_type="spatial", grid_size=(grid, grid))
    st = _rand_state(enc, 31)
    enc = enc.cuda().train()
    _, pts, _ = O.make_inputs(2, 8, n, grid, 7, pad_tail=pad)
    y = enc(pts.cuda())
    so = O.clone_state(st, requires_grad=True)
    yo = O.spatial_lidar_encoder(pts, so, "encoder.", (grid, grid), True)
    assert max_err(y, yo)[1] < TOL
    up = torch.randn(yo.shape, generator=torch.Generator().manual_seed(8))
    (y * up.cuda()).sum().backward()
    (yo * up).sum().backward()
    for name, p in enc.named_parameters():
        want = so[name].grad
        if name.endswith(("point_mlp.0.bias", "point_mlp.3.bias", "point_mlp.6.bias")):
            assert p.grad.abs().max().item() < 1e-3, name
            continue
        assert max_err(p.grad, want)[1] < 5 * TOL, name


def test_lidar_encoder_eval_mode_backward(monkeypatch):
    """eval() with autograd on (frozen-BatchNorm fine-tuning): running statistics in the forward, real gradients back."""
    from src.models.lidar_encoder import LiDAREncoder
    from kdrt import units
    enc = LiDAREncoder(encoder_type="spatial", grid_size=(16, 16))
    st = _rand_state(enc, 33)
    enc = enc.cuda().eval()
    _, pts, _ = O.make_inputs(2, 8, 900, 16, 9, pad_tail=100)
    y = enc(pts.cuda())
    so = O.clone_state(st, requires_grad=True)
    yo = O.spatial_lidar_encoder(pts, so, "encoder.", (16, 16), False)
    assert max_err(y, yo)[1] < TOL
    with torch.no_grad():
        # the one-kernel inference encoder sums each dot product in its own order: oracle tolerance, not bits
        assert max_err(enc(pts.cuda()), yo)[1] < TOL
        monkeypatch.setattr(units, "_LIDAR_FUSED_INFER", False)
        assert torch.equal(enc(pts.cuda()).view(torch.int32), y.detach().view(torch.int32))    # layer-by-layer: same bits
    up = torch.randn(yo.shape, generator=torch.Generator().manual_seed(8))
    (y * up.cuda()).sum().backward()
    (yo * up).sum().backward()
    for name, p in enc.named_parameters():
        assert max_err(p.grad, so[name].grad)[1] < 5 * TOL, name


@pytest.mark.parametrize("fusion", ("concat", "minimal", "weighted"))
def test_fusion_and_head_small(fusion):
    """Fusion block + head driven through the full-model oracle with tiny encoders' outputs replaced
    by random feature maps: isolates fusion_module.py:242-258."""
    from src.models.fusion_module import (ConcatenationFusion, MinimalFusion, SameResolutionSegmentationHead,
                                          WeightedFusion)
    torch.manual_seed(0)
    fus = {"concat": lambda: ConcatenationFusion(128, 128, 256), "minimal": lambda: MinimalFusion(128, 128, 128),
           "weighted": lambda: WeightedFusion(128, 128, 128)}[fusion]()
    head = SameResolutionSegmentationHead(256 if fusion == "concat" else 128, 2)
    stf, sth = _rand_state(fus, 41), _rand_state(head, 42)
    fus, head = fus.cuda().train(), head.cuda().train()
    # data seed 7: with seed 6 the split arithmetic lands one pre-activation on the other side of a ReLU kink
    # (tools/gpu_diag_flip.py: seeds 7..13 agree to <= 1.6e-6 in both arithmetics, seed 6 flips under "split" only)
    g = torch.Generator().manual_seed(7)
    cam, lid = torch.randn(2, 128, 10, 10, generator=g), torch.randn(2, 128, 10, 10, generator=g).clamp_min(0)
    cg, lg = cam.clone().cuda().requires_grad_(True), lid.clone().cuda().requires_grad_(True)
    cc, lc = cam.clone().requires_grad_(True), lid.clone().requires_grad_(True)
    z = head(fus(cg, lg))
    so = O.clone_state({**{"fusion." + k: v for k, v in stf.items()}, **{"head." + k: v for k, v in sth.items()}}, True)
    # oracle: reuse complete_model's fusion/head section by calling the pieces directly
    if fusion == "concat":
        cp = O.conv1x1_block(cc, so, "fusion.camera_proj", True); lp = O.conv1x1_block(lc, so, "fusion.lidar_proj", True)
        h = O._dw_bn_act(torch.cat([cp, lp], 1), so, "fusion.fuse.0", "fusion.fuse.1", "relu", 1, True)
        fused = O._pw_bn_act(h, so, "fusion.fuse.3", "fusion.fuse.4", "relu", True)
    else:
        cp = O.conv1x1_block(cc, so, "fusion.cam_proj", True); lp = O.conv1x1_block(lc, so, "fusion.lidar_proj", True)
        if fusion == "weighted":
            import torch.nn.functional as F
            a = F.conv2d(torch.cat([cp, lp], 1), so["fusion.attention.0.weight"], so["fusion.attention.0.bias"])
            a = F.conv2d(a.clamp_min(0), so["fusion.attention.2.weight"], so["fusion.attention.2.bias"])
            w = torch.softmax(a, 1)
            fused = cp * w[:, 0:1] + lp * w[:, 1:2]
        else:
            fused = cp + lp
    zo = O.seg_head_same(fused, so, "head", True)
    assert max_err(z, zo)[1] < TOL
    up = torch.randn(zo.shape, generator=g)
    (z * up.cuda()).sum().backward()
    (zo * up).sum().backward()
    assert max_err(cg.grad, cc.grad)[1] < 5 * TOL and max_err(lg.grad, lc.grad)[1] < 5 * TOL
    for pre, mod in (("fusion.", fus), ("head.", head)):
        for name, p in mod.named_parameters():
            assert max_err(p.grad, so[pre + name].grad)[1] < 5 * TOL, pre + name


def test_losses_and_confusion():
    from kdrt.losses import confusion, feature_mse, seg_loss
    g = torch.Generator().manual_seed(9)
    for nc in (2, 3):
        zs, zt = torch.randn(3, nc, 9, 7, generator=g) * 3, torch.randn(3, nc, 9, 7, generator=g) * 3
        y = torch.randint(0, nc, (3, 9, 7), generator=g); y[0, 0, :4] = -1
        cw = torch.rand(nc, generator=g) + 0.2
        zg, zc = zs.clone().cuda().requires_grad_(True), zs.clone().requires_grad_(True)
        ce, kl = seg_loss(zg, y.cuda(), cw.cuda(), -1, zt.cuda(), T=4.0, alpha=0.7)
        ce_o = O.weighted_ce(zc, y, cw)
        ps_log, pt = torch.log_softmax(zc / 4, 1), torch.softmax(zt / 4, 1)
        kl_o = (pt * (torch.log_softmax(zt / 4, 1) - ps_log)).sum() / (3 * 9 * 7)
        assert abs(ce.item() - ce_o.item()) < 1e-5 and abs(kl.item() - kl_o.item()) < 1e-6
        (2.5 * ce).backward()
        (2.5 * (ce_o + 0.7 * 16 * kl_o)).backward()
        assert max_err(zg.grad, zc.grad)[1] < TOL
        conf, pred = confusion(zs.cuda(), y.cuda(), num_classes=nc)
        assert torch.equal(pred.cpu(), zs.argmax(1))
        assert np.array_equal(conf.cpu().numpy(), O.confusion_matrix(zs, y, nc).numpy())
    a, b = torch.randn(2, 16, 5, 6, generator=g), torch.randn(2, 16, 5, 6, generator=g)
    ag, ac = a.clone().cuda().requires_grad_(True), a.clone().requires_grad_(True)
    (3.0 * feature_mse(ag, b.cuda())).backward()
    (3.0 * torch.nn.functional.mse_loss(ac, b)).backward()
    assert max_err(ag.grad, ac.grad)[1] < TOL


def test_lidar_resize_and_fpn_target_size():
    """fusion_module.py:239-240 (LiDAR grid != camera grid) and CameraFPNLite(target_size=...)."""
    import torch.nn.functional as F
    from kdrt import units as U
    from src.models.fusion_module import CameraFPNLite
    g = torch.Generator().manual_seed(12)
    for (hi, wi, ho, wo) in ((8, 8, 16, 16), (12, 10, 7, 9), (16, 16, 16, 16)):
        x = torch.randn(2, 8, hi, wi, generator=g)
        xg, xc = x.clone().cuda().requires_grad_(True), x.clone().requires_grad_(True)
        y, yo = U.run_resize(xg, (ho, wo)), F.interpolate(xc, size=(ho, wo), mode="bilinear", align_corners=False)
        assert max_err(y, yo)[1] < TOL
        up = torch.randn(yo.shape, generator=g)
        (y * up.cuda()).sum().backward(); (yo * up).sum().backward()
        assert max_err(xg.grad, xc.grad)[1] < 5 * TOL
    stages = ["stage3", "stage4"]
    fpn = CameraFPNLite({"stage3": 64, "stage4": 128}, 128, stages, target_size=(10, 10))
    st = _rand_state(fpn, 23)
    fpn = fpn.cuda().train()
    feats = {"stage3": torch.randn(2, 64, 12, 12, generator=g), "stage4": torch.randn(2, 128, 6, 6, generator=g)}
    y = fpn({k: v.cuda() for k, v in feats.items()})
    so = O.clone_state(st)
    acc = None
    for s_ in stages:
        t = O.conv1x1_block(feats[s_], {("f." + k): v for k, v in so.items()}, f"f.laterals.{s_}", True)
        t = F.interpolate(t, size=(10, 10), mode="bilinear", align_corners=False)
        acc = t if acc is None else acc + t
    yo = O.dwsep_block(acc, {("f." + k): v for k, v in so.items()}, "f.post", True)
    assert y.shape == (2, 128, 10, 10) and max_err(y, yo)[1] < TOL


@pytest.mark.parametrize("cin,nc,hw,training", [(256, 3, (16, 16), True), (128, 2, (8, 12), True), (128, 2, (7, 5), False)])
def test_x4_head(cin, nc, hw, training):
    """LightweightSegmentationHead (output_mode="x4", fusion_module.py:142-159): ConvTranspose2d as MFMA GEMM +
    col2im, 3x3 classifier; forward, input gradient, every parameter gradient, BN running statistics."""
    from src.models.fusion_module import LightweightSegmentationHead
    torch.manual_seed(0)
    m = LightweightSegmentationHead(cin, nc)
    x = torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(5))
    _compare(m, lambda xc, so: O.seg_head_x4(xc, {"h." + k: v for k, v in so.items()}, "h", training), x, 31,
             training=training)


def test_x4_model_matches_reference_fixture():
    """Whole model with output_mode="x4" against the logits the reference produced (tests/golden/head_x4.npz;
    the reference's own shape check is test_lidar_encoder.py:281-293)."""
    from _util import golden
    from _gpu_util import build_product
    gd = golden("head_x4.npz")
    B, HW, N, G = 2, 64, 512, 16
    model = build_product("concat", G, num_classes=3, output_mode="x4")
    st = O.randomize_state({k: v.detach().clone() for k, v in model.state_dict().items()}, 21)
    for k, v in model.state_dict().items():
        if k.endswith("grid_tensor"):
            st[k] = v.clone()
    model.load_state_dict(st)
    model.cuda().eval()
    images, pts, _ = O.make_inputs(B, HW, N, G, 6)
    with torch.no_grad():
        z = model(images.cuda(), pts.cuda())
    assert z.shape == (2, 3, 64, 64)
    ref = torch.from_numpy(gd["logits"])
    assert (z.cpu() - ref).abs().max().item() < max(1e-4, 5e-6 * ref.abs().max().item())


@pytest.mark.parametrize("h,w,stride", [(9, 6, 2), (5, 11, 2), (6, 9, 1), (1, 7, 2), (33, 2, 2)])
def test_inverted_residual_non_square(h, w, stride):
    """Depthwise kernels on non-square / odd / degenerate maps (quad form of the stride-2 data gradient, 16-row segments)."""
    from src.models.camera_encoder import InvertedResidual
    torch.manual_seed(0)
    m = InvertedResidual(32, 64, stride=stride, expansion_ratio=6)
    x = torch.randn(2, 32, h, w, generator=torch.Generator().manual_seed(h * 100 + w))
    _compare(m, lambda xx, st: O.inverted_residual(xx, {("." + k): v for k, v in st.items()}, "", 32, 64, stride, 6, True), x,
             seed=h + w)


@pytest.mark.parametrize("shape", [(2, 13, 19, 8), (1, 70, 66, 72), (2, 33, 64, 384), (1, 192, 200, 32)])   # the last: a 1200-row slab (64-lane reduce)
def test_dw_stride1_backward_forms_agree(shape):
    """The three forms of the stride-1 depthwise backward (separate data / weight kernels, fused column walk, fused tile
    kernel staged through LDS) on odd and tile-crossing shapes: same data gradient bits (identical fma order), weight
    gradient and BatchNorm-backward sums to rounding.  The forms share their operand helpers, so agreement is not truth:
    every form is held to a float64 reference in tests/test_gpu_conv_kernels.py (test_dw_bwd_stride1_forms and the ladders)."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream, workspace
    B, H, W, C = shape
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    D, Y, x, w = rnd(B * H * W, C), rnd(B * H * W, C), rnd(B * H * W, C), rnd(C, 9)
    al, be, ga, sc, sh, mean = rnd(C), rnd(C) * 0.1, rnd(C) * 0.1, rnd(C).abs() + 0.5, rnd(C) * 0.2, rnd(C) * 0.1
    inv = rnd(C).abs() + 0.5
    outs = []
    prev = lib.kd_set_dw_bwd_mode(0)
    try:
        for mode in (0, 1, 2):
            lib.kd_set_dw_bwd_mode(mode)
            rows = lib.kd_dwconv_bwd_stat_rows(B * H * W, C)
            gx = torch.empty(B * H * W, C, device="cuda")
            part = torch.full((rows * 2 * C,), float("nan"), device="cuda")
            dw = torch.empty(C, 9, device="cuda")
            nbytes = lib.kd_dwconv_bwd_ws_bytes(B * H * W, C)
            ws = workspace(nbytes, gx.device)
            lib.call("kd_dwconv3x3_bwd", P(D), P(Y), P(al), P(be), P(ga), None, None, 0, P(x), P(sc), P(sh), 2, P(mean), P(inv), P(w), P(gx),
                     P(part), P(dw), B, H, W, C, 1, P(ws), nbytes, stream())
            torch.cuda.synchronize()
            outs.append((gx, part.view(rows, 2, C).double().sum(0), dw))
    finally:
        lib.kd_set_dw_bwd_mode(prev)
    (g0, p0, w0), (g1, p1, w1), (g2, p2, w2) = outs
    assert torch.equal(g0, g1) and torch.equal(g0, g2)
    for p, wv in ((p1, w1), (p2, w2)):
        assert ((p - p0).abs().max() / p0.abs().max()).item() < 1e-5        # fp32 partial sums in a different order
        assert ((wv - w0).abs().max() / w0.abs().max()).item() < 2e-5


@pytest.mark.parametrize("shape", [(2, 13, 19, 8), (2, 40, 36, 32), (1, 17, 9, 48)])
@pytest.mark.parametrize("deferred", (True, False))
def test_dw_backward_with_residual_addend(shape, deferred):
    """kd_dwconv3x3_bwd_add (the residual gradient of a depthwise-first inverted-residual block added inside the one-pass
    backward, before the activation mask) against kd_dwconv3x3_bwd followed by the add: materialised input -- the sum, same
    bits; deferred input -- (conv^T dy + addend) * act'(.) and the BatchNorm-backward sums of THAT, checked in float64."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream, workspace
    B, H, W, C = shape
    assert lib.kd_dwconv3x3_bwd_add_supported(C, W, 1) == 1
    M = B * H * W
    g = torch.Generator(device="cuda").manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    D, Y, x, w, add = rnd(M, C), rnd(M, C), rnd(M, C), rnd(C, 9), rnd(M, C)
    al, be, ga, sc, sh, mean = rnd(C), rnd(C) * 0.1, rnd(C) * 0.1, rnd(C).abs() + 0.5, rnd(C) * 0.2, rnd(C) * 0.1
    inv = rnd(C).abs() + 0.5
    rows = lib.kd_dwconv_bwd_stat_rows(M, C)
    nbytes = lib.kd_dwconv_bwd_ws_bytes(M, C)
    ws = workspace(nbytes, D.device)
    d = (P(sc), P(sh), 2, P(mean), P(inv)) if deferred else (None, None, 0, None, None)

    def run(addend):
        gx = torch.full((M, C), float("nan"), device="cuda")
        part = torch.full((rows * 2 * C,), float("nan"), device="cuda") if deferred else None
        dw = torch.full((C, 9), float("nan"), device="cuda")
        head = (P(D), P(Y), P(al), P(be), P(ga), None, None, 0, P(x), *d, P(w))
        tail = (P(gx), P(part), P(dw), B, H, W, C, 1, P(ws), nbytes, stream())
        if addend is None:
            lib.call("kd_dwconv3x3_bwd", *head, *tail)
        else:
            lib.call("kd_dwconv3x3_bwd_add", *head, P(addend), *tail)
        torch.cuda.synchronize()
        return gx, (part.view(rows, 2, C).double().sum(0) if deferred else None), dw
    gx0, _, dw0 = run(None) if not deferred else (None, None, None)
    gx1, p1, dw1 = run(add)
    if not deferred:
        assert torch.equal(gx1, gx0 + add) and torch.equal(dw1, dw0)
        return
    # deferred: rebuild from the UNMASKED data gradient (plain-input call: same conv^T dy bits) in float64
    d = (None, None, 0, None, None)
    raw, _, dw0 = run(None)
    z = x.double() * sc.double() + sh.double()
    mask = ((z > 0) & (z < 6)).double()
    want = (raw.double() + add.double()) * mask
    assert (gx1.double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    xhat = (x.double() - mean.double()) * inv.double()
    s1, s2 = want.sum(0), (want * xhat).sum(0)
    assert ((p1[0] - s1).abs().max() / s1.abs().max()).item() < 1e-5 and ((p1[1] - s2).abs().max() / s2.abs().max()).item() < 1e-5


@pytest.mark.parametrize("shape", [(2, 13, 19, 8), (1, 70, 66, 72), (2, 32, 64, 192), (1, 9, 9, 384)])
@pytest.mark.parametrize("deferred", (True, False))
def test_dw_stride2_backward_forms_agree(shape, deferred):
    """Stride-2 depthwise backward: separate data / weight kernels against the fused quad walk, on odd and even sizes,
    with a deferred (BatchNorm + ReLU6 on load) and a materialised input: same data gradient bits, weight gradient and
    BatchNorm-backward sums to rounding.  The absolute check of both forms against float64 is
    tests/test_gpu_conv_kernels.py::test_dw_bwd_stride2_forms (and the ladders there)."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream, workspace
    B, H, W, C = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator(device="cuda").manual_seed(9)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")
    D, Y, x, w = rnd(B * Ho * Wo, C), rnd(B * Ho * Wo, C), rnd(B * H * W, C), rnd(C, 9)
    al, be, ga, sc, sh, mean = rnd(C), rnd(C) * 0.1, rnd(C) * 0.1, rnd(C).abs() + 0.5, rnd(C) * 0.2, rnd(C) * 0.1
    inv = rnd(C).abs() + 0.5
    outs = []
    prev = lib.kd_set_dw_bwd_mode(0)
    try:
        for mode in (0, 3):
            lib.kd_set_dw_bwd_mode(mode)
            rows = lib.kd_dwconv_bwd_stat_rows(B * H * W, C)
            gx = torch.full((B * H * W, C), float("nan"), device="cuda")
            part = torch.full((rows * 2 * C,), float("nan"), device="cuda") if deferred else None
            dw = torch.full((C, 9), float("nan"), device="cuda")
            nbytes = lib.kd_dwconv_bwd_ws_bytes(B * Ho * Wo, C)
            ws = workspace(nbytes, gx.device)
            lib.call("kd_dwconv3x3_bwd", P(D), P(Y), P(al), P(be), P(ga), None, None, 0, P(x), P(sc) if deferred else None,
                     P(sh) if deferred else None, 2, P(mean) if deferred else None, P(inv) if deferred else None, P(w), P(gx), P(part), P(dw),
                     B, H, W, C, 2, P(ws), nbytes, stream())
            torch.cuda.synchronize()
            outs.append((gx, part.view(rows, 2, C).double().sum(0) if deferred else None, dw))
    finally:
        lib.kd_set_dw_bwd_mode(prev)
    (g0, p0, w0), (g1, p1, w1) = outs
    assert torch.equal(g0, g1)
    if deferred:
        assert ((p1 - p0).abs().max() / p0.abs().max()).item() < 1e-5
    assert ((w1 - w0).abs().max() / w0.abs().max()).item() < 2e-5


def test_fpn_sum_single_pass_equals_accumulate():
    """kd_bilinear_sum_fwd (the FPN sum of fusion_module.py:58-63 in one pass) against lateral-by-lateral
    kd_bilinear_accum_fwd: the same bits, for 1..3 laterals with mixed geometry and activations."""
    from kdrt import ops
    from kdrt.ops import lib, P, stream
    g = torch.Generator().manual_seed(3)
    B, Ho, Wo, C = 2, 12, 10, 128
    geo = [(12, 10), (6, 5), (3, 4)]
    ins = [torch.randn(B * h * w, C, generator=g).cuda() for h, w in geo]
    scs = [torch.rand(C, generator=g).cuda() + 0.5 for _ in geo]
    shs = [torch.randn(C, generator=g).cuda() for _ in geo]
    acts = [ops.ACT_RELU, ops.ACT_NONE, ops.ACT_RELU]
    for n in (1, 2, 3):
        ref = torch.empty(B * Ho * Wo, C, device="cuda")
        for i in range(n):
            lib.call("kd_bilinear_accum_fwd", P(ins[i]), P(scs[i]), P(shs[i]), acts[i], P(ref), int(i > 0), B, geo[i][0],
                     geo[i][1], Ho, Wo, C, stream())
        a = [(P(ins[i]), P(scs[i]), P(shs[i]), acts[i], geo[i][0], geo[i][1]) for i in range(n)]
        a += [(None, None, None, 0, 0, 0)] * (3 - n)
        out = torch.full((B * Ho * Wo, C), float("nan"), device="cuda")
        lib.call("kd_bilinear_sum_fwd", *a[0], *a[1], *a[2], P(out), B, Ho, Wo, C, stream())
        torch.cuda.synchronize()
        assert torch.equal(out, ref), n


@pytest.mark.parametrize("case", ["ir_s1_res", "ir_s2", "ir_s2_128", "ir_t1", "ir_wide", "dwsep", "dwsep_64"])
@pytest.mark.parametrize("hw", [(32, 32), (20, 27), (7, 9)])
def test_dw_pw_inference_fusion_same_bits(case, hw):
    """Eval / no-grad tails that end in (depthwise 3x3, 1x1): the one-kernel form (csrc/kd_block.hip) against the two
    separate kernels -- the same bits, on maps that do and do not fill the 8 x 16 / 8 x 8 pixel tiles, stride 1 and 2, with
    and without the residual, deferred and materialised depthwise inputs (camera_encoder.py:30-42, fusion_module.py:25-34)."""
    from kdrt import ops, units as U
    from src.models.camera_encoder import InvertedResidual
    from src.models.fusion_module import DWSeparableConv
    if ops.get_gemm_arithmetic() != "split":
        pytest.skip("the fused tail exists in the split arithmetic only")
    torch.manual_seed(1)
    m, cin = {"ir_s1_res": (InvertedResidual(32, 32, 1, 6), 32), "ir_s2": (InvertedResidual(32, 64, 2, 6), 32),
              "ir_s2_128": (InvertedResidual(64, 128, 2, 6), 64), "ir_t1": (InvertedResidual(32, 32, 1, 1), 32), "ir_wide": (InvertedResidual(128, 128, 1, 6), 128),
              "dwsep": (DWSeparableConv(128, 128), 128), "dwsep_64": (DWSeparableConv(128, 64), 128)}[case]
    _rand_state(m, 41)
    m = m.cuda().eval()
    x = torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(7)).cuda()
    outs = []
    prev = U.DW_PW_FUSED[0]
    try:
        for fused in (0, 2):                          # 0: two kernels, 2: one kernel for every supported shape
            U.DW_PW_FUSED[0] = fused
            with torch.no_grad():
                outs.append(m(x).clone())
    finally:
        U.DW_PW_FUSED[0] = prev
    assert outs[0].shape == outs[1].shape and torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_dw_pw_inference_fusion_refuses_unsupported_shapes():
    """kd_dw_pw_infer has no silent fallback: a shape without an instance is a KDError (the host logic asks
    kd_dw_pw_infer_supported first and keeps the two separate kernels)."""
    from kdrt import KDError
    from kdrt.ops import lib, P, stream
    assert lib.kd_dw_pw_infer_supported(384, 64, 1) == 1 and lib.kd_dw_pw_infer_supported(192, 64, 2) == 1
    assert lib.kd_dw_pw_infer_supported(48, 64, 1) == 0 and lib.kd_dw_pw_infer_supported(64, 96, 1) == 0
    assert lib.kd_dw_pw_infer_supported(64, 32, 2) == 0 and lib.kd_dw_pw_infer_supported(64, 64, 3) == 0
    x = torch.zeros(1 * 8 * 8, 48, device="cuda")
    v = torch.ones(96, device="cuda")
    w = torch.zeros(96 * 48, device="cuda")
    out = torch.empty(64, 96, device="cuda")
    with pytest.raises(KDError):
        lib.call("kd_dw_pw_infer", P(x), None, None, 0, P(w), P(v), P(v), 1, P(w), None, P(v), P(v), 1, None, 0, P(out), 96, 1, 8, 8, 48, 1, 96,
                 stream())


def test_chain_pairs_match_separate_chains(monkeypatch):
    """stem -> stage1 and stage2 -> stage3 as PairChainFn (the first block's output never materialised: read raw with its
    BatchNorm coefficients by the second block's first convolution AND by its residual connection; the residual gradient
    folded into that convolution's data-gradient kernel before the activation mask) against the separate chains: the same
    forward bits, gradients to summation order (the BatchNorm-backward sums come from different kernels)."""
    from kdrt import units
    from src.models.camera_encoder import TwinLiteEncoder
    torch.manual_seed(3)
    x = torch.randn(2, 3, 96, 80, device="cuda")
    up = None
    res = {}
    for pairs in (True, False):
        monkeypatch.setattr(units, "_CHAIN_PAIRS", pairs)
        enc = TwinLiteEncoder(return_multiscale=True)
        _rand_state(enc, 17)
        enc = enc.cuda().train()
        maps = enc(x, _skip_stages=("stage2",))                   # what CompleteSegmentationModel passes when its FPN does not read stage 2
        assert ("stage2" in maps) == (not pairs)
        assert set(enc(x)) == {"stage2", "stage3", "stage4", "stage5"}     # called plainly: the reference's key set, always
        if up is None:
            up = {k: torch.randn(v.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5)) for k, v in maps.items()}
        sum((maps[k] * up[k]).sum() for k in ("stage3", "stage4", "stage5")).backward()
        torch.cuda.synchronize()
        res[pairs] = ({k: maps[k].detach().clone() for k in ("stage3", "stage4", "stage5")},
                      {n: p.grad.detach().clone() for n, p in enc.named_parameters()},
                      {n: b.detach().clone() for n, b in enc.named_buffers()})
    (m1, g1, b1), (m0, g0, b0) = res[True], res[False]
    for k in m0:
        assert torch.equal(m1[k].view(torch.int32), m0[k].view(torch.int32)), k
    for n in b0:
        assert torch.equal(b1[n], b0[n]), n                      # running statistics: same forward, same bits
    # (a BatchNorm shift that feeds another training-mode BatchNorm has a mathematically ZERO gradient -- what both runs hold
    # there is the rounding residue of a million-term sum, so the floor of the comparison is the largest gradient in the model)
    gmax = max(v.abs().max().item() for v in g0.values())
    for n in g0:
        scale = max(g0[n].abs().max().item(), 1e-2 * gmax)
        assert (g1[n] - g0[n]).abs().max().item() <= 2e-5 * scale, (n, (g1[n] - g0[n]).abs().max().item(), scale)


def test_stem_inference_kernel_same_bits_as_two_passes(monkeypatch):
    """Inference (eval, no autograd): the stem's conv + BatchNorm + ReLU6 run as ONE kernel (kd_stem_conv_fwd_infer); with
    _STEM_INFER = False as conv + kd_bn_act_apply.  Same operations in the same order: every multiscale map has the same bits."""
    from kdrt import units
    from src.models.camera_encoder import TwinLiteEncoder
    torch.manual_seed(4)
    x = torch.randn(3, 3, 70, 94, device="cuda")
    enc = TwinLiteEncoder(return_multiscale=True)
    _rand_state(enc, 23)
    enc = enc.cuda().eval()
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(units, "_STEM_INFER", fused)
        with torch.no_grad():
            res[fused] = enc(x)
    assert set(res[True]) == set(res[False]) == {"stage2", "stage3", "stage4", "stage5"}
    for k in res[True]:
        assert torch.equal(res[True][k].view(torch.int32), res[False][k].view(torch.int32)), k


@pytest.mark.parametrize("rows,C,pstride", [(5, 32, 32), (256, 128, 128), (1023, 64, 64), (1024, 32, 32), (2048, 192, 192), (5120, 128, 128),
                                            (8192, 128, 256), (8192, 64, 64), (8193, 64, 64), (20000, 32, 32), (3000, 6, 6), (2048, 36, 40)])
def test_bn_finalize_on_slabs_of_every_height(rows, C, pstride):
    """kd_bn_finalize_train / kd_bn_bwd_finalize reduce a [rows][2][pstride] slab: short slabs (16 channels x 64 row lanes per workgroup),
    tall ones (>= 1024 rows, C % 4 == 0: four channels x 256 row lanes), above 8192 rows a pre-reduction first.  Every class, plus channel
    counts the tall form must refuse, against float64 sums of the same slab (BatchNorm2d training forward / backward, torch semantics)."""
    from kdrt import ops
    g = torch.Generator().manual_seed(rows * 7 + C)
    slab = torch.randn(rows, 2, pstride, generator=g)
    slab[:, 1] = slab[:, 1].abs() * 3 + 2.0                    # sum of squares: keeps the variance positive
    count = rows * 10
    s = slab.double().sum(0)[:, :C]
    mu = s[0] / count
    var = (s[1] / count - mu * mu).clamp_min(0)
    bn = torch.nn.BatchNorm1d(C).cuda()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g))
    gam, bet = bn.weight.detach().double().cpu(), bn.bias.detach().double().cpu()
    bnc = ops.BNC(C, torch.device("cuda"))
    ops.bn_finalize_train(slab.cuda().contiguous(), rows, C, count, bn, bnc, pstride=pstride)
    inv = 1.0 / torch.sqrt(var + bn.eps)
    for got, want in ((bnc.mean, mu), (bnc.invstd, inv), (bnc.scale, gam * inv), (bnc.shift, bet - mu * gam * inv)):
        assert max_err(got, want.float())[1] < 2e-6
    assert max_err(bn.running_mean, (0.1 * mu).float())[1] < 2e-6
    assert max_err(bn.running_var, (0.9 + 0.1 * var * count / (count - 1)).float())[1] < 2e-6
    assert int(bn.num_batches_tracked) == 1
    # backward coefficients from a second slab (sum G, sum G*xhat) with the statistics just produced
    slab2 = torch.randn(rows, 2, pstride, generator=g)
    t = slab2.double().sum(0)[:, :C]
    dgamma, dbeta, abg, _ = ops.bn_bwd_finalize(slab2.cuda().contiguous(), rows, C, count, bn.weight, bnc, True, pstride=pstride)
    assert max_err(dbeta, t[0].float())[1] < 2e-6 and max_err(dgamma, t[1].float())[1] < 2e-6
    a = gam * bnc.invstd.double().cpu()
    c1, c2 = t[0] / count, t[1] / count
    i32, m32 = bnc.invstd.double().cpu(), bnc.mean.double().cpu()
    for got, want in ((abg[0], a), (abg[1], -a * c2 * i32), (abg[2], a * (c2 * i32 * m32 - c1))):
        assert max_err(got, want.float())[1] < 2e-6
