"""kd_block_infer (csrc/kd_block.hip: a whole eval-mode InvertedResidual in one kernel, the 6x hidden tensor never written)
against the path it replaces -- kd_pwconv_gemm for the expand, then kd_dw_pw_infer -- bit for bit, at the C ABI and through
InvertedResidual, and the dispatch rules around it (reference block: camera_encoder.py:19-44)."""
import pytest
import torch

import kd_oracle as O

pytestmark = pytest.mark.gpu

RELU6, NONE = 2, 0

# (Cin, Ch, Cout, stride, residual, B, H, W): partial tiles in both directions at stride 2 (output 9 x 10 on 8 x 8 tiles); 3 x 3
# tiles of 8 x 16 with the last row and column partial and a residual inside a wider buffer at stride 1; one chunk on a map
# smaller than one tile for each instance
CASES = {
    "s2_192": (32, 192, 64, 2, False, 2, 17, 19),
    "s1_384_res": (64, 384, 64, 1, True, 2, 20, 36),
    "s2_one_chunk": (32, 32, 64, 2, False, 2, 5, 7),
    "s1_one_chunk": (64, 32, 64, 1, True, 2, 5, 7),
}


@pytest.fixture
def split_arith():
    from kdrt import ops
    prev = ops.set_gemm_arithmetic("split")
    yield
    ops.set_gemm_arithmetic(prev)


def _affine(g, n):
    """BatchNorm as (scale, shift): magnitudes 0.5 .. 1.5, about a third of the scales negative"""
    sc = (torch.rand(n, generator=g) + 0.5) * torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0)
    return sc.cuda(), torch.randn(n, generator=g).cuda()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_block_infer_same_bits_as_gemm_then_tail(case, bias, split_arith):
    from kdrt import ops
    from kdrt.ops import lib, P, stream
    Cin, Ch, Cout, s, residual, B, H, W = CASES[case]
    g = torch.Generator().manual_seed(len(case) * 7 + int(bias))
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    M, Mo = B * H * W, B * Ho * Wo
    x = (2.0 * torch.randn(M, Cin, generator=g)).cuda()
    we = (1.5 * torch.randn(Ch, Cin, generator=g) / Cin ** 0.5).cuda()
    eb = torch.randn(Ch, generator=g).cuda() if bias else None
    esc, esh = _affine(g, Ch)
    esh = esh + 3.0                                      # centre of the ReLU6 range: both clamps are hit
    wd = torch.randn(Ch, 9, generator=g).cuda()
    dsc, dsh = _affine(g, Ch)
    dsh = dsh + 3.0
    wp = (torch.randn(Cout, Ch, generator=g) / Ch ** 0.5).cuda()
    pb = torch.randn(Cout, generator=g).cuda() if bias else None
    psc, psh = _affine(g, Cout)
    resbuf = torch.randn(Mo, 80, generator=g).cuda() if residual else None
    res = resbuf[:, 8:8 + Cout] if residual else None
    ldres = 80 if residual else 0

    hid = torch.empty(M, Ch, device="cuda")
    ops.pw_gemm(x, we, hid, M=M, K=Cin, N=Ch, bias=eb, epi=0)
    ref = torch.full((Mo, Cout), float("nan"), device="cuda")
    lib.call("kd_dw_pw_infer", P(hid), P(esc), P(esh), RELU6, P(wd), P(dsc), P(dsh), RELU6, P(wp), P(pb), P(psc), P(psh), NONE,
             P(res), ldres, P(ref), Cout, B, H, W, Ch, s, Cout, stream())
    out = torch.full((Mo, Cout), float("nan"), device="cuda")
    lib.call("kd_block_infer", P(x), P(we), P(eb), P(esc), P(esh), RELU6, P(wd), P(dsc), P(dsh), RELU6, P(wp), P(pb), P(psc),
             P(psh), NONE, P(res), ldres, P(out), Cout, B, H, W, Cin, Ch, s, Cout, stream())
    torch.cuda.synchronize()
    z = hid * esc + esh
    assert (z < 0).float().mean() > 0.05 and (z > 6).float().mean() > 0.05      # ReLU6 clamps at both ends on a visible share
    assert torch.isfinite(ref).all()
    assert torch.equal(out, ref)


def _block(cin, cout, stride, seed):
    from src.models.camera_encoder import InvertedResidual
    m = InvertedResidual(cin, cout, stride=stride)
    m.load_state_dict(O.randomize_state({k: v.detach().clone() for k, v in m.state_dict().items()}, seed))
    return m.cuda()


def _both_modes(m, x, grad=False):
    from kdrt import units as U
    outs = []
    prev = U.BLOCK_INFER[0]
    try:
        for mode in (0, 2):
            U.BLOCK_INFER[0] = mode
            with torch.set_grad_enabled(grad):
                outs.append(m(x).detach().clone())
    finally:
        U.BLOCK_INFER[0] = prev
    return outs


@pytest.mark.parametrize("cin,cout,stride,hw", [(32, 64, 2, (17, 19)), (64, 64, 1, (20, 36)), (32, 64, 2, (5, 7)), (64, 64, 1, (5, 7))])
def test_inverted_residual_one_kernel_same_bits(cin, cout, stride, hw, split_arith, monkeypatch):
    from kdrt import units as U
    m = _block(cin, cout, stride, 23).eval()
    x = torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(5)).cuda()
    calls = []
    real = U.block_forward_final
    monkeypatch.setattr(U, "block_forward_final", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    old, new = _both_modes(m, x)
    assert len(calls) == 1                               # mode 2 took the one-kernel form, mode 0 did not
    assert torch.isfinite(old).all() and torch.equal(old, new)


def test_block_infer_supported_and_refusal():
    from kdrt import KDError
    from kdrt.ops import lib, P, stream
    assert lib.kd_block_infer_supported(32, 192, 64, 2) == 1 and lib.kd_block_infer_supported(64, 384, 64, 1) == 1
    assert lib.kd_block_infer_supported(32, 32, 64, 2) == 1 and lib.kd_block_infer_supported(64, 32, 64, 1) == 1
    assert lib.kd_block_infer_supported(48, 192, 64, 2) == 0 and lib.kd_block_infer_supported(48, 384, 64, 1) == 0      # Cin 48
    assert lib.kd_block_infer_supported(32, 192, 96, 2) == 0 and lib.kd_block_infer_supported(64, 384, 96, 1) == 0      # Cout 96
    assert lib.kd_block_infer_supported(32, 192, 64, 3) == 0 and lib.kd_block_infer_supported(64, 384, 64, 3) == 0      # stride 3
    assert lib.kd_block_infer_supported(32, 40, 64, 2) == 0 and lib.kd_block_infer_supported(64, 40, 64, 1) == 0        # Ch 40
    x = torch.zeros(8 * 8, 48, device="cuda")
    w = torch.zeros(96 * 96, device="cuda")
    v = torch.ones(96, device="cuda")
    out = torch.empty(64, 96, device="cuda")
    with pytest.raises(KDError):
        lib.call("kd_block_infer", P(x), P(w), None, P(v), P(v), RELU6, P(w), P(v), P(v), RELU6, P(w), None, P(v), P(v), NONE, None, 0,
                 P(out), 96, 1, 8, 8, 48, 96, 1, 96, stream())


def _never(*a, **k):
    raise AssertionError("the one-kernel block must not be reached here")


def test_fp32_arithmetic_keeps_the_old_path(monkeypatch):
    from kdrt import ops, units as U
    m = _block(64, 64, 1, 31).eval()
    x = torch.randn(2, 64, 20, 36, generator=torch.Generator().manual_seed(6)).cuda()
    monkeypatch.setattr(U, "block_forward_final", _never)
    prev = ops.set_gemm_arithmetic("fp32")
    try:
        old, new = _both_modes(m, x)
    finally:
        ops.set_gemm_arithmetic(prev)
    assert torch.isfinite(old).all() and torch.equal(old, new)


@pytest.mark.parametrize("training", [True, False])
def test_training_and_grad_mode_never_reach_the_block_kernel(training, split_arith, monkeypatch):
    from kdrt import units as U
    monkeypatch.setattr(U, "block_forward_final", _never)
    for cin, stride, hw in ((32, 2, (17, 19)), (64, 1, (20, 36))):
        m = _block(cin, 64, stride, 37).train(training)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        x = torch.randn(2, cin, *hw, generator=torch.Generator().manual_seed(8)).cuda()
        outs = []
        prev = U.BLOCK_INFER[0]
        try:
            for mode in (0, 2):
                m.load_state_dict(state)                 # (training updates the running statistics: same start for both modes)
                U.BLOCK_INFER[0] = mode
                outs.append(m(x).detach().clone())       # grad mode on: training, or eval with autograd
        finally:
            U.BLOCK_INFER[0] = prev
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
