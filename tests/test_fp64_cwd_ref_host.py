"""CPU tests of the channel-wise distillation term's float64 reference (tests/_fp64_cwd_ref.py) and of its host side: the reference
against torch autograd of a plain float64 log_softmax / KL expression, a plain fp32 evaluation inside the reference's bound on
every case (the bound is attainable), three negative controls outside it (the bound is not vacuous), ChannelKD validation, the
ablation script's knobs, the refusals that need no GPU, and the C ABI of the two entry points (declared, exported, the workspace
formula, every refusal before a launch)."""
import ctypes
import inspect
import re

import pytest
import torch

import _fp64_cwd_ref as V
from kdrt.losses import ChannelKD, channel_kd          # ImportError without the feature

_CACHE = {}


def _case(case):
    """the case's CPU inputs and its float64 reference, computed once"""
    if case not in _CACHE:
        s, t, tau, gcoef, gdev, k = V.case_setup(case, "cpu")
        _CACHE[case] = (s, t, tau, k, V.cwd(s.double(), t.double(), tau, k))
    return _CACHE[case]


def _worst(ref, got):
    """the largest |got - ref| / bound over stats, val and ds (0 / 0 counts as inside)"""
    w = 0.0
    for key in ("stats", "val", "ds"):
        v, e = ref[key]
        d = (torch.as_tensor(got[key][0]).double() - v).abs()
        r = torch.where(d > 0, d / torch.as_tensor(e).double().clamp_min(1e-300), torch.zeros_like(d))
        w = max(w, r.max().item())
    return w


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_reference_against_torch_autograd(case):
    s, t, tau, k, ref = _case(case)
    B, HW, C = s.shape
    sd = s.double().requires_grad_()
    lps = torch.log_softmax(sd / tau, 1)
    lpt = torch.log_softmax(t.double() / tau, 1)
    want = tau * tau / (B * C) * (lpt.exp() * (lpt - lps)).sum()
    want.backward()
    v = ref["val"][0]
    assert abs(v.item() - want.item()) <= 1e-12 * abs(want.item()), (v.item(), want.item())
    # dCWD/dS = tau / (B*C) * (phi(s) - phi(t)); the reference's ds carries k in that coefficient's place
    g = ref["ds"][0] * (tau / (B * C) / k)
    d = (g - sd.grad).abs().max().item()
    assert d <= 1e-12 * sd.grad.abs().max().item() + 1e-300, d
    assert v.item() >= 0.0 and (HW > 1 or v.item() == 0.0)
    assert torch.allclose(ref["phi_s"].sum(1), torch.ones(B, C, dtype=torch.float64), atol=1e-12, rtol=0)


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_plain_fp32_evaluation_meets_the_bound(case):
    s, t, tau, k, ref = _case(case)
    got = V.cwd(s, t, tau, k)
    assert got["ds"][0].dtype == torch.float32
    w = _worst(ref, got)
    print(V.case_id(case), "fp32 evaluation: worst |d| / bound", w)
    assert w <= 1.0
    assert bool(torch.isfinite(ref["val"][1])) and bool(torch.isfinite(ref["ds"][1]).all()) and bool(torch.isfinite(ref["stats"][1]).all())


@pytest.mark.parametrize("case", V.CASES[1:], ids=V.case_id)
def test_negative_controls_violate_the_bound(case):
    """inputs rounded to bf16, tau in place of tau^2, the student's log-sum-exp off by 1e-5 relative: each evaluated in float64,
    each outside the bound.  At tau == 1 the second control is no error at all (tau == tau^2): there it must reproduce the
    reference exactly, and it must violate the bound on every case with another tau."""
    s, t, tau, k, ref = _case(case)
    sd, td = s.double(), t.double()
    w = _worst(ref, V.cwd(sd, td, tau, k, snap=torch.bfloat16))
    print(V.case_id(case), "bf16 inputs:", w)
    assert w > 1.0
    w = _worst(ref, V.cwd(sd, td, tau, k, coef_power=1))
    print(V.case_id(case), "tau for tau^2:", w)
    assert (w == 0.0) if tau == 1.0 else (w > 1.0)
    w = _worst(ref, V.cwd(sd, td, tau, k, lse_rel=1e-5))
    print(V.case_id(case), "log-sum-exp off by 1e-5:", w)
    assert w > 1.0


def test_single_position_is_exactly_zero_and_constant_columns_are_uniform():
    s, t, tau, k, ref = _case(V.CASES[0])
    assert ref["val"][0].item() == 0.0 and bool((ref["ds"][0] == 0).all()) and bool((ref["stats"][0][..., 1::2] == 0).all())
    s, t, tau, k, ref = _case(V.CASES[4])
    HW = s.shape[1]
    for c, x in ((0, 0.0), (1, 1.5 / tau)):
        assert bool((ref["phi_s"][:, :, c] == 1.0 / HW).all())
        st = ref["stats"][0][:, c]
        assert bool((st[:, 0] == x).all()) and bool(((st[:, 1] - torch.log(torch.tensor(float(HW), dtype=torch.float64))).abs() < 1e-14).all())
    assert bool((s == 0).float().mean() > 0.3), "the post-ReLU scene carries many exact zeros"


def test_layout_and_counts():
    assert V.layout(4096, 128) == (32, 8, 512, 8) and V.layout(16384, 4) == (1, 256, 16384, 1) and V.layout(257, 36) == (9, 28, 1792, 1)
    assert V.layout(100, 512) == (128, 2, 128, 1) and V.layout(129, 512)[3] == 2
    assert V.n_seq(4096, 128) == (10, 64 + 8 + 8, 4 * 64 + 9) and V.n_seq(1, 4) == (3, 3, 13) and V.n_seq(63, 8) == (3, 1 + 63 + 1, 13)
    assert V.ws_bytes(256, 4096, 128) == 4 * 256 * 8 * 513


def test_channel_kd_validation():
    spec = ChannelKD()
    assert spec.tau == 4.0 and ChannelKD(2) == ChannelKD(2.0)
    with pytest.raises(Exception):
        spec.tau = 2.0
    for bad in (0.0, -1.0, float("nan"), float("inf"), "4.0", True, None):
        with pytest.raises(ValueError):
            ChannelKD(tau=bad)


def test_refusals_that_need_no_gpu():
    from kdrt import KDError
    from kdrt.kd import KDStep
    from kdrt.losses import kd_objective, kd_objective_backward
    from src.training.trainer import KDTrainer
    a = torch.randn(2, 8, 4, 4, requires_grad=True)
    for b, tau in ((torch.randn(2, 8, 4, 4), 4.0),            # CPU tensors
                   (torch.randn(2, 8, 4, 5), 4.0), (torch.randn(2, 4, 4, 4), 4.0), (torch.randn(2, 8, 16), 4.0)):
        with pytest.raises(KDError):
            channel_kd(a, b, tau)
    for C in (6, 516, 2):
        with pytest.raises(KDError, match="channels"):
            channel_kd(torch.randn(1, C, 2, 2), torch.randn(1, C, 2, 2))
    with pytest.raises(KDError):
        channel_kd(a.double(), torch.randn(2, 8, 4, 4).double())
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            channel_kd(a, a.detach(), tau)
    assert a.grad is None
    # the layers above refuse anything that is not a ChannelKD before they touch a model
    for bad in ("cwd", 4.0, ChannelKD):
        with pytest.raises(ValueError):
            KDStep(None, None, None, feature_loss=bad)
        with pytest.raises(ValueError):
            KDTrainer(None, None, None, None, torch.device("cpu"), feature_loss=bad)
        with pytest.raises(KDError):
            kd_objective(a, {}, a, {}, None, feature_loss=bad)
    for fn in (kd_objective, kd_objective_backward, KDTrainer.__init__):
        p = inspect.signature(fn).parameters
        assert "feature_loss" in p and p["feature_loss"].default is None, fn


def test_ablation_script_reads_the_new_names_and_keeps_the_old():
    import train_with_fusion_ablation as S
    assert S.feature_loss_from_env({}) is None and S.feature_loss_from_env({"KD_FEATURE_LOSS": "mse"}) is None
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "mse", "KD_CWD_TAU": "2"}) is None
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "cwd"}) == ChannelKD(tau=4.0)
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "1.5"}) == ChannelKD(tau=1.5)
    for bad in ({"KD_FEATURE_LOSS": "kl"}, {"KD_FEATURE_LOSS": "CWD"}, {"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "0"},
                {"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "-2"}, {"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "nan"}):
        with pytest.raises(ValueError):
            S.feature_loss_from_env(bad)
    assert S.hard_loss_from_env({"KD_FEATURE_LOSS": "cwd"}) is None          # the hard-label knob does not read the new names
    assert "KD_FEATURE_LOSS" in S.__doc__ and "KD_CWD_TAU" in S.__doc__


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_feat_cwd_fwd_bwd", "kd_feat_cwd_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    V_, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert protos["kd_feat_cwd_ws_bytes"] == (Z, [I, I, I])
    assert protos["kd_feat_cwd_fwd_bwd"] == (I, [V_, V_, I, I, I, F, F, V_, V_, V_, V_, V_, Z, V_])


def test_workspace_query_and_refusals_before_any_launch():
    from kdrt.lib import lib
    q = lib.kd_feat_cwd_ws_bytes
    for B, HW, C, _, _ in V.CASES + [(256, 4096, 128, 4.0, "bench"), (3, 129, 512, 1.0, "two chunks")]:
        assert q(B, HW, C) == V.ws_bytes(B, HW, C) > 0
    assert q(1, 8, 6) == 0 and q(1, 8, 516) == 0 and q(1, 0, 8) == 0 and q(0, 8, 8) == 0
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch

    def rc(s=one, t=one, B=1, HW=8, C=8, tau=1.0, val=one, ws=one, ws_bytes=None):
        nb = V.ws_bytes(max(B, 1), max(HW, 1), 8) if ws_bytes is None else ws_bytes
        return lib.kd_feat_cwd_fwd_bwd(s, t, B, HW, C, tau, 1.0, None, val, one, None, ws, nb, None)
    for kw in (dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")), dict(tau=float("inf")), dict(s=None), dict(t=None), dict(val=None),
               dict(ws=None)):
        assert rc(**kw) == -1, kw                                   # KD_ERR_ARG
        assert b"kd_feat_cwd_fwd_bwd" in lib.kd_last_error_string()
    for kw in (dict(C=6), dict(C=516), dict(C=0), dict(HW=0), dict(B=0), dict(B=-1)):
        assert rc(**kw) == -4, kw                                   # KD_ERR_SHAPE
        assert b"kd_feat_cwd_fwd_bwd" in lib.kd_last_error_string()
    assert rc(ws_bytes=V.ws_bytes(1, 8, 8) - 1) == -3               # KD_ERR_WORKSPACE
    assert rc(s=ctypes.c_void_p(20)) == -2                          # KD_ERR_ALIGN: a float4 load from there would fault
    assert b"kd_feat_cwd_fwd_bwd" in lib.kd_last_error_string()
