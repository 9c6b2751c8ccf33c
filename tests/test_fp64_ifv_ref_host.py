"""CPU tests of the intra-class feature variation distillation term's float64 reference (tests/_fp64_ifv_ref.py) and of its host
side: the closed-form gradient against float64 autograd of the value, the data-parallel claim, the planted label cases, the float32
yardstick, the exact inputs, IntraClassKD and the ablation script's knob, the feature_loss type checks of every layer, the refusals
that need no GPU, and the C ABI of the entry points (declared, exported, the slice count, every refusal before a launch)."""
import ctypes
import dataclasses
import inspect
import re

import pytest
import torch

import _fp64_ifv_ref as V
from kdrt.losses import IntraClassKD, intra_class_kd      # ImportError without the feature

# (B, n, Cs, Ct, NC)
SHAPES = [(1, 2, 8, 8, 2), (2, 64, 8, 8, 3), (3, 576, 36, 36, 5), (2, 153, 132, 256, 9), (2, 576, 128, 64, 16)]


@pytest.mark.parametrize("B, n, Cs, Ct, NC", SHAPES)
def test_reference_gradient_is_float64_autograd_of_the_reference_value(B, n, Cs, Ct, NC):
    S, T, y, _ = V.planted(B, n, Cs, Ct, NC, 3)
    S, T = S.double().requires_grad_(), T.double()
    val = V.value(S, T, y, NC)
    val.backward()
    d = V.direct(S.detach(), T, y, NC)
    assert abs(val.item() - d["val"].item()) <= 1e-15 * max(d["Sv"].item(), 1e-300)
    err = (S.grad - d["grad"]).abs()
    print(f"({B}, {n}, {Cs}, {Ct}, {NC}): value {val.item():.6g}, largest gradient entry {d['grad'].abs().max().item():.3g}, max |d| {err.max().item():.3g}")
    assert bool((err <= 1e-12 * d["M"] + 1e-18).all())
    assert bool((d["grad"][~V.kept_mask(y, NC)] == 0).all())
    if n > 2:
        assert d["val"].item() > 0 and d["grad"].abs().max().item() > 0


def test_mean_of_two_half_batches_is_the_whole_batch():
    S, T, y, _ = V.planted(4, 100, 12, 8, 4, 9)
    S, T = S.double(), T.double()
    whole = V.direct(S, T, y, 4)
    lo, hi = V.direct(S[:2], T[:2], y[:2], 4), V.direct(S[2:], T[2:], y[2:], 4)
    assert abs(0.5 * (lo["val"] + hi["val"]).item() - whole["val"].item()) <= 1e-15 * whole["Sv"].item()
    # and the averaged gradient of the halves is the whole batch's
    g = 0.5 * torch.cat([lo["grad"], hi["grad"]])
    assert bool(((g - whole["grad"]).abs() <= 1e-14 * whole["M"]).all())


def test_planted_cases():
    B, n, NC = 3, 576, 5
    S, T, y, plants = V.planted(B, n, 36, 36, NC, 1000)
    assert plants == {"absent": 1, "zero": 4, "single": 3, "straddle": (63, 64), "empty": 1}
    assert int((y[0] == 1).sum()) == 0 and int((y[2] == 1).sum()) > 0
    assert int((y[0] == 3).sum()) == 1 and (y[0] == 4).nonzero().flatten().tolist() == list(V.ZERO_ROWS)
    assert bool((S[0, list(V.ZERO_ROWS)] == 0).all()) and not bool(V.kept_mask(y[1], NC).any())
    assert bool((y == -1).any()) and bool((y == NC).any()) and y[0, 63] == y[0, 64] == 0
    d = V.direct(S.double(), T.double(), y, NC)
    assert d["img"][1].item() == 0.0 and bool((d["grad"][1] == 0).all()) and d["img"][0].item() > 0 and d["img"][2].item() > 0
    # the single pixel is its own prototype: s = 1 on both sides, nothing to distil there; the zero class has m = 0: no D_c, no
    # first term, although its similarity difference (0 - sT) enters the value
    assert bool((d["grad"][0, V.SINGLE].abs() <= 1e-15).all()) and bool((d["grad"][0, list(V.ZERO_ROWS)] == 0).all())
    # a kept all-zero row of a class with a live prototype still receives D_c / N_bc
    S2 = S.clone().double()
    i = int((y[2] == 2).nonzero()[0])
    S2[2, i] = 0
    assert V.direct(S2, T.double(), y, NC)["grad"][2, i].abs().max().item() > 0


@pytest.mark.parametrize("B, n, Cs, Ct, NC", SHAPES[1:4])
def test_ifv32_is_close_and_not_exact(B, n, Cs, Ct, NC):
    S, T, y, _ = V.planted(B, n, Cs, Ct, NC, 11)
    d, g = V.direct(S.double(), T.double(), y, NC), V.ifv32(S, T, y, NC)
    ev, eg = abs(g["val"].item() - d["val"].item()), (g["grad"] - d["grad"]).abs()
    print(f"ifv32 ({B}, {n}, {Cs}, {Ct}, {NC}): value error {ev:.3g} ({ev / (V.U * d['Sv'].item()):.3g} u Sv), gradient error {eg.max().item():.3g}")
    # the worst case of an fp32 sum of k terms is k u times the sum of the magnitudes
    k = (n + Cs + Ct + 16) * V.U
    assert 0 < ev <= k * d["Sv"].item()
    assert 0 < eg.max().item() and bool((eg <= k * d["M"].clamp_min(d["M"].max() * 1e-3)).all())


def test_exact_inputs_are_exact():
    B, NC, N = 2, 4, 16
    S, T, y = V.exact_inputs(B, NC, N, 16, 8, 12, 1)
    d, g = V.direct(S.double(), T.double(), y, NC), V.ifv32(S, T, y, NC)
    assert d["val"].item() == 0.5 and torch.equal(d["img"], torch.full((B,), 0.5, dtype=torch.float64))     # N/2 of every N differ by 1
    assert torch.equal(d["grad"].float().double(), d["grad"]) and d["grad"].abs().max().item() > 0
    assert d["val"].item() == g["val"].item() and torch.equal(d["grad"], g["grad"]) and torch.equal(d["img"], g["img"])
    # both parts of the gradient occur: the first term alone on rows of the third quarter, D_c / N_bc alone on the second
    k = V.kept_mask(y, NC)
    assert bool((d["grad"][~k] == 0).all()) and int((d["grad"][k].abs().sum(-1) > 0).sum()) > B * NC * N // 2


def test_slice_mirror():
    assert V.slices(256, 4096) == 4 and V.slices(1024, 4096) == 1 and V.slices(1, 1) == 1 and V.slices(2, 576) == 9
    assert V.slices(1, 64) == 1 and V.slices(1, 65) == 2 and V.slice_rows(2, 576) == 64 and V.slice_rows(256, 4096) == 1024


def test_intra_class_kd_spec():
    spec = IntraClassKD()
    assert spec == IntraClassKD() and dataclasses.fields(IntraClassKD) == () and hash(spec) == hash(IntraClassKD())
    with pytest.raises(Exception):
        spec.tau = 2.0
    with pytest.raises(TypeError):
        IntraClassKD(4.0)
    for word in ("1e-12", "prototype", "re-tune", "N_bc", "ECCV 2020"):
        assert word in IntraClassKD.__doc__, word


def test_refusals_that_need_no_gpu():
    from kdrt import KDError
    from kdrt.kd import KDStep
    from kdrt.losses import ChannelKD, PairKD, kd_objective, kd_objective_backward
    from src.training.trainer import KDTrainer
    a = torch.randn(2, 8, 4, 4, requires_grad=True)
    y = torch.zeros(2, 4, 4, dtype=torch.int64)
    for b in (torch.randn(2, 8, 4, 4), torch.randn(2, 12, 4, 4), torch.randn(2, 8, 4, 5), torch.randn(3, 8, 4, 4), torch.randn(2, 8, 16)):
        with pytest.raises(KDError):
            intra_class_kd(a, b, y, 3)
    for C in (6, 260, 2):
        with pytest.raises(KDError):
            intra_class_kd(torch.randn(2, C, 4, 4), torch.randn(2, 8, 4, 4), y, 3)
    assert a.grad is None
    for bad in ("ifv", 4.0, IntraClassKD, PairKD, ChannelKD):
        with pytest.raises(ValueError):
            KDStep(None, None, None, feature_loss=bad)
        with pytest.raises(ValueError):
            KDTrainer(None, None, None, None, torch.device("cpu"), feature_loss=bad)
        with pytest.raises(KDError):
            kd_objective(a, {}, a, {}, None, feature_loss=bad)
    for make in (lambda: KDStep(None, None, None, feature_loss=IntraClassKD()),
                 lambda: KDTrainer(None, None, None, None, torch.device("cpu"), feature_loss=IntraClassKD())):
        with pytest.raises(Exception) as e:
            make()
        assert "feature_loss" not in str(e.value)
    for fn in (kd_objective, kd_objective_backward, KDTrainer.__init__):
        p = inspect.signature(fn).parameters
        assert "feature_loss" in p and p["feature_loss"].default is None, fn
    assert list(inspect.signature(intra_class_kd).parameters) == ["student_feat", "teacher_feat", "target", "num_classes", "ignore_index"]
    assert inspect.signature(intra_class_kd).parameters["ignore_index"].default == -1


def test_ablation_script_reads_the_new_name_and_keeps_the_old():
    from kdrt.losses import ChannelKD, PairKD
    import train_with_fusion_ablation as S
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "ifv"}) == IntraClassKD()
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "ifv", "KD_CWD_TAU": "2"}) == IntraClassKD()
    assert S.feature_loss_from_env({}) is None and S.feature_loss_from_env({"KD_FEATURE_LOSS": "mse"}) is None
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "1.5"}) == ChannelKD(tau=1.5)
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "pair"}) == PairKD()
    for bad in ({"KD_FEATURE_LOSS": "kl"}, {"KD_FEATURE_LOSS": "PAIR"}, {"KD_FEATURE_LOSS": "pairwise"}, {"KD_FEATURE_LOSS": "IFV"},
                {"KD_FEATURE_LOSS": "ifvd"}, {"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "0"}):
        with pytest.raises(ValueError):
            S.feature_loss_from_env(bad)
    assert S.hard_loss_from_env({"KD_FEATURE_LOSS": "ifv"}) is None
    assert "`ifv`" in S.__doc__ and "IntraClassKD" in S.__doc__


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_feat_ifv_fwd_bwd", "kd_feat_ifv_ws_bytes", "kd_feat_ifv_slices"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    V_, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert protos["kd_feat_ifv_ws_bytes"] == (Z, [I, I, I, I, I])
    assert protos["kd_feat_ifv_slices"] == (I, [I, I])
    assert protos["kd_feat_ifv_fwd_bwd"] == (I, [V_, V_, V_, I, I, I, I, I, I, F, V_, V_, V_, V_, V_, Z, V_])


def test_slices_workspace_query_and_refusals_before_any_launch():
    from kdrt.lib import lib
    q, ns = lib.kd_feat_ifv_ws_bytes, lib.kd_feat_ifv_slices
    for B, HW in ((256, 4096), (1024, 4096), (4, 4096), (2, 576), (1, 1), (1, 64), (1, 65), (255, 4096), (3, 153), (1, 1 << 30)):
        assert ns(B, HW) == V.slices(B, HW) >= 1, (B, HW)
    assert ns(0, 8) == 0 and ns(8, 0) == 0 and ns(1, (1 << 30) + 1) == 0
    for B, HW, Cs, Ct, NC in ((1, 1, 4, 4, 2), (2, 576, 128, 64, 16), (2, 153, 132, 256, 9), (256, 4096, 128, 128, 2)):
        assert q(B, HW, Cs, Ct, NC) > 16 * B * HW and q(B, HW, Cs, Ct, NC) % 16 == 0
    for bad in ((1, 8, 6, 8, 2), (1, 8, 8, 6, 2), (1, 8, 260, 8, 2), (1, 8, 8, 260, 2), (1, 8, 0, 8, 2), (1, 0, 8, 8, 2), (0, 8, 8, 8, 2),
                (1, 8, 8, 8, 1), (1, 8, 8, 8, 17), (1, 8, 8, 8, 0)):
        assert q(*bad) == 0, bad
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch
    enough = q(1, 8, 8, 8, 2)

    def rc(s=one, t=one, y=one, B=1, HW=8, Cs=8, Ct=8, NC=2, gcoef=1.0, val=one, ds=one, ws=one, ws_bytes=enough):
        return lib.kd_feat_ifv_fwd_bwd(s, t, y, -1, B, HW, Cs, Ct, NC, gcoef, None, val, ds, None, ws, ws_bytes, None)
    for kw in (dict(gcoef=float("nan")), dict(gcoef=float("inf")), dict(s=None), dict(t=None), dict(y=None), dict(val=None), dict(ws=None)):
        assert rc(**kw) == -1, kw                                   # KD_ERR_ARG
        assert b"kd_feat_ifv_fwd_bwd" in lib.kd_last_error_string()
    for kw in (dict(Cs=6), dict(Ct=6), dict(Cs=260), dict(Ct=260), dict(Cs=0), dict(NC=1), dict(NC=17), dict(HW=0), dict(HW=(1 << 30) + 1),
               dict(B=0), dict(B=-1)):
        assert rc(**kw) == -4, kw                                   # KD_ERR_SHAPE
        assert b"kd_feat_ifv_fwd_bwd" in lib.kd_last_error_string()
    assert rc(ws_bytes=enough - 1) == -3                            # KD_ERR_WORKSPACE
    assert rc(NC=16, ws_bytes=enough) == -3                         # the workspace of fewer classes
    for kw in (dict(s=ctypes.c_void_p(20)), dict(t=ctypes.c_void_p(24)), dict(ds=ctypes.c_void_p(28)), dict(ws=ctypes.c_void_p(8)),
               dict(y=ctypes.c_void_p(20))):
        assert rc(**kw) == -2, kw                                   # KD_ERR_ALIGN
        assert b"kd_feat_ifv_fwd_bwd" in lib.kd_last_error_string()
