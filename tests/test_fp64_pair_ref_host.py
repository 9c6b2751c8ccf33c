"""CPU tests of the pair-wise distillation term's float64 reference (tests/_fp64_pair_ref.py) and of its host side: the direct n x n
form against the Gram form in float64 and against central differences, the zero-row rule, the float32 Gram yardstick, PairKD and
the ablation script's knob, the feature_loss type checks of every layer, the refusals that need no GPU, and the C ABI of the
three entry points (declared, exported, the slice count, every refusal before a launch)."""
import ctypes
import dataclasses
import inspect
import re

import pytest
import torch

import _fp64_pair_ref as V
from kdrt.losses import PairKD, pair_kd                 # ImportError without the feature


@pytest.mark.parametrize("B, n, Cs, Ct", [(1, 1, 4, 4), (2, 64, 8, 8), (3, 576, 36, 36), (2, 153, 132, 256), (1, 4096, 128, 128)])
def test_direct_against_the_gram_form_in_float64(B, n, Cs, Ct):
    S, T = V.relu_maps(B, n, Cs, Ct, 3)
    d, g = V.direct(S.double(), T.double()), V.gram(S.double(), T.double())
    assert abs(d["val"].item() - g["val"].item()) <= 1e-13 * d["Sv"].item()
    assert bool(((d["img"] - g["img"]).abs() <= 1e-13 * d["Sv_img"]).all())
    assert bool(((d["grad"] - g["grad"]).abs() <= 1e-12 * d["M"]).all())
    assert d["val"].item() >= 0 and (n == 1 or d["val"].item() > 0)


def test_direct_gradient_against_central_differences():
    S, T = V.relu_maps(2, 6, 4, 8, 5)
    S, T = S.double() + 0.05, T.double()
    S[:, 2] = 0                                                      # the zero row: no gradient, and none is probed
    g = V.direct(S, T)["grad"]
    h = 1e-6
    for b, i, c in ((0, 0, 0), (0, 3, 2), (1, 5, 3), (1, 1, 1)):
        Sp, Sm = S.clone(), S.clone()
        Sp[b, i, c] += h
        Sm[b, i, c] -= h
        fd = (V.direct(Sp, T)["val"] - V.direct(Sm, T)["val"]) / (2 * h)
        assert abs(fd.item() - g[b, i, c].item()) <= 1e-9 + 1e-6 * abs(g[b, i, c].item()), (b, i, c, fd.item(), g[b, i, c].item())
    assert bool((g[:, 2] == 0).all())


def test_the_zero_row_rule():
    S, T = V.relu_maps(2, 12, 8, 8, 7)
    S, T = S.double(), T.double()
    Sh, r, live = V.normalise(S)
    assert bool((Sh[:, 4] == 0).all()) and not bool(live[:, 4].any()) and bool(live[:, 5].all())
    assert bool(((Sh[:, 5].pow(2).sum(-1) - 1).abs() < 1e-15).all())
    S[0, 7] = 1e-13 / 8 ** 0.5                                       # a norm at 1e-13: below the threshold, zeroed too
    d = V.direct(S, T)
    assert bool(torch.isfinite(d["grad"]).all()) and bool((d["grad"][:, 4] == 0).all()) and bool((d["grad"][0, 7] == 0).all())
    assert bool((d["M"][:, 4] == 0).all())
    # a zeroed student row still counts in the value: its affinities are 0 where the teacher's are not
    T2 = T.clone()
    T2[:, 4] = 0
    assert V.direct(S, T2)["val"].item() != d["val"].item()
    # identical maps: nothing to distil
    z = V.direct(S, S.clone())
    assert z["val"].item() == 0.0 and bool((z["grad"] == 0).all())


@pytest.mark.parametrize("B, n, Cs, Ct", [(2, 64, 8, 8), (3, 576, 36, 36), (2, 576, 128, 64)])
def test_gram32_is_close_and_not_exact(B, n, Cs, Ct):
    S, T = V.relu_maps(B, n, Cs, Ct, 11)
    d, g = V.direct(S.double(), T.double()), V.gram32(S, T)
    ev, eg = abs(g["val"].item() - d["val"].item()), (g["grad"] - d["grad"]).abs().max().item()
    print(f"gram32 ({B}, {n}, {Cs}, {Ct}): value error {ev:.3g} ({ev / (V.U * d['Sv'].item()):.3g} u Sv), gradient error {eg:.3g} "
          f"({eg / d['grad'].abs().max().item():.3g} of the largest entry)")
    # the worst case of an fp32 sum of n terms is n u times the sum of the magnitudes; the norm, the projection and the division add a few u
    k = (n + Cs + Ct + 8) * V.U
    assert 0 < ev <= k * d["Sv"].item()
    assert 0 < eg and bool(((g["grad"] - d["grad"]).abs() <= k * d["M"].clamp_min(d["M"].max() * 1e-3)).all())


def test_exact_maps_are_exact():
    X = V.exact_maps(2, 64, 8, 1)
    Xh, r, live = V.normalise(X.double())
    assert bool(live.all()) and bool((torch.log2(r) == torch.log2(r).round()).all())
    assert set(Xh.abs().unique().tolist()) == {0.0, 0.5, 1.0} and bool((X < 0).any()) and bool((X > 0).any())
    d = V.direct(X.double(), V.exact_maps(2, 64, 8, 2).double())
    g = V.gram32(X, V.exact_maps(2, 64, 8, 2))
    assert d["val"].item() == g["val"].item() and torch.equal(d["grad"], g["grad"]) and torch.equal(d["img"], g["img"])
    assert torch.equal(d["grad"].float().double(), d["grad"])


def test_slice_mirror():
    assert V.slices(256, 4096) == 1 and V.slices(1000, 4096) == 1 and V.slices(1, 1) == 1 and V.slices(4, 4096) == 64
    assert V.slices(2, 576) == 9 and V.slices(1, 64) == 1 and V.slices(1, 65) == 2 and V.slices(255, 4096) == 2


def test_pair_kd_spec():
    spec = PairKD()
    assert spec == PairKD() and dataclasses.fields(PairKD) == () and hash(spec) == hash(PairKD())
    with pytest.raises(Exception):
        spec.tau = 2.0
    with pytest.raises(TypeError):
        PairKD(4.0)
    for word in ("1e-12", "Gss", "re-tune", "n^2"):
        assert word in PairKD.__doc__, word


def test_refusals_that_need_no_gpu():
    from kdrt import KDError
    from kdrt.kd import KDStep
    from kdrt.losses import ChannelKD, kd_objective, kd_objective_backward
    from src.training.trainer import KDTrainer
    a = torch.randn(2, 8, 4, 4, requires_grad=True)
    for b in (torch.randn(2, 8, 4, 4), torch.randn(2, 12, 4, 4),           # CPU tensors, equal and unequal widths
              torch.randn(2, 8, 4, 5), torch.randn(3, 8, 4, 4), torch.randn(2, 8, 16)):
        with pytest.raises(KDError):
            pair_kd(a, b)
    for C in (6, 260, 2):
        with pytest.raises(KDError):
            pair_kd(torch.randn(1, C, 2, 2), torch.randn(1, 8, 2, 2))
        with pytest.raises(KDError):
            pair_kd(torch.randn(1, 8, 2, 2), torch.randn(1, C, 2, 2))
    with pytest.raises(KDError):
        pair_kd(a.double(), torch.randn(2, 8, 4, 4).double())
    assert a.grad is None
    # every layer takes a PairKD where it takes a ChannelKD, and refuses what it refused before with what it raised before
    for bad in ("pair", "cwd", 4.0, PairKD, ChannelKD):
        with pytest.raises(ValueError):
            KDStep(None, None, None, feature_loss=bad)
        with pytest.raises(ValueError):
            KDTrainer(None, None, None, None, torch.device("cpu"), feature_loss=bad)
        with pytest.raises(KDError):
            kd_objective(a, {}, a, {}, None, feature_loss=bad)
    # a PairKD passes the type checks: what fails next is the missing model, not the option
    for make in (lambda: KDStep(None, None, None, feature_loss=PairKD()),
                 lambda: KDTrainer(None, None, None, None, torch.device("cpu"), feature_loss=PairKD())):
        with pytest.raises(Exception) as e:
            make()
        assert "feature_loss" not in str(e.value)
    for fn in (kd_objective, kd_objective_backward, KDTrainer.__init__):
        p = inspect.signature(fn).parameters
        assert "feature_loss" in p and p["feature_loss"].default is None, fn


def test_ablation_script_reads_the_new_name_and_keeps_the_old():
    from kdrt.losses import ChannelKD
    import train_with_fusion_ablation as S
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "pair"}) == PairKD()
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "pair", "KD_CWD_TAU": "2"}) == PairKD()
    assert S.feature_loss_from_env({}) is None and S.feature_loss_from_env({"KD_FEATURE_LOSS": "mse"}) is None
    assert S.feature_loss_from_env({"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "1.5"}) == ChannelKD(tau=1.5)
    for bad in ({"KD_FEATURE_LOSS": "kl"}, {"KD_FEATURE_LOSS": "PAIR"}, {"KD_FEATURE_LOSS": "pairwise"}, {"KD_FEATURE_LOSS": "cwd", "KD_CWD_TAU": "0"}):
        with pytest.raises(ValueError):
            S.feature_loss_from_env(bad)
    assert S.hard_loss_from_env({"KD_FEATURE_LOSS": "pair"}) is None
    assert "`pair`" in S.__doc__ and "PairKD" in S.__doc__


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_feat_pair_fwd_bwd", "kd_feat_pair_ws_bytes", "kd_feat_pair_slices"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    V_, I, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    assert protos["kd_feat_pair_ws_bytes"] == (Z, [I, I, I, I])
    assert protos["kd_feat_pair_slices"] == (I, [I, I])
    assert protos["kd_feat_pair_fwd_bwd"] == (I, [V_, V_, I, I, I, I, F, V_, V_, V_, V_, V_, Z, V_])


def test_slices_workspace_query_and_refusals_before_any_launch():
    from kdrt.lib import lib
    q, ns = lib.kd_feat_pair_ws_bytes, lib.kd_feat_pair_slices
    for B, HW in ((256, 4096), (1000, 4096), (4, 4096), (2, 576), (1, 1), (1, 64), (1, 65), (255, 4096), (3, 153), (1, 1 << 30)):
        assert ns(B, HW) == V.slices(B, HW) >= 1, (B, HW)
    assert ns(256, 4096) == 1 and ns(4, 4096) > 1 and ns(0, 8) == 0 and ns(8, 0) == 0 and ns(1, (1 << 30) + 1) == 0
    for B, HW, Cs, Ct in ((1, 1, 4, 4), (2, 576, 128, 64), (2, 153, 132, 256), (256, 4096, 128, 128), (4, 4096, 128, 128)):
        assert q(B, HW, Cs, Ct) > 2 * 4 * B * HW and q(B, HW, Cs, Ct) % 16 == 0
    assert q(4, 4096, 128, 128) >= 4 * 64 * 48 * 4096 > q(256, 4096, 128, 128) // 64 * 4    # 64 slices of 48 tiles of 4 KiB per image
    for bad in ((1, 8, 6, 8), (1, 8, 8, 6), (1, 8, 260, 8), (1, 8, 8, 260), (1, 8, 0, 8), (1, 0, 8, 8), (0, 8, 8, 8), (-1, 8, 8, 8)):
        assert q(*bad) == 0, bad
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch
    enough = q(1, 8, 8, 8)

    def rc(s=one, t=one, B=1, HW=8, Cs=8, Ct=8, gcoef=1.0, val=one, ds=one, ws=one, ws_bytes=enough):
        return lib.kd_feat_pair_fwd_bwd(s, t, B, HW, Cs, Ct, gcoef, None, val, ds, None, ws, ws_bytes, None)
    for kw in (dict(gcoef=float("nan")), dict(gcoef=float("inf")), dict(gcoef=-float("inf")), dict(s=None), dict(t=None), dict(val=None),
               dict(ws=None)):
        assert rc(**kw) == -1, kw                                   # KD_ERR_ARG
        assert b"kd_feat_pair_fwd_bwd" in lib.kd_last_error_string()
    for kw in (dict(Cs=6), dict(Ct=6), dict(Cs=260), dict(Ct=260), dict(Cs=0), dict(Ct=2), dict(HW=0), dict(HW=(1 << 30) + 1), dict(B=0), dict(B=-1)):
        assert rc(**kw) == -4, kw                                   # KD_ERR_SHAPE
        assert b"kd_feat_pair_fwd_bwd" in lib.kd_last_error_string()
    assert rc(ws_bytes=enough - 1) == -3                            # KD_ERR_WORKSPACE
    assert rc(Ct=256, ws_bytes=enough) == -3                        # the workspace of a narrower teacher
    for kw in (dict(s=ctypes.c_void_p(20)), dict(t=ctypes.c_void_p(24)), dict(ds=ctypes.c_void_p(28)), dict(ws=ctypes.c_void_p(8))):
        assert rc(**kw) == -2, kw                                   # KD_ERR_ALIGN: a float4 access there would fault
        assert b"kd_feat_pair_fwd_bwd" in lib.kd_last_error_string()
