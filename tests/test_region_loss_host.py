"""CPU tests of the host side of the opt-in focal + Tversky hard-label loss: parameter validation before anything touches the
device, the "no CPU fallback" refusal, the `hard_loss=` keyword on the training entry points, and the C ABI of the two new
entry points (declared in include/kd_hip.h, exported by the built library, arguments refused with KD_ERR_ARG)."""
import ctypes
import inspect
import re

import pytest
import torch

from kdrt.losses import RegionLoss, region_seg_loss          # ImportError without the feature


def test_region_loss_defaults_and_frozen():
    spec = RegionLoss()
    assert (spec.gamma, spec.wf, spec.wt, spec.a, spec.b, spec.s) == (2.0, 1.0, 1.0, 0.7, 0.3, 1.0)
    assert spec.args() == (2.0, 1.0, 1.0, 0.7, 0.3, 1.0)
    with pytest.raises(Exception):
        spec.gamma = 1.0
    for ok in (dict(gamma=0), dict(gamma=1), dict(gamma=3.5), dict(wf=0), dict(wt=0), dict(a=0, b=0), dict(s=1e-6)):
        RegionLoss(**ok)


@pytest.mark.parametrize("bad", [dict(gamma=0.5), dict(gamma=-1.0), dict(gamma=0.999), dict(a=-0.1), dict(b=-1e-9), dict(s=0.0),
                                 dict(s=-1.0), dict(wf=-1.0), dict(wt=-0.5), dict(wf=0.0, wt=0.0), dict(gamma=float("nan")),
                                 dict(s=float("inf")), dict(a="0.7")],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_region_loss_refuses(bad):
    with pytest.raises(ValueError):
        RegionLoss(**bad)


def test_region_seg_loss_refuses_cpu_tensors_and_other_specs():
    from kdrt import KDError
    z, y = torch.randn(2, 2, 4, 4, requires_grad=True), torch.zeros(2, 4, 4, dtype=torch.int64)
    with pytest.raises(KDError):
        region_seg_loss(z, y, RegionLoss())
    sig = inspect.signature(region_seg_loss)
    assert list(sig.parameters) == ["logits", "target", "spec", "class_weights", "ignore_index", "teacher_logits", "T", "alpha"]
    assert [sig.parameters[k].default for k in ("class_weights", "ignore_index", "teacher_logits", "T", "alpha")] == [None, -1, None, 4.0, 1.0]


def test_entry_points_take_hard_loss_and_default_to_none():
    from kdrt.kd import KDStep
    from kdrt.losses import kd_objective, kd_objective_backward
    from src.training.trainer import KDTrainer, Trainer
    for fn in (KDStep.__init__, Trainer.__init__, kd_objective, kd_objective_backward):
        p = inspect.signature(fn).parameters
        assert "hard_loss" in p and p["hard_loss"].default is None, fn
        assert list(p)[-1] == "hard_loss", f"{fn}: the parent commit's positional arguments keep their places"
    assert "kw" in inspect.signature(KDTrainer.__init__).parameters         # hard_loss reaches Trainer through **kw


def test_ablation_script_reads_the_environment_knobs():
    import train_with_fusion_ablation as S
    assert S.hard_loss_from_env({}) is None and S.hard_loss_from_env({"KD_HARD_LOSS": "ce"}) is None
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky"}) == RegionLoss()
    got = S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky", "KD_FOCAL_GAMMA": "1", "KD_TVERSKY_ALPHA": "0.5", "KD_TVERSKY_BETA": "0.5"})
    assert got == RegionLoss(gamma=1.0, a=0.5, b=0.5)
    with pytest.raises(ValueError):
        S.hard_loss_from_env({"KD_HARD_LOSS": "dice"})
    with pytest.raises(ValueError):
        S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky", "KD_FOCAL_GAMMA": "0.5"})


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_seg_region_loss_fwd_bwd", "kd_seg_region_loss_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    res, args = protos["kd_seg_region_loss_fwd_bwd"]
    ce_res, ce_args = protos["kd_seg_loss_fwd_bwd"]
    # kd_seg_loss_fwd_bwd's arguments with gamma, wf, wt, a, b, s after the gradient scale
    assert res is ce_res and args == ce_args[:9] + [ctypes.c_float] * 6 + ce_args[9:]


def test_workspace_query_and_argument_errors():
    from kdrt.lib import lib
    for npix, rows in ((1, 1), (256, 1), (257, 2), (262144, 1024), (262145, 1024), (1 << 24, 1024)):
        assert lib.kd_seg_region_loss_ws_bytes(npix) == rows * 16 * 4
    one = ctypes.c_void_p(16)            # never dereferenced: every call below is refused before a launch

    def rc(gamma=2.0, wf=1.0, wt=1.0, a=0.7, b=0.3, s=1.0, NC=2, ws_bytes=64):
        return lib.kd_seg_region_loss_fwd_bwd(one, None, one, None, -1, 4.0, 1.0, 1.0, None, gamma, wf, wt, a, b, s, one, None, 1, NC, 8,
                                              one, ws_bytes, None)
    for kw in (dict(gamma=0.5), dict(gamma=-2.0), dict(gamma=float("nan")), dict(a=-0.1), dict(b=-0.1), dict(s=0.0), dict(wf=-1.0),
               dict(wt=-1.0), dict(wf=0.0, wt=0.0)):
        assert rc(**kw) == -1, kw                                   # KD_ERR_ARG
        assert b"kd_seg_region_loss_fwd_bwd" in lib.kd_last_error_string()
    assert rc(NC=5) == -4 and rc(NC=1) == -4                        # KD_ERR_SHAPE
    assert rc(ws_bytes=60) == -3                                    # KD_ERR_WORKSPACE
