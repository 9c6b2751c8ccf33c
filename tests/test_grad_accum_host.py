"""CPU tests of the host side of gradient accumulation: the C ABI of kd_grad_accumulate (declared, exported, arguments refused before
a launch), `accum_steps` on FusedAdamW / AccumCycle / KDStep / Trainer, the KD_ACCUM_STEPS switch and the reducer's bookkeeping
(hooks silent on the first k-1 micro-batches, one fold per bucket on the last, before the world-size early return).  Nothing here
launches a kernel."""
import ctypes
import inspect
import re

import pytest
import torch

from kdrt.optim import AccumCycle, FusedAdamW           # ImportError without the feature

KD_ERR_ARG, KD_ERR_ALIGN = -1, -2


def _small():
    torch.manual_seed(1)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3, bias=False), torch.nn.Linear(3, 2))


def test_header_declares_and_library_exports_the_entry_point():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    name = "kd_grad_accumulate"
    assert re.search(r"\b%s\s*\(" % name, text) and name in protos
    assert hasattr(ctypes.CDLL(SO_PATH), name)
    V, I = ctypes.c_void_p, ctypes.c_int
    assert protos[name] == (I, [V, V, ctypes.c_int64, I, V])


def test_argument_errors_before_any_launch():
    from kdrt.lib import lib
    a, g = ctypes.c_void_p(16), ctypes.c_void_p(48)      # never dereferenced: every call below returns before a launch
    for fold in (0, 1):
        for args in ((a, a, 4), (None, g, 4), (a, None, 4), (None, None, 1), (a, g, -1), (a, g, -4)):
            assert lib.kd_grad_accumulate(*args, fold, None) == KD_ERR_ARG, (args, fold)
            assert b"kd_grad_accumulate" in lib.kd_last_error_string()
        for args in ((ctypes.c_void_p(20), g, 4), (a, ctypes.c_void_p(56), 4), (ctypes.c_void_p(17), ctypes.c_void_p(49), 1)):
            assert lib.kd_grad_accumulate(*args, fold, None) == KD_ERR_ALIGN, (args, fold)
            assert b"aligned" in lib.kd_last_error_string()
        for args in ((a, g, 0), (None, None, 0), (a, a, 0)):  # nothing to do: OK without a launch
            assert lib.kd_grad_accumulate(*args, fold, None) == 0, (args, fold)
    assert lib.kd_grad_accumulate(a, g, 4, 2, None) == KD_ERR_ARG


def test_accum_steps_validation_and_the_buffer():
    for bad in (0, -1, 2.0, "2", None, True, 1.5):
        with pytest.raises(ValueError, match="accum_steps"):
            FusedAdamW(_small().parameters(), accum_steps=bad)
    q = inspect.signature(FusedAdamW.__init__).parameters
    assert q["accum_steps"].default == 1 and list(q)[-1] == "accum_steps"
    off = FusedAdamW(_small().parameters(), lr=1e-3)
    assert off.accum_steps == 1 and off.flat.accum is None
    for call in (off.accumulate, off.fold, lambda: off.fold(0, 4)):
        with pytest.raises(RuntimeError, match="accum_steps"):
            call()
    for k in (2, 5):
        on = FusedAdamW(_small().parameters(), lr=1e-3, accum_steps=k, max_grad_norm=1.0, ema_decay=0.9)
        acc = on.flat.accum
        assert on.accum_steps == k and acc.shape == on.flat.grad.shape and acc.dtype == torch.float32 and acc.device == on.flat.grad.device
        assert acc.data_ptr() != on.flat.grad.data_ptr() and float(acc.abs().max()) == 0.0
        assert "accum" not in str(sorted(on.state_dict()["param_groups"][0])) and set(on.state_dict()) == {"state", "param_groups"}
    with pytest.raises(ValueError, match="slice"):
        on.fold(8, 4)
    with pytest.raises(ValueError, match="slice"):
        on.fold(0, on.flat.numel + 4)


def test_cycle_takes_the_optimisers_value_and_refuses_another():
    opt1, opt3 = FusedAdamW(_small().parameters()), FusedAdamW(_small().parameters(), accum_steps=3)
    assert AccumCycle(opt1).k == 1 and AccumCycle(opt1, None, 1).k == 1 and AccumCycle(opt3).k == 3 and AccumCycle(opt3, None, 3).k == 3
    for opt, k in ((opt1, 3), (opt3, 1), (opt3, 2)):
        with pytest.raises(ValueError, match="disagrees"):
            AccumCycle(opt, None, k)
    for bad in (0, -2, 1.0, "3"):
        with pytest.raises(ValueError, match="accum_steps"):
            AccumCycle(opt3, None, bad)
    c = AccumCycle(opt3)
    assert [c.begin(), c.pending] == [False, 0] and c.flush() is False        # nothing pending: flush does nothing


def _kd_pair(k_opt):
    from _gpu_util import build_product
    torch.manual_seed(0)
    student, teacher = build_product("weighted", 16, device="cpu"), build_product("concat", 16, device="cpu")
    kw = {} if k_opt == 1 else {"accum_steps": k_opt}
    return student, teacher, FusedAdamW(student.parameters(), lr=1e-3, **kw)


def test_kd_step_keyword():
    from kdrt.kd import KDStep
    s, t, opt = _kd_pair(1)
    assert KDStep(s, t, opt).cycle.k == 1
    s, t, opt = _kd_pair(1)
    assert KDStep(s, t, opt, accum_steps=1).cycle.k == 1
    s, t, opt = _kd_pair(3)
    step = KDStep(s, t, opt)                                                  # None: the optimiser's value
    assert step.cycle.k == 3 and step.cycle.opt is opt and step.flush() is False
    s, t, opt = _kd_pair(3)
    assert KDStep(s, t, opt, None, 4.0, 1.0, 1.0, -1, None, "fp32", True, None, accum_steps=3).cycle.k == 3
    for k_opt, k_step in ((1, 2), (3, 1), (3, 4)):
        s, t, opt = _kd_pair(k_opt)
        with pytest.raises(ValueError, match="disagrees"):
            KDStep(s, t, opt, accum_steps=k_step)
    s, t, opt = _kd_pair(3)
    with pytest.raises(ValueError, match="accum_steps"):
        KDStep(s, t, opt, accum_steps=0)
    with pytest.raises(TypeError):
        KDStep(s, t, opt, accum_stepz=3)


def test_trainer_keyword_and_environment_switch(tmp_path):
    from _gpu_util import build_product
    from src.training.trainer import KDTrainer, Trainer, optim_options_from_env
    p = inspect.signature(Trainer.__init__).parameters
    assert p["accum_steps"].default == 1 and "kw" in inspect.signature(KDTrainer.__init__).parameters
    assert optim_options_from_env({}) == {} and optim_options_from_env({"KD_ACCUM_STEPS": ""}) == {}
    assert optim_options_from_env({"KD_ACCUM_STEPS": "4"}) == {"accum_steps": 4}
    assert optim_options_from_env({"KD_ACCUM_STEPS": "1", "KD_NO_DECAY_NORM_BIAS": "1"}) == {"accum_steps": 1, "no_decay_norm_bias": True}
    for bad in ("0", "-2", "2.5", "two", "1e1"):
        with pytest.raises(ValueError, match="KD_ACCUM_STEPS|accum_steps"):
            optim_options_from_env({"KD_ACCUM_STEPS": bad})
    dev = torch.device("cpu")
    tr = Trainer(build_product("weighted", 16, device="cpu"), [], [], dev, save_dir=str(tmp_path / "a"), accum_steps=3)
    assert tr.accum_steps == 3 and tr.optimizer.accum_steps == 3 and tr.cycle.k == 3 and tr.optimizer.flat.accum is not None
    assert tr.flush() is False
    tr1 = Trainer(build_product("weighted", 16, device="cpu"), [], [], dev, save_dir=str(tmp_path / "b"))
    assert tr1.accum_steps == 1 and tr1.optimizer.flat.accum is None and tr1.cycle.k == 1
    kt = KDTrainer(build_product("weighted", 16, device="cpu"), build_product("concat", 16, device="cpu"), [], [], dev,
                   save_dir=str(tmp_path / "c"), accum_steps=2)
    assert kt.cycle is kt.kd_step.cycle and kt.cycle.k == 2
    for bad in (0, 2.0):
        with pytest.raises(ValueError, match="accum_steps"):
            Trainer(build_product("weighted", 16, device="cpu"), [], [], dev, save_dir=str(tmp_path / "d"), accum_steps=bad)
    import train_pandaset
    import train_with_fusion_ablation
    for mod in (train_pandaset, train_with_fusion_ablation):
        assert "KD_ACCUM_STEPS" in mod.__doc__


def test_reducer_folds_each_bucket_once_on_the_last_micro_batch_only():
    """world of one rank, not forced: no collective, and the fold still runs (before the early return), per bucket slice"""
    from kdrt.ddp import BucketedAllReduce
    net = _small()
    opt = FusedAdamW(net.parameters(), lr=1e-3, accum_steps=2)
    names = [n for n, _ in net.named_parameters()]
    red = BucketedAllReduce(opt.flat, names, n_buckets=3)
    assert red.fold is None and "fold" in inspect.signature(BucketedAllReduce.__init__).parameters
    cyc = AccumCycle(opt, red)
    assert red.fold == opt.fold
    folds = []
    red.fold = lambda lo, hi: folds.append((lo, hi))
    slices = [(opt.flat.offsets[a], opt.flat.offsets[e]) for a, e in red.spans]
    assert len(slices) == 3 and slices[0][0] == 0 and slices[-1][1] == opt.flat.numel and all(lo % 4 == 0 for lo, _ in slices)
    # micro-batch 1: the owner silences the hooks
    assert cyc.begin() is False and red.enabled is False
    for q in reversed(opt.flat.params):
        red.notify(q)
    assert folds == [] and red.launch_order == [] and red.collectives_issued == 0 and red.pending == [e - a for a, e in red.spans]
    # micro-batch 2: every bucket the moment its last gradient lands, backward order; finish() adds nothing
    cyc.pending = 1
    assert cyc.begin() is True and red.enabled is True
    for q in reversed(opt.flat.params):
        red.notify(q)
    assert red.launch_order == [2, 1, 0] and folds == slices[::-1]
    assert red.finish() == 1.0 and folds == slices[::-1] and red.collectives_issued == 0
    # buckets whose hooks did not all fire go through the same path from finish()
    del folds[:]
    red.notify(opt.flat.params[-1])
    assert red.finish() == 1.0 and sorted(folds) == slices and len(folds) == 3


def test_gradsink_no_longer_rules_accumulation_out():
    from kdrt import gradsink
    src = inspect.getsource(gradsink)
    assert "accumulation is not supported" not in src and "accum_steps" in src and "micro-batch" in gradsink.__doc__
