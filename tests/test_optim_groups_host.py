"""CPU tests of the host side of parameter groups and the EMA weight copy in FusedAdamW: the C ABI of the new entry point
(declared in include/kd_hip.h, exported by the built library, arguments refused before a launch), `decay_groups`, the segment
table, torch.optim.AdamW's state_dict layout for G groups, the EMA helpers' bookkeeping and the keywords of the trainers and
entry scripts.  Nothing here launches a kernel."""
import ctypes
import inspect
import re

import pytest
import torch

import _fp64_optim_groups_ref as G
from kdrt.optim import FusedAdamW, decay_groups          # ImportError without the feature

KD_ERR_ARG, KD_ERR_ALIGN, KD_ERR_WORKSPACE, KD_ERR_SHAPE = -1, -2, -3, -4


def test_header_declares_and_library_exports_the_entry_point():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    name = "kd_adamw_step_groups_dev"
    assert re.search(r"\b%s\s*\(" % name, text) and name in protos
    assert hasattr(dll, name)
    res, args = protos[name]
    V, F, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    assert res is I and args == [V, V, V, V, ctypes.c_int64, V, V, V, V, V, I, V, I, V, V, F, I, V, V, ctypes.c_size_t, F, F, F, F, F, V]
    for old in ("kd_adamw_step", "kd_adamw_step_dev", "kd_adamw_step_clip_dev"):
        assert old in protos and hasattr(dll, old)


def test_argument_errors_before_any_launch():
    from kdrt.lib import lib
    one = ctypes.c_void_p(16)             # never dereferenced: every call below is refused before a launch
    I32 = ctypes.c_int32

    def rc(n=16, ends=(1, 4), grps=(0, 1), G_=2, p=one, ema=None, ema_state=None, decay=0.5, clip=None, ws=None, ws_bytes=0, max_norm=1.0,
           n_seg=None):
        e, g = (I32 * len(ends))(*ends), (I32 * len(grps))(*grps)
        return lib.kd_adamw_step_groups_dev(p, one, one, one, n, one, one, one, ctypes.cast(e, ctypes.c_void_p), ctypes.cast(g, ctypes.c_void_p),
                                            len(ends) if n_seg is None else n_seg, one, G_, ema, ema_state, decay, 0, clip, ws, ws_bytes,
                                            0.9, 0.999, 1e-8, 1.0, max_norm, None)

    for kw in (dict(n=18), dict(n=17), dict(n=0), dict(n=-4), dict(ends=(1, 3)), dict(ends=(1, 5)), dict(ends=(2, 2, 4), grps=(0, 1, 0)),
               dict(ends=(0, 4)), dict(ends=(3, 2, 4), grps=(0, 1, 0)), dict(grps=(0, 2)), dict(grps=(-1, 0)), dict(G_=1), dict(G_=0),
               dict(n_seg=0), dict(ema=one), dict(ema_state=one), dict(ema=one, ema_state=one, decay=1.5), dict(ema=one, ema_state=one, decay=-0.1),
               dict(ema=one, ema_state=one, decay=float("nan")), dict(clip=one), dict(ws=one), dict(clip=one, ws=one, ws_bytes=8, max_norm=0.0),
               dict(clip=one, ws=one, ws_bytes=8, max_norm=float("inf"))):
        assert rc(**kw) == KD_ERR_ARG, kw
        assert b"kd_adamw_step_groups_dev" in lib.kd_last_error_string()
    assert rc(p=ctypes.c_void_p(20)) == KD_ERR_ALIGN
    assert rc(ema=ctypes.c_void_p(24), ema_state=one) == KD_ERR_ALIGN
    assert rc(clip=one, ws=ctypes.c_void_p(12), ws_bytes=8) == KD_ERR_ALIGN
    assert rc(clip=one, ws=one, ws_bytes=0) == KD_ERR_WORKSPACE
    # the table lives in LDS: 4097 segments are refused (4096, the most that are accepted, run in tests/test_gpu_optim_groups.py)
    n4 = 4097
    assert rc(n=4 * n4, ends=tuple(range(1, n4 + 1)), grps=(0, 1) * 2048 + (0,)) == KD_ERR_SHAPE
    assert b"4097 segments" in lib.kd_last_error_string()


def _models():
    from _gpu_util import FUSIONS, build_product
    for fusion in FUSIONS:
        torch.manual_seed(0)
        yield fusion, build_product(fusion, 16, device="cpu")


def test_decay_groups_on_the_published_models():
    import _fp64_loss_ref as R
    counts = []
    for fusion, model in _models():
        groups = decay_groups(model, 1e-3, 1e-2)
        assert len(groups) == 2 and [g["weight_decay"] for g in groups] == [1e-2, 0.0] and all(g["lr"] == 1e-3 for g in groups)
        named = dict(model.named_parameters())
        nd_ids = {id(p) for p in named.values() if p.ndim <= 1}
        assert {id(p) for p in groups[1]["params"]} == nd_ids and nd_ids
        assert {id(p) for p in groups[0]["params"]} == {id(p) for p in named.values()} - nd_ids
        for mod in model.modules():                  # every BatchNorm scale and bias, every bias
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                assert id(mod.weight) in nd_ids and id(mod.bias) in nd_ids
        assert all(id(p) in nd_ids for n, p in named.items() if n.endswith(".bias"))
        counts.append(sum(p.numel() for p in named.values()))
        # a multiplier per top-level module, with and without the no-decay split
        top = [n for n, _ in model.named_children()]
        assert "camera_encoder" in top
        g4 = decay_groups(model, 1e-3, 1e-2, lr_mult={"camera_encoder": 0.1})
        assert len(g4) == 4 and sorted((round(g["lr"], 9), g["weight_decay"]) for g in g4) == [(1e-4, 0.0), (1e-4, 1e-2), (1e-3, 0.0), (1e-3, 1e-2)]
        cam = {id(p) for n, p in named.items() if n.startswith("camera_encoder.")}
        assert {id(p) for g in g4 if round(g["lr"], 9) == 1e-4 for p in g["params"]} == cam
        assert sum(len(g["params"]) for g in g4) == len(named)
        g2 = decay_groups(model, 1e-3, 1e-2, lr_mult={"camera_encoder": 0.1}, no_decay=False)
        assert len(g2) == 2 and all(g["weight_decay"] == 1e-2 for g in g2)
        with pytest.raises(ValueError, match="camera_encodr"):
            decay_groups(model, 1e-3, 1e-2, lr_mult={"camera_encodr": 0.1})
        with pytest.raises(ValueError):
            decay_groups(model, 1e-3, 1e-2, lr_mult={"camera_encoder.stem": 0.1})
    assert sorted(counts) == sorted(R.PARAM_COUNTS)


def _small():
    torch.manual_seed(1)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3, bias=False), torch.nn.Linear(3, 2))


def test_segment_table_and_flat_order():
    net = _small()
    params = list(net.parameters())                  # W0 [7,5], b0 [7], bn.w [7], bn.b [7], W2 [3,7], W3 [2,3], b3 [2]
    groups = decay_groups(net, 1e-3, 1e-2)
    opt = FusedAdamW(groups, lr=1e-3, weight_decay=1e-2, flat_order=net.parameters())
    assert [id(p) for p in opt.flat.params] == [id(p) for p in params]
    group_of = [0 if p.ndim > 1 else 1 for p in params]
    ends, grp = G.segment_table([p.numel() for p in params], group_of)
    assert opt.grouped and opt.seg_end_host.dtype == torch.int32
    assert (opt.seg_end_host.tolist(), opt.seg_group_host.tolist()) == (ends, grp) and grp == [0, 1, 0, 1]
    assert ends[-1] * 4 == opt.flat.numel
    # default order: the concatenation of the groups -> one segment per group
    net2 = _small()
    opt2 = FusedAdamW(decay_groups(net2, 1e-3, 1e-2), lr=1e-3, weight_decay=1e-2)
    assert [p.ndim for p in opt2.flat.params] == [2, 2, 2, 1, 1, 1, 1] and opt2.seg_group_host.tolist() == [0, 1]
    for q, ref in zip(net2.parameters(), _small().parameters()):
        assert torch.equal(q, ref)                   # re-homing keeps the values
    with pytest.raises(ValueError, match="flat_order"):
        FusedAdamW(decay_groups(_small(), 1e-3, 1e-2), flat_order=list(_small().parameters()))
    net3 = _small()
    with pytest.raises(ValueError, match="flat_order"):
        FusedAdamW(decay_groups(net3, 1e-3, 1e-2), flat_order=list(net3.parameters())[:-1])
    # an empty tensor takes no float4 and no segment, wherever it stands (as in G.segment_table)
    for where in (0, 3, 7):
        net4 = _small()
        ps = list(net4.parameters())
        ps.insert(where, torch.nn.Parameter(torch.zeros(0)))
        group_of = [0 if q.ndim > 1 else 1 for q in ps]
        opt4 = FusedAdamW([{"params": [q for q, gi in zip(ps, group_of) if gi == 0]},
                           {"params": [q for q, gi in zip(ps, group_of) if gi == 1], "weight_decay": 0.0}], lr=1e-3, flat_order=ps)
        want = G.segment_table([q.numel() for q in ps], group_of)
        assert (opt4.seg_end_host.tolist(), opt4.seg_group_host.tolist()) == want == (ends, grp), where
    # one group, no EMA: the single-group path with its attributes as before
    opt1 = FusedAdamW(_small().parameters(), lr=1e-3)
    assert not opt1.grouped and opt1.group_state is None and opt1.ema is None and opt1.ema_decay is None
    one_group_list = FusedAdamW([{"params": list(_small().parameters())}], lr=1e-3)
    assert not one_group_list.grouped


def test_per_group_betas_or_eps_raise():
    for bad in (dict(betas=(0.8, 0.999)), dict(eps=1e-6)):
        net = _small()
        groups = decay_groups(net, 1e-3, 1e-2)
        groups[1].update(bad)
        with pytest.raises(ValueError, match="betas"):
            FusedAdamW(groups, lr=1e-3)
    net = _small()
    groups = decay_groups(net, 1e-3, 1e-2)
    groups[1].update(betas=(0.8, 0.99), eps=1e-6)
    groups[0].update(betas=(0.8, 0.99), eps=1e-6)
    FusedAdamW(groups, lr=1e-3, betas=(0.8, 0.99), eps=1e-6)        # the same everywhere: fine
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FusedAdamW(_small().parameters(), ema_decay=bad)


def test_state_dict_has_torch_layout_for_groups():
    net = _small()
    ref = [torch.nn.Parameter(p.detach().clone()) for p in net.parameters()]
    byid = {id(p): r for p, r in zip(net.parameters(), ref)}
    groups = decay_groups(net, 1e-3, 1e-2, lr_mult={"0": 0.5})
    tgroups = [{**g, "params": [byid[id(p)] for p in g["params"]]} for g in groups]
    opt = FusedAdamW(groups, lr=1e-3, weight_decay=1e-2, flat_order=net.parameters(), ema_decay=0.9)
    topt = torch.optim.AdamW(tgroups, lr=1e-3, weight_decay=1e-2)
    for r in ref:
        r.grad = torch.ones_like(r)
    topt.step()
    opt.exp_avg.copy_(torch.arange(opt.flat.numel) * 0.5)           # recognisable moments, as a device step would leave them
    opt.exp_avg_sq.copy_(torch.arange(opt.flat.numel) * 0.25)
    opt.note_steps(2)
    sd, tsd = opt.state_dict(), topt.state_dict()
    assert len(sd["param_groups"]) == len(groups) == 4
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in tsd["param_groups"]]        # indices in group order
    assert sorted(sd["state"]) == sorted(tsd["state"]) == list(range(7))
    for a, b in zip(sd["param_groups"], tsd["param_groups"]):
        assert (a["lr"], a["weight_decay"], tuple(a["betas"]), a["eps"]) == (b["lr"], b["weight_decay"], tuple(b["betas"]), b["eps"])
        assert "ema_decay" not in a and "max_grad_norm" not in a
    for i in sd["state"]:
        assert set(sd["state"][i]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][i]["exp_avg"].shape == tsd["state"][i]["exp_avg"].shape
    # FusedAdamW -> torch.optim.AdamW and back: index i of the state is the i-th parameter in GROUP order
    topt.load_state_dict(sd)
    order = [p for g in groups for p in g["params"]]
    for i, p in enumerate(order):
        st = topt.state[byid[id(p)]]
        assert float(st["step"]) == 2.0 and torch.equal(st["exp_avg"], opt.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], opt.state[p]["exp_avg_sq"])
    net_b = _small()
    opt_b = FusedAdamW(decay_groups(net_b, 1e-3, 1e-2, lr_mult={"0": 0.5}), lr=1e-3, weight_decay=1e-2, flat_order=net_b.parameters())
    tsd2 = topt.state_dict()
    tsd2["param_groups"][0]["lr"] = 7e-4
    opt_b.load_state_dict(tsd2)
    for pb, pa in zip(net_b.parameters(), net.parameters()):          # (per tensor: the padding between tensors is not state)
        assert torch.equal(opt_b.state[pb]["exp_avg"], opt.state[pa]["exp_avg"]) and torch.equal(opt_b.state[pb]["exp_avg_sq"], opt.state[pa]["exp_avg_sq"])
        assert opt_b.state[pb]["exp_avg"].data_ptr() - opt_b.exp_avg.data_ptr() == opt.state[pa]["exp_avg"].data_ptr() - opt.exp_avg.data_ptr()
    assert opt_b._step == 2
    assert opt_b.param_groups[0]["lr"] == 7e-4 and opt_b._dev_groups is None
    # the single-group layout is unchanged
    sd1 = FusedAdamW(_small().parameters(), lr=1e-3).state_dict()
    assert len(sd1["param_groups"]) == 1 and sd1["param_groups"][0]["params"] == list(range(7))


def test_ema_helpers_on_the_host():
    net = _small()
    opt = FusedAdamW(net.parameters(), lr=1e-3, ema_decay=0.9, ema_warmup=True)
    assert opt.grouped and opt.ema_warmup and torch.equal(opt.ema, opt.flat.data) and opt.ema.data_ptr() != opt.flat.data.data_ptr()
    assert opt.seg_end_host.tolist() == [opt.flat.numel // 4] and opt.seg_group_host.tolist() == [0]
    live = opt.flat.data.clone()
    pat = torch.zeros(opt.flat.numel)                # recognisable values; the padding between tensors stays 0, as on the device
    for q, o in zip(opt.flat.params, opt.flat.offsets):
        pat[o:o + q.numel()] = torch.arange(o, o + q.numel()) * 1.0
    opt.ema.copy_(pat)
    net[1].running_mean.fill_(3.0)
    sd = opt.ema_state_dict(net)
    assert list(sd) == list(net.state_dict())
    assert torch.equal(sd["0.weight"].reshape(-1), torch.arange(35.0)) and torch.equal(sd["0.bias"], torch.arange(36.0, 43.0))
    assert torch.equal(sd["1.running_mean"], torch.full((7,), 3.0)) and sd["1.running_mean"].data_ptr() != net[1].running_mean.data_ptr()
    assert sd["0.weight"].data_ptr() != opt.ema.data_ptr()                       # copies, not views
    fresh = _small()
    fresh.load_state_dict(sd)
    assert torch.equal(fresh[3].bias, sd["3.bias"])
    e0, ep = opt.ema.clone(), opt.epoch
    with opt.swap_ema():
        assert opt.epoch == ep + 1 and torch.equal(opt.flat.data, e0) and torch.equal(net[0].weight.reshape(-1), torch.arange(35.0))
    assert opt.epoch == ep + 2 and torch.equal(opt.flat.data.view(torch.int32), live.view(torch.int32))
    with pytest.raises(RuntimeError):
        with opt.swap_ema():
            raise RuntimeError("inside")
    assert torch.equal(opt.flat.data, live)                                        # restored on an exception too
    opt.reset_ema()
    assert torch.equal(opt.ema, live)
    opt.load_ema(sd, net)
    assert torch.equal(opt.ema, e0)
    with pytest.raises(RuntimeError, match="model"):
        opt.load_ema(sd)                             # a mapping needs the model its names belong to, every time
    opt.reset_ema()
    opt.load_ema(e0)
    assert torch.equal(opt.ema, e0)
    with pytest.raises(KeyError):
        opt.load_ema({k: v for k, v in sd.items() if k != "3.bias"}, net)
    off = FusedAdamW(_small().parameters(), lr=1e-3)
    for call in (lambda: off.ema_state_dict(net), lambda: off.load_ema(sd, net), off.reset_ema, lambda: off.swap_ema().__enter__()):
        with pytest.raises(RuntimeError, match="ema_decay"):
            call()
    with pytest.raises(RuntimeError, match="model"):
        FusedAdamW(_small().parameters(), ema_decay=0.5).load_ema(sd)


def test_trainer_keywords_and_environment_switches():
    from src.training.trainer import KDTrainer, Trainer, optim_options_from_env
    p = inspect.signature(Trainer.__init__).parameters
    assert list(p)[-5:-1] == ["ema_decay", "ema_warmup", "no_decay_norm_bias", "lr_mult"] and list(p)[-6] == "max_grad_norm"
    assert [p[k].default for k in list(p)[-5:-1]] == [None, False, False, None]
    assert "kw" in inspect.signature(KDTrainer.__init__).parameters
    q = inspect.signature(FusedAdamW.__init__).parameters
    assert list(q)[:7] == ["self", "params", "lr", "betas", "eps", "weight_decay", "max_grad_norm"]
    assert [q[k].default for k in ("flat_order", "ema_decay", "ema_warmup")] == [None, None, False]
    assert optim_options_from_env({}) == {}
    assert optim_options_from_env({"KD_EMA_DECAY": "0.999"}) == {"ema_decay": 0.999, "ema_warmup": False}
    assert optim_options_from_env({"KD_EMA_DECAY": "0.99", "KD_EMA_WARMUP": "1", "KD_NO_DECAY_NORM_BIAS": "1",
                                   "KD_LR_MULT": "camera_encoder=0.1, lidar_encoder=0.5"}) == {
        "ema_decay": 0.99, "ema_warmup": True, "no_decay_norm_bias": True, "lr_mult": {"camera_encoder": 0.1, "lidar_encoder": 0.5}}
    for bad in ({"KD_EMA_WARMUP": "1"}, {"KD_LR_MULT": "camera_encoder"}, {"KD_LR_MULT": "=0.1"}, {"KD_LR_MULT": "a=b"}):
        with pytest.raises(ValueError):
            optim_options_from_env(bad)
    import train_pandaset
    import train_with_fusion_ablation
    for mod in (train_pandaset, train_with_fusion_ablation):
        assert "optim_options_from_env()" in inspect.getsource(mod)
