"""tests/_fp64_objective_ref.py on the CPU: every term of the combined objective, value and gradient, against that term's own
float64 reference; the sum against _fp64_loss_ref.kd_total; and, for every case tests/test_gpu_objective_matrix.py runs, the
condition under which the reference's discrete choices (OhemCE's mined set, the Lovasz order) are the device's too."""
import json
import os

import numpy as np
import pytest
import torch

import _fp64_cwd_ref as CW
import _fp64_ifv_ref as IV
import _fp64_loss_ref as L
import _fp64_lovasz_ref as LV
import _fp64_objective_ref as M
import _fp64_pair_ref as PR
import _fp64_region_loss_ref as RR
import _fp64_step_ref as R
import kd_oracle as O
import _ohem_ref as OH

RTOL, ATOL = 1e-9, 1e-13                          # two float64 evaluations of one formula in different operation orders


def _close(what, got, want):
    got, want = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(want, dtype=torch.float64)
    d = (got - want).abs()
    assert got.shape == want.shape and bool((d <= ATOL + RTOL * want.abs().max()).all()), (what, d.max().item(), want.abs().max().item())


def _evaluate(c, dtype=torch.float64):
    inp, hard, feature = M.case_setup(c, dtype)
    total, parts = M.case_objective(c, inp, hard, feature)
    total.backward()
    return inp, hard, feature, total.detach(), parts


def _hard_reference(c, inp, hard):
    """-> (hard value, kl, dzs [B, NC, HW], {part: value}) assembled from the per-term references"""
    zs, zt, y = M.flat3(inp)
    cw = inp["cw"].detach()
    npix = y.numel()
    ns = L.seg_n_seq(npix)
    extra = {}
    if hard is None:
        r = L.seg_loss(zs, zt, y, cw, c.ign, M.T_KD, M.ALPHA, 1.0, ns)
        return r["losses"][0][0], r["losses"][0][1], r["dzs"][0], extra
    if isinstance(hard, M.OhemCE):
        keep = M.ohem_keep(zs, y, c.ign, hard)[0]
        r = OH.ohem(zs, zt, y, cw, c.ign, M.T_KD, M.ALPHA, 1.0, keep, ns)
        g = M.ohem_gap(zs, y, c.ign, hard)
        extra = {"ce_all": r["vals"][0][3], "ohem_theta": g["theta"], "ohem_kept": g["share"]}
        return r["vals"][0][0], r["vals"][0][1], r["dzs"][0], extra
    base = hard.base if isinstance(hard, M.LovaszLoss) else hard
    if base is None:
        r = L.seg_loss(zs, zt, y, cw, c.ign, M.T_KD, M.ALPHA, 1.0, ns)
        hv, kl, g = r["losses"][0][0], r["losses"][0][1], r["dzs"][0]
    else:
        r = RR.region_loss(zs, zt, y, cw, c.ign, M.T_KD, M.ALPHA, 1.0, ns, RR.spec(**base._asdict()))
        hv, kl, g = r["vals"][0][0], r["vals"][0][1], r["dzs"][0]
        extra = {"focal": r["vals"][0][3], "tversky": r["vals"][0][4]}
    if isinstance(hard, M.LovaszLoss):
        lv = LV.lovasz(zs, y, c.ign, M.f32(hard.weight), 1.0, hv.item())
        extra.update(lovasz=lv["vals"][0][0], class_lovasz=lv["vals"][0][1:])
        hv, g = lv["hard"][0], g + lv["dzs"][0]
    return hv, kl, g, extra


def _feature_reference(c, inp, feature, key):
    """-> (value, beta * d value / d student map as [B, H * W, C]) from the term's own reference"""
    S, T = M._rows(inp["ms"][key].detach()), M._rows(inp["mt"][key].detach())
    B, n, C = S.shape
    if feature is None:
        return L.mse_value(S, T, 1)["loss"][0], L.mse_grad(S, T, 2.0 / S.numel() * M.BETA)["da"][0]
    if isinstance(feature, M.ChannelKD):
        tau = M.f32(feature.tau)
        r = CW.cwd(S, T, tau, M.BETA * tau / (B * C))
        return r["val"][0], r["ds"][0]
    if isinstance(feature, M.PairKD):
        r = PR.direct(S, T)
    else:
        r = IV.direct(S, T, inp["target"].reshape(B, -1), c.NC, c.ign)
    return r["val"], M.BETA * r["grad"]


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_every_term_against_its_own_reference(case):
    inp, hard, feature, total, parts = _evaluate(case)
    B, NC = inp["zs"].shape[:2]
    assert set(parts) == M.part_names(hard, feature, autograd_form=True)
    hv, kl, g, extra = _hard_reference(case, inp, hard)
    _close("ce", parts["ce"], hv)
    _close("kl", parts["kl"], kl)
    _close("d/d logits", inp["zs"].grad.reshape(B, NC, -1), g)
    assert set(extra) == set(parts) - {"ce", "kl"} - {k for k in parts if k.endswith(("_cam", "_lidar"))}
    for k, v in extra.items():
        _close(k, parts[k], v)
    pre = M.feature_prefix(feature)
    fv = {}
    for key, name in (("camera_feat", pre + "_cam"), ("lidar_feat", pre + "_lidar")):
        fv[name], fg = _feature_reference(case, inp, feature, key)
        _close(name, parts[name], fv[name])
        _close("d/d " + key, M._rows(inp["ms"][key].grad), fg)
        assert parts[name].item() > 0 and bool(inp["ms"][key].grad.abs().max() > 0)
    # the two maps are told apart: their values differ
    assert parts[pre + "_cam"].item() != parts[pre + "_lidar"].item()
    # the sum: kd_total rounds every operation to float32, so the float64 sum lies within its five roundings ...
    ckl = M.ALPHA * M.T_KD * M.T_KD
    want = L.kd_total(parts["ce"].item(), parts["kl"].item(), fv[pre + "_cam"].item(), fv[pre + "_lidar"].item(), ckl, M.BETA)
    mag = abs(parts["ce"].item()) + abs(ckl * parts["kl"].item()) + M.BETA * (parts[pre + "_cam"].item() + parts[pre + "_lidar"].item())
    assert abs(total.item() - float(want)) <= 6 * L.U * mag, (total.item(), float(want))
    # ... and the float32 evaluation of the same objective forms its total by exactly those operations (once per combination)
    if case != next(c for c in M.CASES if (c.hard, c.feature) == (case.hard, case.feature)):
        return
    _, _, _, t32, p32 = _evaluate(case, torch.float32)
    want32 = L.kd_total(p32["ce"].item(), p32["kl"].item(), p32[pre + "_cam"].item(), p32[pre + "_lidar"].item(), ckl, M.BETA)
    assert np.float32(t32.item()).view(np.int32) == want32.view(np.int32), (t32.item(), float(want32))
    assert abs(t32.item() - total.item()) <= 1e-4 * abs(total.item())


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_inputs_and_discrete_choices_are_stable(case):
    """labels: ignore_index pixels, out-of-range labels, a class absent from one image; the mined set and the Lovasz order of the
    float64 reference survive the float32 error of the quantities they are read from"""
    inp, hard, feature = M.case_setup(case)
    zs, zt, y = M.flat3(inp)
    B, NC = zs.shape[:2]
    assert bool((y == case.ign).any()) and bool((y == NC + 1).any()) and bool((y == -7).any())
    present = [[bool(((y[b] == k) & (y[b] != case.ign)).any()) for k in range(NC)] for b in range(B)]
    assert not present[B - 1][NC - 1] and present[0][NC - 1], "class NC - 1 is absent from the last image only"
    ok, text = M.stability(zs, y, case.ign, hard)
    print(M.case_id(case), text)
    assert ok, text
    if isinstance(hard, M.OhemCE):
        g = M.ohem_gap(zs, y, case.ign, hard)
        assert g["rank"] == (hard is M.OHEM_RANK) and 0 < g["share"] < 1
        assert g["gap"] > g["e_theta"], "theta stands clear of every other l"


def test_case_list_covers_the_matrix():
    combos = {(c.hard, c.feature) for c in M.CASES}
    assert combos == set(M.COMBOS) and len(combos) == 16
    for h, f in M.COMBOS:
        ncs = {c.NC for c in M.CASES if (c.hard, c.feature) == (h, f) and c.ign == -1}
        assert {2, 4} <= ncs and (3 in ncs) == (h in ("region", "lovasz")) and ({8, 16} <= ncs) == (h in ("ce", "ohem"))
        assert {c.shape for c in M.CASES if (c.hard, c.feature) == (h, f)} == set(M.SHAPES)
    specs = [M.case_specs(c)[0] for c in M.CASES]
    assert M.LOVASZ_REGION in specs and M.HARDS["lovasz"] in specs and M.OHEM_RANK in specs and M.HARDS["ohem"] in specs
    assert sum(c.ign == 0 for c in M.CASES) >= 1
    for f, widths in M.SHAPES["b3_12x20"][3].items():
        assert all(w % 4 == 0 for pair in widths for w in pair) and all(any(w & (w - 1) for w in pair) for pair in widths), "no power of two"
        assert f in ("mse", "cwd") or all(a != b for a, b in widths), "student and teacher widths differ"
    assert (3 * 12 * 20) % 256 and (12 * 20) % 256


def test_swapping_the_teachers_maps_changes_the_reference():
    """the wiring error the GPU test must see is visible in the reference's own numbers"""
    for c in (M.Case("ce", "mse", 2, "b2_16x16", -1), M.Case("region", "cwd", 3, "b2_16x16", -1)):
        inp, hard, feature = M.case_setup(c)
        good = M.case_objective(c, inp, hard, feature)[0]
        inp["mt"] = {"camera_feat": inp["mt"]["lidar_feat"], "lidar_feat": inp["mt"]["camera_feat"]}
        bad = M.case_objective(c, inp, hard, feature)[0]
        assert abs(good.item() - bad.item()) > 1e-3 * abs(good.item())


def test_to_kdrt_round_trip():
    from kdrt import losses
    for spec in (M.REGION, M.LOVASZ_REGION, M.HARDS["lovasz"], M.HARDS["ohem"], M.OHEM_RANK, M.FEATURES["cwd"], M.FEATURES["pair"], M.FEATURES["ifv"]):
        k = M.to_kdrt(spec)
        assert type(k).__name__ == type(spec).__name__ and type(k).__module__ == losses.__name__
        for name, v in spec._asdict().items():
            assert (getattr(k, name) == v) if name != "base" else ((k.base is None) == (v is None))
    assert M.to_kdrt(None) is None


@pytest.mark.parametrize("name", list(M.STEP_CASES))
def test_step_cases_on_the_cpu(name):
    """The one-step cases of tests/test_gpu_objective_matrix.py (c): every golden batch seed meets the gap condition on the logits of
    the float64 oracle's forward pass from the student's initial state (the state the device's step starts from)."""
    hard, feature, nc, grid, every = M.STEP_CASES[name]
    seeds = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp64_clean_seeds.json")))["objective"][name]
    state = {k: (v.double() if v.is_floating_point() else v) for k, v in R.random_state(R.build_model("weighted", nc, grid=grid), R.STUDENT_SEED).items()}
    assert seeds
    for seed in seeds:
        images, pts, labels = M.step_batch(name, seed)
        assert (every == 1) == (int((labels == -1).sum()) < labels.numel() // 2)
        with torch.no_grad():
            zs, _ = O.complete_model(images.double(), pts.double(), O.clone_state(state), fusion_type="weighted", grid=(grid, grid), training=True)
        ok, text = M.step_gaps(name, zs, labels)
        print(name, seed, text)
        assert ok, (name, seed, text)


def test_one_step_case_with_the_float32_oracle_in_the_devices_place():
    """the plumbing of (c) on the CPU, once: the objective callable inside oracle_step, the documented part names, and the float32
    oracle's step inside the assertions the device's step has to pass"""
    name = "lovasz_region+pair"
    hard, feature, nc, grid, _ = M.STEP_CASES[name]
    seeds = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp64_clean_seeds.json")))["objective"][name]
    state = R.random_state(R.build_model("weighted", nc, grid=grid), R.STUDENT_SEED)
    kw = dict(t_state=R.random_state(R.build_model("concat", nc, grid=grid), R.TEACHER_SEED), kd_objective=M.step_objective(name), cw=R.CW, grid=grid)
    batch = M.step_batch(name, seeds[0])
    ref64 = R.oracle_step("kd", "weighted", state, batch, torch.float64, **kw)
    ref32 = R.oracle_step("kd", "weighted", state, batch, torch.float32, **kw)
    assert set(ref64["parts"]) == M.part_names(hard, feature) | {"total"}
    assert all(v == v and abs(v) < 1e3 for v in ref64["parts"].values()) and ref64["parts"]["pair_lidar"] > 0
    R.check_losses_and_logits(ref32["parts"], ref32["logits"], ref64, ref32, name)
    R.check_gradients(ref32["grads"], ref64, ref32, name)


def test_oracle_step_default_objective_is_unchanged():
    """kd_objective=None is kd_oracle.kd_loss: the same parts as passing it explicitly, bit for bit"""
    state, batch = R.student_state("weighted"), R.inputs(1)
    a = R.oracle_step("kd", "weighted", state, batch, torch.float32)
    b = R.oracle_step("kd", "weighted", state, batch, torch.float32, kd_objective=O.kd_loss, cw=R.CW, grid=R.G)
    assert a["parts"] == b["parts"] and set(a["parts"]) == {"ce", "kl", "mse_cam", "mse_lidar", "total"}
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
