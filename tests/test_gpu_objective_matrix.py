"""The KD objective with its hard-label term and its feature term combined: every hard_loss x feature_loss a user can reach.

(a) Model-free, against float64.  kdrt.losses.kd_objective (the autograd form) on synthetic logits, teacher logits and feature
    maps, then total.backward(): every part, the total, d/d logits, d/d camera_feat and d/d lidar_feat against the one plain-torch
    objective of tests/_fp64_objective_ref.py.  Each term is held to the bound its own GPU test applies, through that test's
    helper; the total to the sum of those bounds weighted by alpha * T^2 and beta, plus one float32 rounding of the running sum
    for each of the three additions of the total; d/d logits under a LovaszLoss to the base's bound plus the Lovasz term's.
(b) Through the small models of tests/test_gpu_multiclass_step.py with lr = 0: the autograd form against the fused form, bit for
    bit, for every combination; the hard-label choice leaves the feature parts' bits alone and the reverse.
(c) One KD step of the weighted student under four option pairs (every term once) against the float64 oracle of
    tests/_fp64_step_ref.py started from the device's own state, the objective of tests/_fp64_objective_ref.py in kd_loss's place.
(d) Teeth: each layer is watched going red on the wiring bug it exists for -- and staying green on the ones it cannot see.

All of it is one test id, test_objective_matrix, as tests/test_gpu_ifv_loss.py groups its parts; its runner runs every part whatever
the others did and names each part that failed.

Measured on an MI355X: profiles/objective_matrix_error.txt."""
import json
import os

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
import _ohem_ref as OH
import kd_oracle as O
from test_gpu_ifv_loss import _bounds as ifv_bounds
from test_gpu_multiclass_step import B as MB, CW as CW8, HW as MHW, N as MN, SEED as MSEED, _model
from test_gpu_pair_loss import _bounds as pair_bounds

pytestmark = pytest.mark.gpu

_REF = {}


# ---- (a) model-free, against float64 ----------------------------------------------------------------------------------------------

def _reference(case):
    """the float64 objective of a case with its gradients and every bound, computed once and shared (never modified)"""
    if case not in _REF:
        inp, hard, feature = M.case_setup(case)
        total, parts = M.case_objective(case, inp, hard, feature)
        total.backward()
        _REF[case] = (inp, hard, feature, total.detach(), parts, _bounds(case, inp, hard, feature, parts))
    return _REF[case]


def _hard_bounds(case, inp, hard):
    """-> ({part: bound}, bound of d/d logits [B, NC, HW]) from the references the per-term GPU tests check their kernels with"""
    zs, zt, y = M.flat3(inp)
    cw = inp["cw"].detach()
    ns = L.seg_n_seq(y.numel())
    if isinstance(hard, M.OhemCE):
        keep = M.ohem_keep(zs, y, case.ign, hard)[0]
        r = OH.ohem(zs, zt, y, cw, case.ign, M.T_KD, M.ALPHA, 1.0, keep, ns)
        g = M.ohem_gap(zs, y, case.ign, hard)
        e = r["vals"][1]
        share = torch.tensor(g["share"], dtype=torch.float64)
        return {"ce": e[0], "kl": e[1], "ce_all": e[3], "ohem_theta": torch.tensor(g["e_theta"], dtype=torch.float64),
                "ohem_kept": L._bound(1, share)}, r["dzs"][1]
    base = hard.base if isinstance(hard, M.LovaszLoss) else hard
    if base is None:
        r = L.seg_loss(zs, zt, y, cw, case.ign, M.T_KD, M.ALPHA, 1.0, ns)
        hv, out, e_g = r["losses"][0][0], {"ce": r["losses"][1][0], "kl": r["losses"][1][1]}, r["dzs"][1]
    else:
        r = RR.region_loss(zs, zt, y, cw, case.ign, M.T_KD, M.ALPHA, 1.0, ns, RR.spec(**base._asdict()))
        v, e = r["vals"]
        hv, out, e_g = v[0], {"ce": e[0], "kl": e[1], "focal": e[3], "tversky": e[4]}, r["dzs"][1]
    if isinstance(hard, M.LovaszLoss):
        lv = LV.lovasz(zs, y, case.ign, M.f32(hard.weight), 1.0, hv.item())
        out["ce"] = out["ce"] + lv["hard"][1]                       # the base call's bound and the bound of hard + weight * L
        out["lovasz"], out["class_lovasz"] = lv["vals"][1][0], lv["vals"][1][1:]
        e_g = e_g + lv["dzs"][1]                                     # the base's and the Lovasz term's
    return out, e_g


def _feature_bounds(case, inp, feature, key):
    """-> (bound of the value, bound of beta * d value / d student map [B, HW, C])"""
    S, T = M._rows(inp["ms"][key].detach()), M._rows(inp["mt"][key].detach())
    B, n, C = S.shape
    if feature is None:
        return L.mse_value(S, T, L.mse_n_seq(S.numel()))["loss"][1], L.mse_grad(S, T, L.f32(2.0 / S.numel()), M.BETA)["da"][1]
    if isinstance(feature, M.ChannelKD):
        tau = M.f32(feature.tau)
        r = CW.cwd(S, T, tau, L.f32(tau / (B * C)) * M.BETA)
        return r["val"][1], r["ds"][1]
    if isinstance(feature, M.PairKD):
        bv, _, bg = pair_bounds(PR.direct(S, T), PR.gram32(S.float(), T.float()))
    else:
        y = inp["target"].reshape(B, -1)
        bv, _, bg = ifv_bounds(IV.direct(S, T, y, case.NC, case.ign), IV.ifv32(S.float(), T.float(), y, case.NC, case.ign))
    return torch.tensor(bv, dtype=torch.float64), M.BETA * bg


def _bounds(case, inp, hard, feature, parts):
    parts_b, e_dzs = _hard_bounds(case, inp, hard)
    pre = M.feature_prefix(feature)
    grads_b = {"logits": e_dzs}
    for key, name in (("camera_feat", pre + "_cam"), ("lidar_feat", pre + "_lidar")):
        parts_b[name], grads_b[key] = _feature_bounds(case, inp, feature, key)
    # total = (ce + ckl * kl) + beta * (f_cam + f_lidar): the terms' bounds with their weights, and one float32 rounding of the
    # running sum for each of the three additions
    ckl = M.ALPHA * M.T_KD * M.T_KD
    t1 = parts["ce"] + ckl * parts["kl"]
    m = parts[pre + "_cam"] + parts[pre + "_lidar"]
    total_b = (parts_b["ce"] + ckl * parts_b["kl"] + M.BETA * (parts_b[pre + "_cam"] + parts_b[pre + "_lidar"])
               + L.U * (t1.abs() + m.abs() + (t1 + M.BETA * m).abs()))
    return parts_b, total_b, grads_b


def _device_objective(case, inp, hard, feature):
    """kd_objective on the case's float32 inputs, then total.backward() -> (total, parts, {"logits" / map: gradient})"""
    from kdrt import losses
    dev = lambda t, grad=False: t.detach().float().cuda().requires_grad_(grad)
    zs, ms = dev(inp["zs"], True), {k: dev(v, True) for k, v in inp["ms"].items()}
    total, parts = losses.kd_objective(zs, ms, dev(inp["zt"]), {k: dev(v) for k, v in inp["mt"].items()}, inp["target"].cuda(),
                                       dev(inp["cw"]), T=M.T_KD, alpha=M.ALPHA, beta=M.BETA, ignore_index=case.ign,
                                       feature_loss=M.to_kdrt(feature), hard_loss=M.to_kdrt(hard))
    total.backward()
    torch.cuda.synchronize()
    B, NC = zs.shape[:2]
    grads = {"logits": zs.grad.reshape(B, NC, -1)}
    grads.update({k: M._rows(v.grad) for k, v in ms.items()})
    return total.detach(), parts, grads


def matrix_case(case):
    """-> (worst |d| / bound, [what lies outside its bound]) of one case, every figure printed"""
    inp, hard, feature, total, parts, (parts_b, total_b, grads_b) = _reference(case)
    t_dev, p_dev, g_dev = _device_objective(case, inp, hard, feature)
    bad, worst = [], 0.0

    def look(name, got, want, bound):
        nonlocal worst
        got, want, bound = got.detach().double().cpu().reshape(want.shape), want.detach(), torch.as_tensor(bound).reshape(want.shape)
        d = (got - want).abs()
        ratio = (d / bound.clamp_min(1e-300)).max().item() if bool((d > 0).any()) else 0.0
        ratio = float("inf") if not bool(torch.isfinite(got).all()) else ratio
        worst = max(worst, ratio)
        print(f"{M.case_id(case)} {name}: largest |d| {d.max().item():.3g}, worst |d|/bound {ratio:.3g}")
        if not ratio <= 1.0:
            bad.append((name, ratio))
    assert set(p_dev) == set(parts) == M.part_names(hard, feature, autograd_form=True)
    for name in sorted(parts):
        look(name, p_dev[name], parts[name], parts_b[name])
    look("total", t_dev, total, total_b)
    look("d/d logits", g_dev["logits"], inp["zs"].grad.reshape(g_dev["logits"].shape), grads_b["logits"])
    for key in ("camera_feat", "lidar_feat"):
        look("d/d " + key, g_dev[key], M._rows(inp["ms"][key].grad), grads_b[key])
        assert bool(g_dev[key].abs().max() > 0)
    return worst, bad


def _part_a_objective_against_float64(combo):
    """every class count and both shapes of one hard x feature combination (and its ignore_index = 0 run, where it has one); all
    cases run and print before the assertion names the ones outside their bound"""
    cases = [c for c in M.CASES if (c.hard, c.feature) == combo]
    assert len(cases) >= 3
    results = {M.case_id(c): matrix_case(c) for c in cases}
    print(f"MATRIX {'+'.join(combo)}: largest |d| / bound {max(w for w, _ in results.values()):.3g} over {len(cases)} cases "
          f"(classes {sorted({c.NC for c in cases})})")
    bad = {k: b for k, (_, b) in results.items() if b}
    assert not bad, bad


# ---- (b) through the model, both forms ----------------------------------------------------------------------------------------------

_RIGS, _STEPS = {}, {}


def _rig(nc):
    """teacher, student, optimiser (lr = 0: no step moves a parameter) and batch of one class count, built once"""
    if nc not in _RIGS:
        from kdrt.optim import FusedAdamW
        images, pts, _ = O.make_inputs(MB, MHW, MN, 16, MSEED, pad_tail=40)
        labels = O.make_inputs(MB, MHW, MN, MHW // 4, MSEED, pad_tail=40, num_classes=nc)[2]      # labels live on the logits' grid
        teacher, _ = _model("concat", 11, num_classes=nc)
        student, _ = _model("weighted", 12, num_classes=nc)
        student.train()
        opt = FusedAdamW(student.parameters(), lr=0.0, weight_decay=0.0)
        cw = torch.tensor([0.4, 3.5] if nc == 2 else CW8).cuda()
        _RIGS[nc] = (teacher, student, opt, cw, (images.cuda(), pts.cuda(), labels.cuda()))
    return _RIGS[nc]


def model_step(nc, hard, feature, fused, beta=0.7):
    """one KD step through the model -> (parts without the logits, flat gradient), computed once per argument set"""
    key = (nc, hard, feature, fused, beta)
    if key not in _STEPS:
        from kdrt import gradsink
        from kdrt.kd import KDStep
        teacher, student, opt, cw, batch = _rig(nc)
        try:
            step = KDStep(student, teacher, opt, cw, T=M.T_KD, alpha=M.ALPHA, beta=beta, fused_objective=fused,
                          hard_loss=M.to_kdrt(M.HARDS[hard] if isinstance(hard, str) else hard), feature_loss=M.to_kdrt(M.FEATURES[feature]))
            parts = step(*batch)
            torch.cuda.synchronize()
            _STEPS[key] = ({k: v.clone() for k, v in parts.items() if k != "logits"}, opt.flat.grad.clone())
        finally:
            gradsink.uninstall()
            gradsink.drop_pending()
    return _STEPS[key]


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _require(ok, *info):
    """an assertion whose AssertionError carries `info` as a tuple (the teeth read it)"""
    if not ok:
        raise AssertionError(info)


def forms_agree(nc, hard, feature, beta=0.7):
    """the assertions of (b) for one combination"""
    spec = M.HARDS[hard] if isinstance(hard, str) else hard
    (p0, g0), (p1, g1) = model_step(nc, hard, feature, False, beta), model_step(nc, hard, feature, True, beta)
    want = M.part_names(spec, M.FEATURES[feature]) | {"total"}
    tag = f"nc{nc} {hard if isinstance(hard, str) else 'lovasz_region'}+{feature} beta {beta}"
    _require(set(p1) == want and set(p0) == M.part_names(spec, M.FEATURES[feature], autograd_form=True) | {"total"}, tag, "keys", sorted(p0), sorted(p1))
    for k in p1:
        _require(_same_bits(p0[k], p1[k]), tag, k, p0[k].tolist(), p1[k].tolist())
    _require(bool(torch.isfinite(g1).all()) and g1.abs().max() > 0, tag, "gradient finite and non-zero")
    _require(_same_bits(g0, g1), tag, "flat gradient", (g0 - g1).abs().max().item())
    return p1, g1


def _part_b_both_forms_two_classes(hard):
    for feature in M.FEATURES:
        forms_agree(2, M.LOVASZ_REGION if hard == "lovasz_region" else hard, feature)


def _part_b_both_forms_eight_classes():
    for hard in ("ce", "ohem"):
        for feature in M.FEATURES:
            forms_agree(8, hard, feature)


def _part_b_beta_zero():
    """beta = 0: no feature gradient is formed or deposited; the feature values are still reported and both forms still agree"""
    for hard, feature in zip(("ce", "region", "lovasz", "ohem"), M.FEATURES):
        p, g = forms_agree(2, hard, feature, beta=0.0)
        pb, gb = forms_agree(2, hard, feature)
        pre = M.feature_prefix(M.FEATURES[feature])
        assert _same_bits(p[pre + "_cam"], pb[pre + "_cam"]) and _same_bits(p[pre + "_lidar"], pb[pre + "_lidar"]) and _same_bits(p["ce"], pb["ce"])
        assert not _same_bits(g, gb) and not _same_bits(p["total"], pb["total"])


def _part_b_one_axis_leaves_the_other_axis_alone():
    """changing only the hard-label term leaves the bits of the feature parts (and of the KL) unchanged; changing only the feature
    term leaves the bits of the hard-label parts unchanged; and each choice does change its own parts and the gradient"""
    res = {(h, f): model_step(2, h, f, True) for h in M.HARDS for f in M.FEATURES}
    for f in M.FEATURES:
        pre = M.feature_prefix(M.FEATURES[f])
        for h in M.HARDS:
            for k in (pre + "_cam", pre + "_lidar", "kl"):
                assert _same_bits(res[(h, f)][0][k], res[("ce", f)][0][k]), (h, f, k)
            if h != "ce":
                assert not _same_bits(res[(h, f)][0]["ce"], res[("ce", f)][0]["ce"]) and not _same_bits(res[(h, f)][1], res[("ce", f)][1]), (h, f)
    for h in M.HARDS:
        for f in M.FEATURES:
            for k in M.part_names(M.HARDS[h], None) - {"mse_cam", "mse_lidar"}:
                assert _same_bits(res[(h, f)][0][k], res[(h, "mse")][0][k]), (h, f, k)
            if f != "mse":
                assert not _same_bits(res[(h, f)][1], res[(h, "mse")][1]), (h, f)


# ---- (c) one step through the model against the float64 oracle --------------------------------------------------------------------

_ORACLE = {}


def step_seeds():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp64_clean_seeds.json")
    return json.load(open(path))["objective"]


def oracle_refs(name, snap_state, t_state, batch):
    """the float64 and the float32 CPU oracle's step of a case from the device's initial state, computed once and shared"""
    hard, feature, nc, grid, _ = M.STEP_CASES[name]
    flat = torch.cat([v.double().flatten() for k, v in sorted(snap_state.items()) if v.is_floating_point()])
    if name in _ORACLE:
        assert torch.equal(flat, _ORACLE[name][0]), "the rig's initial state is the one the cached oracle step started from"
        return _ORACLE[name][1:]
    kw = dict(t_state=t_state, kd_objective=M.step_objective(name), cw=R.CW if nc == 2 else M.STEP_CW8, grid=grid)
    ref64 = R.oracle_step("kd", "weighted", snap_state, batch, torch.float64, **kw)
    ref32 = R.oracle_step("kd", "weighted", snap_state, batch, torch.float32, **kw)
    _ORACLE[name] = (flat, ref64, ref32)
    return ref64, ref32


def step_case(name):
    """one KD step of the weighted student under the case's options: losses, logits, every parameter gradient and the AdamW update
    against the float64 oracle started from the device's own initial state, with tests/_fp64_step_ref.py's assertions as they stand"""
    from kdrt import gradsink
    from test_gpu_step_sequence import Rig
    hard, feature, nc, grid, _ = M.STEP_CASES[name]
    batch = M.step_batch(name, step_seeds()[name][0])
    try:
        rig = Rig("kd", "weighted", num_classes=nc, grid=None if grid == R.G else grid,
                  step_kw={"hard_loss": M.to_kdrt(hard), "feature_loss": M.to_kdrt(feature)})
        snap = rig.cpu_state()
        t_state = {k: v.detach().cpu().clone() for k, v in rig.teacher.state_dict().items()}
        parts = rig.run(tuple(t.cuda() for t in batch))
        got = rig.cpu_state()
    finally:
        gradsink.uninstall()
        gradsink.drop_pending()
    ref64, ref32 = oracle_refs(name, snap["state"], t_state, batch)
    ok, text = M.step_gaps(name, ref64["logits"], batch[2])
    print(f"{name}: {text}")
    assert ok, (name, text)
    assert set(ref64["parts"]) == M.part_names(hard, feature) | {"total"} == {k for k in parts if k != "logits"}
    tag = f"objective step {name}"
    R.check_losses_and_logits({n: v.item() for n, v in parts.items() if n != "logits"}, parts["logits"].cpu(), ref64, ref32, tag)
    R.check_gradients(got["grads"], ref64, ref32, tag)
    names = list(got["grads"])
    R.check_adamw(({n: snap["state"][n] for n in names}, snap["exp_avg"], snap["exp_avg_sq"]),
                  ({n: got["state"][n] for n in names}, got["exp_avg"], got["exp_avg_sq"]), got["grads"], 1, snap["state"], tag, g64=ref64["grads"])


def _part_c_one_step_against_the_float64_oracle(name):
    step_case(name)


# ---- (d) teeth ----------------------------------------------------------------------------------------------------------------------

def _fresh():
    _STEPS.clear()


def _patch_lib_call(monkeypatch, edit):
    """edit(name, args list) -> args: applied to every entry-point call"""
    from kdrt.lib import lib
    real = type(lib).call
    monkeypatch.setattr(type(lib), "call", lambda self, name, *a: real(self, name, *edit(name, list(a))))


def _part_d_swapped_teacher_maps_are_caught_by_a_and_c_not_by_b(monkeypatch):
    """the teacher's camera_feat and lidar_feat swapped inside kd_objective and kd_objective_backward alike.  (a): caught (the two
    feature parts and both map gradients leave their bounds).  (c): caught (the feature parts of the step leave the oracle's).
    (b): not caught -- both forms carry the same mistake."""
    from kdrt import kd, losses
    swap = lambda mt: {**mt, "camera_feat": mt["lidar_feat"], "lidar_feat": mt["camera_feat"]}

    def wrap(real):
        return lambda zs, ms, zt, mt, *a, **kw: real(zs, ms, zt, swap(mt), *a, **kw)
    case = M.Case("ce", "mse", 2, "b2_16x16", -1)
    assert not matrix_case(case)[1]
    for name in ("kd_objective", "kd_objective_backward"):
        patched = wrap(getattr(losses, name))
        monkeypatch.setattr(losses, name, patched)
        monkeypatch.setattr(kd, name, patched)                      # KDStep calls the names kdrt.kd imported
    try:
        _fresh()
        worst, bad = matrix_case(case)
        print("swapped teacher maps, (a):", bad)
        assert {"mse_cam", "mse_lidar", "total", "d/d camera_feat", "d/d lidar_feat"} <= {n for n, _ in bad} and worst > 100
        swapped = forms_agree(2, "ce", "mse")                       # (b) stays green
        with pytest.raises(AssertionError) as err:
            step_case("ce+ifv-grid8")
        print("swapped teacher maps, (c):", err.value.args[0])
        assert err.value.args[0][1] in ("ifv_cam", "ifv_lidar")
    finally:
        monkeypatch.undo()
        _fresh()
    good = forms_agree(2, "ce", "mse")
    assert not _same_bits(swapped[0]["mse_cam"], good[0]["mse_cam"]) and not _same_bits(swapped[1], good[1]), "the patch was live in (b)"


def _part_d_beta_applied_again_in_the_total_is_caught_by_b_not_by_a_or_c(monkeypatch):
    """beta is folded into the feature gradient's coefficient; the fused form's total kernels receive beta * beta.  (b): caught (the
    total's bits differ between the forms, nothing else does).  (a): not caught -- it runs the autograd form, which never calls
    those kernels.  (c): not caught -- its steps run at beta = 1 (tests/_fp64_step_ref.py), where beta * beta is beta."""
    def edit(name, a):
        if name == "kd_kd_total":
            a[4] = a[4] * a[4]
        if name == "kd_kd_objective_final":
            a[6] = a[6] * a[6]
        return a
    _patch_lib_call(monkeypatch, edit)
    try:
        _fresh()
        for feature in ("mse", "cwd"):
            with pytest.raises(AssertionError) as err:
                forms_agree(2, "ce", feature)
            print("beta twice, (b):", err.value.args[0][:2])
            assert err.value.args[0][1] == "total"
        assert not matrix_case(M.Case("ce", "cwd", 2, "b3_12x20", -1))[1]
        step_case("region+cwd")
    finally:
        monkeypatch.undo()
        _fresh()
    forms_agree(2, "ce", "cwd")


def _part_d_total_reading_vals_under_ohem_is_caught_by_b_and_c_not_by_a(monkeypatch):
    """under OhemCE the hard-label term and the KL live in the OhemCE call's own buffer, not in slots 0 and 1 of `vals`, which that
    path never writes; the total kernels are handed such an 8-float buffer (here zero-filled, so the run is repeatable) in `hard`'s
    place.  (b): caught (the total).  (c): caught (the step's total against the oracle's).  (a): not caught -- the autograd form adds
    the total with torch operations."""
    stale = torch.zeros(8, device="cuda")

    def edit(name, a):
        if name in ("kd_kd_total", "kd_kd_objective_final"):
            a[0] = stale.data_ptr()
        return a
    _patch_lib_call(monkeypatch, edit)
    try:
        _fresh()
        for feature in ("mse", "ifv"):
            with pytest.raises(AssertionError) as err:
                forms_agree(2, "ohem", feature)
            print("vals for hard, (b):", err.value.args[0][:2])
            assert err.value.args[0][1] == "total"
        assert not matrix_case(M.Case("ohem", "mse", 2, "b2_16x16", -1))[1]
        with pytest.raises(AssertionError) as err:
            step_case("ohem+ifv-nc8")
        print("vals for hard, (c):", err.value.args[0])
        assert err.value.args[0][1] == "total"
    finally:
        monkeypatch.undo()
        _fresh()
    forms_agree(2, "ohem", "ifv")


def _part_d_skipped_lovasz_call_is_caught_by_a_and_c_not_by_b(monkeypatch):
    """the Lovasz call after its base call does nothing (its value slots read 0).  (a): caught ("ce", "lovasz", "class_lovasz", the
    total and d/d logits leave their bounds).  (c): caught ("lovasz" and "ce" against the oracle's).  (b): not caught -- both forms
    go through the same _hard_call."""
    from kdrt import losses
    case = M.Case("lovasz", "mse", 2, "b2_16x16", -1)
    assert not matrix_case(case)[1]
    monkeypatch.setattr(losses, "_lovasz_call", lambda spec, zs, target, ignore_index, gdev, vals, hard, dzs: vals.zero_())
    try:
        _fresh()
        worst, bad = matrix_case(case)
        print("skipped Lovasz call, (a):", bad)
        assert {"ce", "lovasz", "class_lovasz", "total", "d/d logits"} <= {n for n, _ in bad} and worst > 100
        skipped = forms_agree(2, "lovasz", "mse")                   # (b) stays green
        assert skipped[0]["lovasz"].item() == 0.0
        with pytest.raises(AssertionError) as err:
            step_case("lovasz_region+pair")
        print("skipped Lovasz call, (c):", err.value.args[0])
        assert err.value.args[0][1] in ("lovasz", "ce")
    finally:
        monkeypatch.undo()
        _fresh()
    assert forms_agree(2, "lovasz", "mse")[0]["lovasz"].item() > 0


def _part_cwd_with_lovasz_two_optimiser_steps():
    """ChannelKD + LovaszLoss through two real optimiser steps at lr 1e-3 (the body of the former
    tests/test_gpu_cwd_loss.py::test_with_lovasz_hard_loss: the documented parts, everything finite), and on top of it: the parameters
    after the two steps are the same bits under the fused and the autograd form, and the steps moved them"""
    from kdrt.losses import ChannelKD, LovaszLoss
    from test_gpu_region_loss import _kd_step
    kw = dict(feature_loss=ChannelKD(), hard_loss=LovaszLoss())
    p, g, w = _kd_step(1e-3, steps=2, **kw)
    assert set(p) == {"ce", "kl", "cwd_cam", "cwd_lidar", "total", "lovasz"}
    assert all(bool(torch.isfinite(p[k])) for k in p) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(w).all())
    pa, ga, wa = _kd_step(1e-3, steps=2, fused_objective=False, **kw)
    assert _same_bits(w, wa) and _same_bits(g, ga) and all(_same_bits(p[k], pa[k]) for k in p)
    assert not _same_bits(w, _kd_step(0.0, steps=1, **kw)[2])


# ---- the test of this file: every part runs, whatever the parts before it did, and the report names each part that failed ----------

def _parts():
    for combo in M.COMBOS:
        yield "(a) " + "+".join(combo), _part_a_objective_against_float64, (combo,), False
    for hard in list(M.HARDS) + ["lovasz_region"]:
        yield "(b) both forms, 2 classes, " + hard, _part_b_both_forms_two_classes, (hard,), False
    yield "(b) both forms, 8 classes", _part_b_both_forms_eight_classes, (), False
    yield "(b) beta = 0", _part_b_beta_zero, (), False
    yield "(b) one axis leaves the other alone", _part_b_one_axis_leaves_the_other_axis_alone, (), False
    yield "(b) ChannelKD + LovaszLoss, two optimiser steps", _part_cwd_with_lovasz_two_optimiser_steps, (), False
    for name in M.STEP_CASES:
        yield "(c) " + name, _part_c_one_step_against_the_float64_oracle, (name,), False
    yield "TEETH swapped teacher maps", _part_d_swapped_teacher_maps_are_caught_by_a_and_c_not_by_b, (), True
    yield "TEETH beta applied again in the total", _part_d_beta_applied_again_in_the_total_is_caught_by_b_not_by_a_or_c, (), True
    yield "TEETH total reading vals under OhemCE", _part_d_total_reading_vals_under_ohem_is_caught_by_b_and_c_not_by_a, (), True
    yield "TEETH skipped Lovasz call", _part_d_skipped_lovasz_call_is_caught_by_a_and_c_not_by_b, (), True


def test_objective_matrix(monkeypatch):
    """Every part above, each on its own: a part that fails does not stop the others, the patches and the memoised device results of
    a teeth part are gone before the next part starts (the other caches hold deterministic CPU references only), and the assertion
    names every part that failed, the teeth apart from the checks."""
    failed = {}
    for label, part, args, teeth in _parts():
        try:
            part(*args, *((monkeypatch,) if teeth else ()))
            print("PART ok:", label)
        except Exception as e:                                       # (a KDError is a finding too)
            print("PART FAILED:", label, repr(e)[:300])
            failed[label] = e
        finally:
            monkeypatch.undo()
            if teeth or label in failed:
                _fresh()
    assert not failed, {k: repr(v)[:500] for k, v in failed.items()}
