"""The float64 reference of tests/_fp64_region_loss_ref.py (the truth of tests/test_gpu_region_loss.py) on the CPU: its closed-form
gradient against torch.autograd on the same formula written with stock ops, gamma = 0 / wt = 0 against the weighted-CE reference
of tests/_fp64_loss_ref.py, the bound it states met by a plain fp32 evaluation of itself on every case of the GPU ladder, and
two wrong formulas (a and b swapped, the 1/NC dropped) landing outside that bound."""
import pytest
import torch

import _fp64_loss_ref as L
import _fp64_region_loss_ref as R

D = torch.float64


def _rel_close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


def _small(NC, seed, weights=True, teacher=True, absent=False, ign=-1):
    zs, zt, y, cw = R.region_inputs(3, NC, 61, seed, "cpu", ign, weights, teacher, absent)
    d = lambda t: None if t is None else t.double()
    return d(zs), d(zt), y, d(cw)


@pytest.mark.parametrize("pset", list(R.PSETS) + ["gamma1.5", "focal_only_s"])
@pytest.mark.parametrize("teacher", [True, False], ids=["teacher", "hard_only"])
@pytest.mark.parametrize("weights", [True, False], ids=["weights", "unweighted"])
@pytest.mark.parametrize("NC", [2, 3, 4])
def test_closed_form_is_autograd_of_the_definition(NC, weights, teacher, pset):
    extra = {"gamma1.5": {"gamma": 1.5}, "focal_only_s": {"s": 0.25, "a": 0.2, "b": 1.1}}
    sp = R.spec(**(R.PSETS[pset] if pset in R.PSETS else extra[pset]))
    ign, T, alpha, gs = (255 if NC == 3 else -1), 4.0, R.f32(0.7), R.f32(2.5) * R.f32(0.5)
    zs, zt, y, cw = _small(NC, 5 * NC + len(pset), weights, teacher, absent=NC != 3, ign=ign)
    r = R.region_loss(zs, zt, y, cw, ign, T, alpha, gs, 1, sp)
    z = zs.clone().requires_grad_()
    total, hard, focal, tv = R.autograd_loss(z, zt, y, cw, ign, T, alpha, sp)
    (gs * total).backward()
    v = r["vals"][0]
    _rel_close(v[0], hard.detach())
    if sp["wf"] > 0:
        _rel_close(v[3], focal.detach())
    else:
        assert v[3].item() == 0.0
    if sp["wt"] > 0:
        _rel_close(v[4], tv.detach())
        assert bool(((v[5:] > 0) & (v[5:] <= 1)).all())
    else:
        assert v[4].item() == 0.0 and bool((v[5:] == 0).all())
    _rel_close(r["dzs"][0], z.grad)
    assert bool((r["vals"][1] >= 0).all()) and bool((r["dzs"][1] >= 0).all()) and bool(torch.isfinite(r["dzs"][1]).all())


@pytest.mark.parametrize("teacher", [True, False], ids=["teacher", "hard_only"])
@pytest.mark.parametrize("NC", [2, 3, 4])
def test_gamma0_wt0_is_the_weighted_cross_entropy(NC, teacher):
    zs, zt, y, cw = _small(NC, 40 + NC, True, teacher)
    a = (-1, 4.0, R.f32(0.7), R.f32(1.25), 1)
    r = R.region_loss(zs, zt, y, cw, *a, R.spec(gamma=0.0, wt=0.0))
    ce = L.seg_loss(zs, zt, y, cw, *a)
    _rel_close(r["vals"][0][:3], ce["losses"][0])
    _rel_close(r["vals"][0][3], ce["losses"][0][0])
    _rel_close(r["dzs"][0], ce["dzs"][0])


def test_all_ignored_batch():
    zs, zt, y, cw = _small(3, 9)
    y = torch.full_like(y, -1)
    r = R.region_loss(zs, None, y, cw, -1, 4.0, 1.0, 1.0, 1, R.spec(wf=0.0))
    # no kept pixel: TP = A = N = 0, every TI = s / s = 1, Tversky = 0, and nothing depends on the logits
    assert r["vals"][0][0].item() == 0.0 and bool((r["vals"][0][5:] == 1).all()) and bool((r["dzs"][0] == 0).all())
    assert bool((r["dzs"][1] == 0).all())
    r = R.region_loss(zs, zt, y, cw, -1, 4.0, 1.0, 1.0, 1, R.spec())
    assert bool(torch.isnan(r["vals"][0][0])) and bool(torch.isnan(r["vals"][0][3])) and r["vals"][0][4].item() == 0.0
    assert bool(torch.isfinite(r["dzs"][0]).all())                 # the KL part alone
    kl = L.seg_loss(zs, zt, y, cw, -1, 4.0, 1.0, 1.0, 1)
    _rel_close(r["dzs"][0], kl["dzs"][0])


def _within(r64, r32, what):
    for k, (v, err) in r64.items():
        d = (r32[k][0].double() - v).abs()
        ok = (d <= err) | (torch.isnan(v) & torch.isnan(r32[k][0]))
        assert bool(ok.all()), (what, k, (d / err.clamp_min(1e-300)).max().item())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_fp32_evaluation_meets_the_bound(case):
    tensors, a = R.case_setup(case, "cpu")
    r64 = R.case_reference(case, tensors, a)
    assert bool(torch.isfinite(r64["vals"][0]).all())
    _within(r64, R.case_reference(case, tensors, a, dtype=torch.float32), R.case_id(case))


def test_cases_cover_what_the_gpu_test_promises():
    cs = R.CASES
    assert {c.size for c in cs} == set(R.LADDER) and {c.NC for c in cs} == {2, 3, 4}
    for size in R.LADDER:
        sub = [c for c in cs if c.size == size]
        assert {c.grad for c in sub} == {True, False} and {c.teacher for c in sub} == {True, False}
        assert {c.weights for c in sub} == {True, False}
    assert {c.pset for c in cs if c.size in ("few", "partial_block")} == set(R.PSETS)
    assert {c.pset for c in cs if c.size not in ("few", "partial_block")} == set(R.PSETS)
    assert {c.absent for c in cs} == {True, False}
    # the inputs hold what they promise: ignored, out-of-range and negative labels, both ends of the logit gap, an absent class
    c = next(c for c in cs if c.size == "cap+1" and c.NC == 3 and c.absent)
    (zs, zt, y, cw), a = R.case_setup(c, "cpu")
    share = (y == a["ign"]).float().mean().item()
    assert 0.17 < share < 0.23 and bool((y == c.NC + 1).any()) and bool((y == -7).any()) and not bool((y == c.NC - 1).any())
    py = torch.softmax(zs.double(), 1).gather(1, y.clamp(0, c.NC - 1).view(a["B"], 1, a["HW"]))[:, 0].reshape(-1)[:512]
    assert bool((py > 1 - 1e-15).any()) and bool((py < 1e-16).any()) and bool((py > 0).all())
    for size, (B, HW) in R.LADDER.items():
        grid, iters = R.seg_layout(B * HW)
        assert (grid, iters) == {"few": (1, 1), "partial_block": (1, 1), "cap-1": (1024, 1), "cap": (1024, 1), "cap+1": (1024, 2),
                                 "ragged": (1024, 3)}[size]
    assert R.LADDER["ragged"][0] == 3 and R.LADDER["ragged"][1] % 256 != 0


@pytest.mark.parametrize("mutation", ["swap_ab", "no_mean"])
@pytest.mark.parametrize("NC", [2, 3, 4])
def test_a_wrong_formula_lands_outside_the_bound(NC, mutation):
    # wf = 0: L_hard is the Tversky term alone (with the focal term in, its share of L_hard's bound hides a small move of a and b)
    c = R.Case("partial_block", NC, True, True, True, "wf0", False, 0)
    tensors, a = R.case_setup(c, "cpu")
    good, bad = R.case_reference(c, tensors, a), R.case_reference(c, tensors, a, mutate=mutation)
    for k, idx in (("vals", 0), ("vals", 4)):
        d = (bad[k][0][idx] - good[k][0][idx]).abs()
        assert d > good[k][1][idx], (k, idx, d.item(), good[k][1][idx].item())
    d = (bad["dzs"][0] - good["dzs"][0]).abs()
    assert (d > good["dzs"][1]).double().mean().item() > 0.25                  # the kept pixels outside the logit-gap block
