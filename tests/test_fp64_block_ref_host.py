"""Self-check of tests/_fp64_block_ref.py (the truth of tests/test_gpu_block_kernels.py) on the host: the references ARE the fused
blocks (compared in float64 with F.conv2d, groups = Ch, and a matmul -- independent of the references' own tap indexing), their
bounds hold for a plain fp32 evaluation and for an fp32 emulation of the kernels' split arithmetic (three bf16 pieces, K ascending,
one rounded add per piece product, the kernels' fma order) on the recipes of the GPU suite, reject seven wrong readings of the
contract, and on the exact recipe float32, float64 and the emulation agree bit for bit.

Measured here, worst element of the emulation / bound (printed as HOST ...): (32, 192, 64, stride 2) on 3 x 17 x 19 0.004,
(64, 96, 64, stride 1) on 3 x 9 x 17 0.005, (64, 384, 64, stride 1) on 20 x 36 0.002; the short chains use most (32 hidden channels
on a 1 x 1 map: 0.01 - 0.035).  The bounds are worst-case chains, and every wrong reading misses them by a factor of 5e3 or more
(printed as WRONG ...)."""
import pytest
import torch
import torch.nn.functional as F

import _fp64_block_ref as R

D = torch.float64
RED = [R.red_case(i) for i in R.INST]
HOST = R.CASES                                                     # the GPU suite's whole table: it is small


def _gen(c, exact=False):
    return torch.Generator().manual_seed(R.seed_of(c, exact))


def _ratio(got, ref):
    val, err = ref
    return ((got.double() - val).abs() / err.clamp_min(1e-300)).max().item()


def _shares(c, d, pre):
    """the rule of the GPU suite: a ReLU6 operand of at least 4096 elements has 1 % of its pre-activations in every regime"""
    for what, raw, sc, sh in R.relu6_operands(c, d, pre):
        if raw.numel() >= 4096:
            assert min(R.relu6_shares(raw, sc, sh)) >= 0.01, (what, R.relu6_shares(raw, sc, sh))


# ---- the references are the operations they claim to be ----------------------------------------------------------------------

def _stock_tail(a, wd, dsc, dsh, dact, wp, pbias, psc, psh, pact, res, stride):
    Ch = a.shape[-1]
    y = F.conv2d(a.permute(0, 3, 1, 2), wd.view(Ch, 1, 3, 3), stride=stride, padding=1, groups=Ch).permute(0, 2, 3, 1)
    h = R.act(y * dsc + dsh, dact).reshape(-1, Ch)
    return R.act((h @ wp.t() + pbias) * psc + psh, pact) + res


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W", [(2, 6, 8), (1, 7, 9), (2, 6, 9), (2, 7, 8), (3, 1, 11), (2, 11, 1), (1, 1, 1), (1, 16, 17), (1, 15, 15)],
                         ids=lambda v: str(v))
def test_references_are_conv2d_and_matmul(B, H, W, stride):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + W + stride)
    r = lambda *s: torch.randn(*s, generator=g, dtype=D)
    Cin, Ch, Cout = 5, 8, 6
    Mo = B * R._out_size(H, stride) * R._out_size(W, stride)
    x, xe = 2 * r(B, H, W, Ch), r(B, H, W, Cin)
    we, eb, wd, wp, pb, res = r(Ch, Cin), r(Ch), r(Ch, 9), r(Cout, Ch), r(Cout), r(Mo, Cout)
    (isc, ish), (esc, esh), (dsc, dsh), (psc, psh) = ((-r(n), r(n) + 2) for n in (Ch, Ch, Ch, Cout))
    for iact, dact, pact in ((2, 2, 0), (1, 1, 1), (0, 2, 2)):
        tail = (wd, dsc, dsh, dact, wp, pb, psc, psh, pact, res, stride)
        want = _stock_tail(R.act(x * isc + ish, iact), *tail)
        got = R.dw_pw_infer(x, isc, ish, iact, *tail)[0]
        assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
        want = _stock_tail(R.act(x, 0), *tail)
        assert (R.dw_pw_infer(x, None, None, iact, *tail)[0] - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())
        want = _stock_tail(R.act((xe @ we.t() + eb) * esc + esh, iact), *tail)
        got = R.block_infer(xe, we, eb, esc, esh, iact, *tail)[0]
        assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_n_seq_is_the_count_of_the_kernel_source():
    """bias and residual present: (Cin + 4 + 1 + 1) + (9 + 1) + (Ch + 4 + 1 + 1) + 1; the tail alone with a deferred input: 1 + ..."""
    for inst, Ch, want in (("block_s2", 96, 151), ("block_s1", 64, 151), ("block_s2", 192, 247), ("block_s1", 384, 471),
                           ("dwpw_s1_64", 384, 1 + 10 + 384 + 4 + 3), ("dwpw_s2_64", 32, 1 + 10 + 32 + 4 + 3)):
        blk = R.INST[inst][0] == "kd_block_infer"
        c = R.Case(inst, 1, 3, 4, Ch, None if blk else "relu6", 2, 0, True, True, 0, 2 if blk else None, True if blk else None)
        pre = {}
        R.reference(c, R.to_double(R.inputs(torch.Generator().manual_seed(1), c)), pre=pre)
        assert pre["n_seq"] == want, (inst, Ch, pre["n_seq"], want)
    c = R.Case("dwpw_s1_32", 1, 3, 4, 32, "asis", 2, 0, False, False, 0, None, None)
    pre = {}
    R.reference(c, R.to_double(R.inputs(torch.Generator().manual_seed(1), c)), pre=pre)
    assert pre["n_seq"] == 10 + 32 + 4 + 1


def test_case_table_covers_every_value():
    """every map, hidden width, batch size and argument variant meets every instance at least once"""
    for inst, (fn, stride, _, _) in R.INST.items():
        cs = [c for c in R.CASES if c.inst == inst]
        assert {(c.H, c.W) for c in cs} == {(1, 1), (1, 23), (23, 1), (5, 7)} | ({(8, 16), (9, 17), (20, 36)} if stride == 1 else {(15, 15), (16, 16), (17, 19)})
        assert {c.Ch for c in cs} == {32, 64, 96, 384 if stride == 1 else 192}
        assert {c.B for c in cs} == {1, 3}
        assert max(c.B * c.H * c.W * c.Ch for c in cs) <= 2 * 20 * 36 * 384
        for field, values in (("dact", {1, 2}), ("pact", {0, 1}), ("pbias", {False, True}), ("res", {False, True}), ("pad", {0, 4})):
            assert {getattr(c, field) for c in cs} == values, (inst, field)
        if fn == "kd_dw_pw_infer":
            assert {c.inp for c in cs} == set(R.INPUT_MODES)
        else:
            assert {c.eact for c in cs} == {1, 2} and {c.ebias for c in cs} == {False, True}
        red = R.red_case(inst)
        assert red.res and red.inp != "asis" and red.H > 1 and red.W > 1
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    assert set().union(*(R.wrongs_of(c) for c in RED)) == set(R.WRONGS)


# ---- the bounds hold for honest fp32 and for the emulated split arithmetic ------------------------------------------------------

@pytest.mark.parametrize("c", HOST, ids=R.case_id)
def test_bounds_hold_for_fp32_and_for_the_split_emulation(c):
    d = R.inputs(_gen(c), c)
    pre = {}
    ref = R.reference(c, R.to_double(d), pre=pre)
    _shares(c, d, pre)
    r32, rem = _ratio(R.reference(c, d)[0], ref), _ratio(R.emulate(c, d), ref)
    print(f"\nHOST {R.case_id(c)} fp32 {r32:.4f} emulation {rem:.4f}")
    assert r32 <= 1.0, f"plain fp32 evaluation {r32:.3g}x the bound"
    assert rem <= 1.0, f"emulated split arithmetic {rem:.3g}x the bound"


# ---- the bounds have teeth ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", RED, ids=R.case_id)
def test_goes_red(c):
    """against the emulated kernel output, every wrong reading of the contract is outside the bound; on the exact recipe it is unequal"""
    for exact in (False, True):
        d = R.inputs(_gen(c, exact), c, exact)
        d64 = R.to_double(d)
        em = R.emulate(c, d)
        assert _ratio(em, R.reference(c, d64)) <= (0.0 if exact else 1.0)
        for w in R.wrongs_of(c):
            wr = R.reference(c, d64, wrong=w)
            if exact:
                assert not torch.equal(em.double(), wr[0]), f"exact recipe: equal to the reference with {R.WRONGS[w]}"
            else:
                r = _ratio(em, wr)
                print(f"\nWRONG {R.case_id(c)} {w}: {r:.3g}x the bound")
                assert r > 1.0, f"the reference with {R.WRONGS[w]} is within the bound ({r:.3g}x)"


# ---- the exact recipe ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", HOST, ids=R.case_id)
def test_exact_recipe_is_exact(c):
    d = R.inputs(_gen(c, True), c, exact=True)
    pre = {}
    r64 = R.reference(c, R.to_double(d), pre=pre)[0]
    assert R.exact_headroom(pre) < 2 ** 24
    _shares(c, d, pre)
    r32, em = R.reference(c, d)[0], R.emulate(c, d)
    assert r32.dtype == torch.float32 and em.dtype == torch.float32
    assert torch.equal(r32.double(), r64), "float32 and float64 evaluations of the exact recipe differ"
    assert torch.equal(em.double(), r64), "the split emulation of the exact recipe differs from float64"


@pytest.mark.parametrize("inst,B,H,W,Ch", [("block_s2", 2, 17, 19, 96), ("block_s1", 1, 9, 17, 384), ("dwpw_s2_64", 2, 17, 19, 192)])
def test_exact_recipe_meets_both_clamps(inst, B, H, W, Ch):
    """at or below 0, inside (0, 6), at or above 6: at least 10 % of each ReLU6 pre-activation of the exact recipe"""
    blk = R.INST[inst][0] == "kd_block_infer"
    c = R.Case(inst, B, H, W, Ch, None if blk else "relu6", 2, 0, True, True, 0, 2 if blk else None, True if blk else None)
    d = R.inputs(_gen(c, True), c, exact=True)
    pre = {}
    R.reference(c, R.to_double(d), pre=pre)
    ops = [("depthwise", pre["d_raw"].float(), d["dsc"], d["dsh"])]
    ops.append(("expand", pre["e_raw"].float(), d["esc"], d["esh"]) if blk else ("input", d["x"], d["isc"], d["ish"]))
    for what, raw, sc, sh in ops:
        shares = R.relu6_shares(raw, sc, sh)
        print(f"\nSHARES {inst} {what} {shares[0]:.3f} / {shares[1]:.3f} / {shares[2]:.3f}")
        assert min(shares) >= 0.10, (what, shares)
