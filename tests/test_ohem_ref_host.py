"""tests/_ohem_ref.py on the CPU: the bit-exact selection against a brute-force sort (random inputs and inputs full of ties), the
float64 reference of the whole call against an independent torch expression, the bounds it states met by a plain fp32 evaluation,
the OhemCE / KD_HARD_LOSS=ohem validation, the header and the library, and the reference-only condition of the set-agreement check
of tests/test_gpu_ohem_loss.py: for every case of its continuous and dropped-label scenes the share of valid pixels inside the
margin (see _ohem_ref's docstring) is at most 2 %."""
import ctypes
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fp64_loss_ref as L
import _ohem_ref as R


def _brute(nll, mask, lam, min_kept, min_divisor):
    """the definition, by a full descending sort of (bits, index) pairs in Python integers"""
    bits = [int(b) & 0x7FFFFFFF for b in np.asarray(nll, dtype=np.float32).view(np.uint32)]
    valid = sorted((bits[i] for i in range(len(bits)) if mask[i]), reverse=True)
    n = len(valid)
    m = min(n, max(min_kept, (n + min_divisor - 1) // min_divisor))
    lam_bits = int(np.array([lam], dtype=np.float32).view(np.uint32)[0])
    if n == 0:
        return 0, None, lam_bits, [False] * len(bits)
    tau = valid[m - 1]
    theta = min(tau, lam_bits)
    return m, tau, theta, [bool(mask[i]) and bits[i] >= theta for i in range(len(bits))]


def _as_bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("kind", ["random", "ties", "narrow", "nan", "none_valid"])
def test_select_is_the_brute_force_sort(kind):
    rng = np.random.default_rng(5)
    for trial in range(40):
        n = int(rng.integers(1, 400))
        nll = (rng.standard_normal(n) ** 2 * 2).astype(np.float32)
        if kind == "ties":
            nll = rng.choice(np.array([0.0, 0.25, 0.25000003, 1.5, 7.0], dtype=np.float32), n)
        elif kind == "narrow":
            nll = (np.float32(0.6931472) + rng.integers(-20, 20, n).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
        elif kind == "nan" and n > 2:
            nll[rng.integers(0, n)] = np.nan
        mask = rng.random(n) < (0.0 if kind == "none_valid" else 0.8)
        lam = R.lam_of(float(rng.choice([1.0, 0.7, 0.2, 1e-30])))
        min_kept, min_divisor = int(rng.choice([1, 5, 10 ** 6])), int(rng.choice([1, 3, 16, 2 ** 40]))
        m, tau, theta, keep = R.select(nll, mask, lam, min_kept, min_divisor)
        bm, btau, btheta, bkeep = _brute(nll, mask, lam, min_kept, min_divisor)
        assert m == bm and _as_bits(theta) == btheta and keep.tolist() == bkeep, (kind, trial)
        assert (tau is None) == (btau is None) and (tau is None or _as_bits(tau) == btau)
        if m:
            assert int(keep.sum()) >= m                       # at least m, more only by ties at tau_m or by the threshold
            if lam >= 60:
                assert int(keep.sum()) == int((R._bits(nll)[mask] >= btau).sum())


def test_select_known_answers():
    nll = np.array([0.5, 2.0, 2.0, 2.0, 0.1, 9.0, 0.0, 3.0], dtype=np.float32)
    mask = np.array([1, 1, 1, 1, 1, 0, 1, 1], dtype=bool)
    big = R.lam_of(1e-30)
    m, tau, theta, keep = R.select(nll, mask, big, 1, 3)                    # n = 7, m = 3: 3.0 and the tie group at 2.0
    assert (m, float(tau), float(theta)) == (3, 2.0, 2.0) and keep.tolist() == [False, True, True, True, False, False, False, True]
    m, tau, theta, keep = R.select(nll, mask, R.lam_of(0.7), 1, 16)         # the threshold 0.357 decides
    assert m == 1 and float(tau) == 3.0 and _as_bits(theta) == _as_bits(R.lam_of(0.7)) and int(keep.sum()) == 5
    assert R.select(nll, mask, big, 100, 16)[3].tolist() == mask.tolist()    # min_kept > n
    assert R.select(nll, mask, 0.0, 1, 16)[3].tolist() == mask.tolist()      # thresh = 1
    assert R.select(nll, mask, big, 1, 1)[3].tolist() == mask.tolist()       # min_divisor = 1
    assert R.select(np.full(5, 1.25, np.float32), np.ones(5, bool), big, 1, 16)[3].all()
    assert R.lam_of(1.0) == 0.0 and math.copysign(1.0, R.lam_of(1.0)) == 1.0


def _d(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("NC,teacher,weights", [(2, True, True), (5, False, True), (16, True, False)])
def test_ohem_reference_is_the_cross_entropy_over_the_kept_pixels(NC, teacher, weights):
    B, HW, ign, T = 3, 61, -1, 4.0
    zs, zt, y, cw = R.ohem_inputs(B, NC, HW, 3 + NC, "cpu", "dropped", ign, teacher, weights)
    zs, zt, cw = _d(zs), _d(zt), _d(cw)
    alpha, gs = R.f32(0.7) if teacher else 0.0, R.f32(2.5)
    valid, l, e_l = R.per_pixel(zs, y, ign)
    s = R.select64(l, e_l, valid, R.lam_of(1e-30), 1, 4)
    keep = s["keep"].reshape(B, HW)
    assert int(keep.sum()) == s["m"] == -(-int(valid.sum()) // 4)
    r = R.ohem(zs, zt, y, cw, ign, T, alpha, gs, keep, n_seq=1)
    z = zs.clone().requires_grad_()
    nll = F.cross_entropy(z, torch.where(valid, y, torch.full_like(y, 0)), reduction="none")
    assert (nll.detach() * valid - l).abs().max().item() < 1e-12
    w = (torch.ones(NC, dtype=torch.float64) if cw is None else cw)[torch.where(valid, y, torch.zeros_like(y))] * keep
    hard = (w * nll).sum() / w.sum()
    kl = torch.zeros((), dtype=torch.float64)
    if teacher:
        kl = F.kl_div(torch.log_softmax(z / T, 1), torch.log_softmax(zt / T, 1), reduction="sum", log_target=True) / (B * HW)
    (gs * (hard + alpha * T * T * kl)).backward()
    wa = (torch.ones(NC, dtype=torch.float64) if cw is None else cw)[torch.where(valid, y, torch.zeros_like(y))] * valid
    want = torch.stack([hard.detach(), kl.detach(), w.sum(), (wa * nll.detach()).sum() / wa.sum()])
    assert (r["vals"][0] - want).abs().max().item() < 1e-12
    assert (r["dzs"][0] - z.grad).abs().max().item() < 1e-12
    if not teacher:
        assert bool((r["dzs"][0][(valid & ~keep).reshape(B, 1, HW).expand(B, NC, HW)] == 0).all())


def _within(r64, r32, what):
    for k, (v, err) in r64.items():
        d = (r32[k][0].double() - v).abs()
        ok = (d <= err) | (torch.isnan(v) & torch.isnan(r32[k][0]))
        assert bool(ok.all()), (what, k, (d / err.clamp_min(1e-300)).max().item())


CPU_CASES = [c for c in R.CASES if c[0] != "ragged"] + [c for c in R.CASES if c[0] == "ragged" and c[2] in R.SET_SCENES]


@pytest.mark.parametrize("case", CPU_CASES, ids=R.case_id)
def test_fp32_evaluation_meets_the_bounds(case):
    """the house convention: the same formulas in plain fp32, the selection on the fp32 l, held to the float64 bounds over that set"""
    (zs, zt, y, cw), a = R.case_setup(case, "cpu")
    valid, l32, _ = R.per_pixel(zs, y, a["ign"])
    _, l64, e_l = R.per_pixel(zs.double(), y, a["ign"])
    assert bool(((l32.double() - l64).abs() <= e_l).all())
    assert bool((l32 >= 0).all())
    keep = torch.from_numpy(R.select(l32, valid, a["lam"], a["min_kept"], a["min_divisor"])[3]).reshape(y.shape)
    args = (a["ign"], a["T"], a["alpha"], a["gs"], keep, a["n_seq"])
    _within(R.ohem(zs.double(), _d(zt), y, _d(cw), *args), R.ohem(zs, zt, y, cw, *args), R.case_id(case))


@pytest.mark.parametrize("case", [c for c in R.CASES if c[2] in R.SET_SCENES], ids=R.case_id)
def test_margin_share_of_the_set_agreement_cases(case):
    """the reference-only condition of check 4 of tests/test_gpu_ohem_loss.py, on the CPU from float64 alone"""
    (zs, zt, y, cw), a = R.case_setup(case, "cpu")
    valid, l, e_l = R.per_pixel(zs.double(), y, a["ign"])
    s = R.select64(l, e_l, valid, a["lam"], a["min_kept"], a["min_divisor"])
    n = int(valid.sum())
    print(f"{R.case_id(case)}: n {n} m {s['m']} theta {s['theta']:.6g} e_theta {s['e_theta']:.3g} margin {int(s['margin'].sum())} ({s['share'] * 100:.3f} %)")
    assert n > 0 and s["share"] <= R.MARGIN_CAP, (R.case_id(case), s["share"])
    assert s["m"] <= int(s["keep"].sum()) <= n


def test_cases_cover_what_the_issue_lists():
    assert {c[1] for c in R.CASES} == {2, 3, 4, 5, 8, 9, 16} and {c[0] for c in R.CASES} == set(R.SHAPES)
    assert {c[2] for c in R.CASES} == {"continuous", "dropped", "narrow", "ties", "identical", "ignored"}
    assert {c[5] for c in R.CASES} == set(R.PARAMS)
    assert {c[3] for c in R.CASES} == {True, False} and {c[4] for c in R.CASES} == {True, False}
    assert R.SHAPES["ragged"][0] * R.SHAPES["ragged"][1] > 1024 * 256 and L.seg_layout(17 * 16384)[1] == 2
    # a tie case puts m inside a tie group, the narrow band leaves the first two digits to one bucket each
    for case in R.CASES:
        if case[2] in ("ties", "narrow") and case[0] == "partial_block":
            (zs, _, y, _), a = R.case_setup(case, "cpu")
            valid, l32, _ = R.per_pixel(zs, y, a["ign"])
            m, tau, theta, keep = R.select(l32, valid, a["lam"], a["min_kept"], a["min_divisor"])
            bits = R._bits(l32)[valid.reshape(-1).numpy()]
            if case[2] == "ties":
                assert int(keep.sum()) > m               # (the kernel sees 5 * NC distinct l at most; a vectorised CPU softmax may
                                                         # split a group by an ulp, which only makes this harder to meet)
            else:
                assert len(np.unique(bits >> 10)) == 1 and len(np.unique(bits)) > 1


def test_ohem_ce_validation():
    from kdrt.losses import OhemCE
    assert OhemCE() == OhemCE(thresh=0.7, min_divisor=16, min_kept=1)
    assert OhemCE(1, 1, 1).lam() == 0.0 and math.copysign(1.0, OhemCE(1.0).lam()) == 1.0
    assert OhemCE(0.7).lam() == R.lam_of(0.7) == float(np.float32(-math.log(0.7)))
    for bad in (dict(thresh=0.0), dict(thresh=-0.1), dict(thresh=1.0001), dict(thresh=float("nan")), dict(thresh=float("inf")),
                dict(thresh=True), dict(thresh="0.7"), dict(thresh=None), dict(min_divisor=0), dict(min_divisor=-3), dict(min_divisor=16.0),
                dict(min_divisor=True), dict(min_kept=0), dict(min_kept=1.5), dict(min_kept=False), dict(min_kept="1")):
        with pytest.raises(ValueError, match="OhemCE"):
            OhemCE(**bad)
    with pytest.raises(Exception):
        OhemCE().thresh = 0.5                                   # frozen


def test_ablation_script_reads_the_ohem_knobs():
    import train_with_fusion_ablation as S
    from kdrt.losses import LovaszLoss, OhemCE, RegionLoss
    assert S.hard_loss_from_env({}) is None and S.hard_loss_from_env({"KD_HARD_LOSS": "ce"}) is None
    assert S.hard_loss_from_env({"KD_OHEM_THRESH": "0.5"}) is None          # unset behaves as before, the knobs are not read
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "focal_tversky"}) == RegionLoss()
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "ce_lovasz"}) == LovaszLoss()
    assert S.hard_loss_from_env({"KD_HARD_LOSS": "ohem"}) == OhemCE()
    got = S.hard_loss_from_env({"KD_HARD_LOSS": "ohem", "KD_OHEM_THRESH": "0.9", "KD_OHEM_MIN_DIVISOR": "8", "KD_OHEM_MIN_KEPT": "1000"})
    assert got == OhemCE(thresh=0.9, min_divisor=8, min_kept=1000)
    for bad in ({"KD_OHEM_THRESH": "0"}, {"KD_OHEM_THRESH": "1.5"}, {"KD_OHEM_THRESH": "nan"}, {"KD_OHEM_THRESH": "hard"},
                {"KD_OHEM_MIN_DIVISOR": "0"}, {"KD_OHEM_MIN_DIVISOR": "2.5"}, {"KD_OHEM_MIN_KEPT": "-1"}, {"KD_OHEM_MIN_KEPT": "many"}):
        with pytest.raises(ValueError):
            S.hard_loss_from_env({"KD_HARD_LOSS": "ohem", **bad})
    with pytest.raises(ValueError, match="'ohem'"):
        S.hard_loss_from_env({"KD_HARD_LOSS": "topk"})
    for knob in ("KD_OHEM_THRESH", "KD_OHEM_MIN_DIVISOR", "KD_OHEM_MIN_KEPT"):
        assert knob in S.__doc__


def test_header_declares_and_library_exports_the_entry_points():
    from kdrt.lib import HEADER_PATH, SO_PATH, parse_header
    protos = parse_header(HEADER_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(HEADER_PATH).read(), flags=re.S)
    dll = ctypes.CDLL(SO_PATH)
    for name in ("kd_seg_ohem_fwd_bwd", "kd_seg_ohem_ws_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in protos
        assert hasattr(dll, name)
    V_, I, F_, Z, Q = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t, ctypes.c_int64
    assert protos["kd_seg_ohem_ws_bytes"] == (Z, [Q])
    assert protos["kd_seg_ohem_fwd_bwd"] == (I, [V_, V_, V_, V_, I, F_, F_, F_, V_, F_, Q, Q, V_, V_, V_, V_, V_, I, I, I, V_, Z, V_])
    # the workspace size is a host function: no device needed
    dll.kd_seg_ohem_ws_bytes.restype, dll.kd_seg_ohem_ws_bytes.argtypes = Z, [Q]
    for npix in (1, 6, 183, 262144, 278528):
        assert dll.kd_seg_ohem_ws_bytes(npix) == R.ws_bytes(npix)
    assert dll.kd_seg_ohem_ws_bytes(0) == 0
