"""CPU tests of the BEV label rules: the numpy mirror (tests/_label_rule_ref.py) on hand-worked cells, one per tie level of each
rule; its agreement with the first-point oracle where a cell holds one class; LabelRule and class_weights_from_counts (validation
and values); the ablation script's environment parsing; the C ABI of the three entry points (declared, exported, refusals that
return before a launch)."""
import json

import numpy as np
import pytest

import _label_rule_ref as R
import data_oracle as D

RANGE = (-50, 50, -50, 50)


# ---- the mirror on hand-worked cells ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counts, rank, min_points, want, votes", [
    ([0, 3, 5, 1], None, 1, 2, 5),                       # majority: the largest count
    ([0, 4, 4, 1], [0, 0, 1, 5], 1, 2, 4),               # equal counts -> the larger rank (class 3 outranks both but has fewer points)
    ([0, 4, 4, 4], [0, 2, 2, 2], 1, 1, 4),               # equal counts and ranks -> the smaller class
    ([0, 3, 5, 1], None, 4, 2, 5),                       # min_points: 1 and 3 are not eligible
    ([0, 5, 3, 1], None, 4, 1, 5),
    ([0, 3, 5, 1], None, 6, 0, 0),                       # nobody eligible: background
    ([9, 0, 0, 0], None, 1, 0, 0),                       # a count in column 0 is not a vote
])
def test_majority_by_hand(counts, rank, min_points, want, votes):
    m, v = R.resolve(np.array([counts], np.int64), R.MAJORITY, rank, min_points)
    assert (int(m[0]), int(v[0])) == (want, votes)


@pytest.mark.parametrize("counts, rank, min_points, want, votes", [
    ([0, 9, 1, 0], [0, 1, 5, 9], 1, 2, 1),               # priority: the largest rank among the classes PRESENT (3 has no point)
    ([0, 2, 7, 7], [0, 3, 3, 1], 1, 2, 7),               # equal ranks -> the larger count
    ([0, 5, 5, 0], [0, 2, 2, 2], 1, 1, 5),               # equal ranks and counts -> the smaller class
    ([0, 9, 1, 0], [0, 1, 5, 9], 2, 1, 9),               # min_points moves the winner to the runner-up ...
    ([0, 9, 1, 0], [0, 1, 5, 9], 10, 0, 0),              # ... and then to background
    ([0, 2, 3, 0], [7, -4, -9, 0], 1, 1, 2),             # negative ranks order like any integers; rank[0] is ignored
    ([0, 2, 3, 4], None, 1, 3, 4),                       # no ranks: all equal, the count decides
])
def test_priority_by_hand(counts, rank, min_points, want, votes):
    m, v = R.resolve(np.array([counts], np.int64), R.PRIORITY, rank, min_points)
    assert (int(m[0]), int(v[0])) == (want, votes)


def test_counts_by_hand():
    """grid 2 x 2 over [-50, 50]^2: trunc((v + 50) / 100 * 1) is 1 only at v = 50, so three cells collect the edges"""
    x = np.array([0, 0, 0, 50, 50, -50, np.nan, 60, 0, 0, 0], np.float32)
    y = np.array([0, 0, 0, 0, 50, 50, 0, 0, 0, 0, 0], np.float32)
    c = np.array([1, 2, 2, 3, 3, 1, 2, 2, 0, -1, 4], np.int64)          # the last three count nowhere with NC = 4
    cnt = R.cell_counts(x, y, c, (2, 2), RANGE, 4)
    assert cnt.tolist() == [[0, 1, 2, 0], [0, 0, 0, 1], [0, 1, 0, 0], [0, 0, 0, 1]]
    m, v = R.rasterize_vote(x, y, c, (2, 2), RANGE, 4, R.MAJORITY)
    assert m.tolist() == [[2, 3], [1, 3]] and v.tolist() == [[2, 1], [1, 1]]
    assert R.cell_counts(x, y, c, (2, 2), RANGE, 5)[0].tolist() == [0, 1, 2, 0, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_class_per_cell_equals_the_first_point_oracle(seed):
    """with at most one non-zero class per cell no rule has anything to decide"""
    r = np.random.RandomState(seed)
    grid, NC, n = (8, 12), 6, 900
    x, y = (r.randn(n) * 30).astype(np.float32), (r.randn(n) * 30).astype(np.float32)
    keep, row, col = D.bev_cells(x, y, grid, RANGE)
    cell_class = r.randint(1, NC, grid[0] * grid[1])
    c = np.zeros(n, np.int64)
    c[keep] = cell_class[row * grid[1] + col]
    c[r.rand(n) < 0.3] = 0                                                # background points anywhere
    want = D.rasterize_bev(x, y, c, grid, RANGE)
    assert len(np.unique(want)) > 3
    rank = r.randint(-3, 4, NC)
    for rule in (R.MAJORITY, R.PRIORITY):
        assert np.array_equal(R.rasterize_vote(x, y, c, grid, RANGE, NC, rule, rank)[0], want)


def test_histogram_mirror():
    assert R.label_histogram([0, 1, 1, 3, -1, 4, 99, 2], 4).tolist() == [1, 2, 1, 1, 3]
    assert R.label_histogram(np.zeros((0,), np.int64), 3).tolist() == [0, 0, 0, 0]


# ---- LabelRule ----------------------------------------------------------------------------------------------------------------

def test_label_rule_values():
    import dataclasses
    from src.data_loading.pandaset_dataset import LabelRule
    r = LabelRule()
    assert (r.kind, r.priority, r.min_points, r.code) == ("majority", None, 1, 1)
    assert r.ranks(5).tolist() == [0] * 5 and r.ranks(5).dtype == np.int32
    p = LabelRule("priority", {3: 7, 1: -2}, min_points=np.int64(3))
    assert p.code == 2 and p.min_points == 3 and isinstance(p.min_points, int)
    assert p.ranks(4).tolist() == [0, -2, 0, 7] and p.ranks(16).tolist() == [0, -2, 0, 7] + [0] * 12
    s = LabelRule("majority", [0, 5, 4, 3])
    assert s.priority == (0, 5, 4, 3) and s.ranks(4).tolist() == [0, 5, 4, 3]
    assert LabelRule("majority", np.array([0, 1, 2])).ranks(3).tolist() == [0, 1, 2]
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.kind = "priority"


@pytest.mark.parametrize("kw, match", [
    (dict(kind="first"), "kind"), (dict(kind="Majority"), "kind"), (dict(kind=1), "kind"),
    (dict(min_points=0), "min_points"), (dict(min_points=-2), "min_points"), (dict(min_points=1.5), "min_points"),
    (dict(min_points=True), "min_points"), (dict(min_points="2"), "min_points"),
    (dict(priority=[0, 1.5, 2]), "integer"), (dict(priority={1: "high"}), "integer"), (dict(priority={"1": 2}), "integer"),
    (dict(priority=[0, True]), "integer"), (dict(priority={1: 1 << 31}), "int32"),
    (dict(priority={16: 1}), "class index"), (dict(priority={-1: 1}), "class index"),
    (dict(priority=[1]), "one rank per class"), (dict(priority=list(range(17))), "one rank per class"),
    (dict(priority="road"), "priority"), (dict(priority=3), "priority"), (dict(priority=np.zeros((2, 2), int)), "priority"),
])
def test_label_rule_refuses(kw, match):
    from src.data_loading.pandaset_dataset import LabelRule
    with pytest.raises(ValueError, match=match):
        LabelRule(**kw)


def test_label_rule_against_a_class_map():
    from src.data_loading.pandaset_dataset import (LabelRule, SyntheticRawPandaSet, create_pandaset_dataloaders,
                                                   rasterize_bev_batch)
    cmap = {3: 4, 9: 7}                                                   # classes 0..7
    ds = SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map=cmap, label_rule=LabelRule("priority", {7: 2, 4: 1}))
    assert ds.label_rule.kind == "priority" and ds.num_classes == 8
    assert SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map=cmap).label_rule is None
    with pytest.raises(ValueError, match="names class 8"):
        SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map=cmap, label_rule=LabelRule("priority", {8: 1}))
    with pytest.raises(ValueError, match="4 ranks"):
        SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map=cmap, label_rule=LabelRule("majority", [0, 1, 2, 3]))
    with pytest.raises(ValueError, match="needs a class_map"):
        SyntheticRawPandaSet(n_frames=2, sweep_points=10, label_rule=LabelRule())
    with pytest.raises(ValueError, match="LabelRule"):
        SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map=cmap, label_rule="majority")
    with pytest.raises(ValueError, match="needs a class_map"):
        create_pandaset_dataloaders("/nonexistent/pandaset", ["001"], ["002"], verbose=False, label_rule=LabelRule())
    with pytest.raises(ValueError, match="names class 9"):
        create_pandaset_dataloaders("/nonexistent/pandaset", ["001"], ["002"], verbose=False, class_map=cmap,
                                    label_rule=LabelRule("priority", {9: 1}))
    tr, va = create_pandaset_dataloaders("/nonexistent/pandaset", ["001"], ["002"], verbose=False, class_map=cmap, label_rule=LabelRule())
    assert tr.dataset.num_classes == 8
    # a pickled copy (a spawned worker's) carries the rule and no device tensor
    import pickle
    ds._rank_dev = object()
    assert pickle.loads(pickle.dumps(ds.__getstate__()))["_rank_dev"] is None
    # the batch call refuses a rule it cannot honour before it touches the device
    one = [np.zeros(1, np.float32)]
    for kw in (dict(rule=LabelRule()), dict(rule=LabelRule(), remap=True, num_classes=4), dict(rule="majority", num_classes=4),
               dict(want_votes=True), dict(rule=LabelRule(), num_classes=17), dict(rule=LabelRule("majority", [0, 1, 2]), num_classes=4)):
        with pytest.raises(ValueError):
            rasterize_bev_batch(one, one, [np.zeros(1, np.int64)], **kw)


def test_label_counts_refuses_to_run_on_cpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("checks the no-GPU behaviour")
    from kdrt import KDError
    from src.data_loading.pandaset_dataset import LabelRule, SyntheticRawPandaSet
    ds = SyntheticRawPandaSet(n_frames=2, sweep_points=10, class_map={3: 4, 9: 7}, label_rule=LabelRule())
    with pytest.raises(KDError, match="no CPU fallback"):
        ds.label_counts()
    with pytest.raises(ValueError, match="batch_size"):
        ds.label_counts(batch_size=0)


# ---- class weights ------------------------------------------------------------------------------------------------------------

def test_class_weights_from_counts():
    from kdrt.losses import class_weights_from_counts
    w = class_weights_from_counts([600, 300, 100])
    assert all(type(v) is float for v in w)
    assert w == [0.3 / 0.6, 0.3 / 0.3, 0.3 / 0.1]                        # median frequency 0.3
    w = class_weights_from_counts(np.array([70, 0, 20, 10, 0], np.int64))
    assert w[1] == 0.0 and w[4] == 0.0                                    # absent classes: weight 0, and they do not move the median
    assert w == R.median_freq_weights([70, 0, 20, 10, 0]) and w[2] == 1.0
    even = class_weights_from_counts([5, 15, 30, 50])                     # four classes present: the median is the mean of the middle two
    assert np.allclose(even, [0.225 / 0.05, 0.225 / 0.15, 0.225 / 0.30, 0.225 / 0.50], rtol=1e-15)
    big = class_weights_from_counts([1 << 40, 1 << 20, 1])
    assert big == R.median_freq_weights([1 << 40, 1 << 20, 1]) and big[1] == 1.0
    assert class_weights_from_counts([0, 7]) == [0.0, 1.0]
    for bad in ([0, 0, 0], [], [3, -1], [1.5, 2], [[1, 2]], [float("nan"), 1], ["a", "b"]):
        with pytest.raises(ValueError):
            class_weights_from_counts(bad)
    with pytest.raises(ValueError, match="scheme"):
        class_weights_from_counts([1, 2], scheme="inverse")


# ---- the ablation script's knobs ----------------------------------------------------------------------------------------------

def test_label_rule_from_env():
    import train_with_fusion_ablation as S
    assert S.label_rule_from_env(8, {}) is None
    assert S.label_rule_from_env(8, {"KD_LABEL_RULE": "first"}) is None
    r = S.label_rule_from_env(8, {"KD_LABEL_RULE": "majority"})
    assert (r.kind, r.priority, r.min_points) == ("majority", None, 1)
    r = S.label_rule_from_env(4, {"KD_LABEL_RULE": "priority", "KD_LABEL_MIN_POINTS": "3", "KD_CLASS_PRIORITY": "[0, 3, 2, 1]"})
    assert (r.kind, r.priority, r.min_points) == ("priority", (0, 3, 2, 1), 3)
    r = S.label_rule_from_env(8, {"KD_LABEL_RULE": "majority", "KD_CLASS_PRIORITY": json.dumps({"5": 2, "1": -1})})
    assert r.ranks(8).tolist() == [0, -1, 0, 0, 0, 2, 0, 0]
    for env in ({"KD_LABEL_RULE": "median"}, {"KD_LABEL_RULE": "majority", "KD_LABEL_MIN_POINTS": "two"},
                {"KD_LABEL_RULE": "majority", "KD_LABEL_MIN_POINTS": "0"},
                {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": "road>car"}, {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": "3"},
                {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": '{"road": 1}'}, {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": "[0, 1.5]"},
                {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": "[0, 1, 2]"},          # three ranks, eight classes
                {"KD_LABEL_RULE": "priority", "KD_CLASS_PRIORITY": '{"8": 1}'},           # class 8 of 0..7
                {"KD_LABEL_MIN_POINTS": "2"}, {"KD_LABEL_RULE": "first", "KD_CLASS_PRIORITY": "[0, 1]"}):
        with pytest.raises(ValueError, match="KD_LABEL_RULE|KD_LABEL_MIN_POINTS|KD_CLASS_PRIORITY|LabelRule"):
            S.label_rule_from_env(8, env)


def test_class_weights_from_env():
    import train_with_fusion_ablation as S
    assert S.class_weights_from_env(3, {}) is None and S.class_weights_from_env(3, {"KD_CLASS_WEIGHTS": "default"}) is None
    assert S.class_weights_from_env(3, {"KD_CLASS_WEIGHTS": "median_freq"}) == "median_freq"
    w = S.class_weights_from_env(3, {"KD_CLASS_WEIGHTS": "[0.5, 2, 3.25]"})
    assert w == [0.5, 2.0, 3.25] and all(type(v) is float for v in w)
    for text in ("[1, 2]", "[1, 2, 3, 4]", "balanced", "[1, -2, 3]", '[1, "2", 3]', "[1, true, 3]", "[1, NaN, 3]", '{"0": 1}', "1.0"):
        with pytest.raises(ValueError, match="KD_CLASS_WEIGHTS"):
            S.class_weights_from_env(3, {"KD_CLASS_WEIGHTS": text})


def test_the_label_knobs_are_read_with_a_class_map_only(monkeypatch):
    """without KD_CLASS_MAP the script's set-up is the parent's: multiclass_from_env returns (None, None) and nothing else is parsed"""
    import inspect
    import train_with_fusion_ablation as S
    for k in ("KD_NUM_CLASSES", "KD_CLASS_MAP"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("KD_LABEL_RULE", "nonsense")
    assert S.multiclass_from_env() == (None, None)
    src = inspect.getsource(S.train_fusion_variant)
    assert src.index("if class_map is not None:") < src.index("label_rule_from_env(") < src.index("create_pandaset_dataloaders(")


# ---- C ABI --------------------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_refuse_before_a_launch():
    from kdrt.lib import lib
    for name in ("kd_bev_rasterize_vote_ws_bytes", "kd_bev_rasterize_vote", "kd_label_histogram"):
        assert name in lib.protos and getattr(lib, name) is not None
    ws = lib.kd_bev_rasterize_vote_ws_bytes
    assert ws(3, 8, 12, 2) == ws(3, 8, 12, 4) == 3 * 8 * 12 * 4 * 4
    assert ws(3, 8, 12, 5) == ws(3, 8, 12, 8) == 3 * 8 * 12 * 8 * 4
    assert ws(3, 8, 12, 9) == ws(3, 8, 12, 16) == 3 * 8 * 12 * 16 * 4
    assert ws(3, 8, 12, 17) == 0 and ws(3, 8, 12, 1) == 0 and ws(0, 8, 12, 4) == 0
    fake = 4096                                            # non-null, aligned; every call below returns before it is used
    def vote(NC=4, rule=1, min_points=1, B=1, n=0, H=2, W=2, wsp=fake, nbytes=1 << 20, mask=fake, off=fake):
        return lib.kd_bev_rasterize_vote(None, None, None, off, B, n, NC, rule, None, min_points, H, W, -50.0, 100.0, 50.0, -50.0,
                                         100.0, 50.0, wsp, nbytes, mask, None, None)
    assert vote(NC=17) == -4 and vote(NC=1) == -4
    assert vote(rule=0) == -1 and b"first-point rule is kd_bev_rasterize" in lib.kd_last_error_string()
    assert vote(rule=3) == -1
    assert vote(min_points=0) == -1 and b"min_points" in lib.kd_last_error_string()
    assert vote(n=5) == -1                                 # null point arrays
    assert vote(mask=None) == -1 and vote(off=None) == -1 and vote(B=0) == -1
    assert vote(wsp=fake + 4) == -2
    assert vote(nbytes=15) == -3
    assert vote(B=1 << 12, H=1 << 10, W=1 << 10) == -4     # more than 2^31 counters
    assert lib.kd_label_histogram(fake, 5, 17, fake, None) == -4 and lib.kd_label_histogram(fake, 5, 0, fake, None) == -4
    assert lib.kd_label_histogram(fake, 5, 4, None, None) == -1 and lib.kd_label_histogram(None, 5, 4, fake, None) == -1
    assert lib.kd_label_histogram(None, 0, 4, fake, None) == 0          # n = 0: nothing is launched
