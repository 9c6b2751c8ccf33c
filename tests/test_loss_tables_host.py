"""CPU tests of the two tables of loss terms in kdrt.losses: every accepted spec class (and None, the default) has a row, the rows
name the parts kd_objective's docstring documents, and every place that takes a `hard_loss=` / `feature_loss=` refuses another type
with the one message that names every accepted class.  Nothing here touches a device."""
import pytest

from kdrt import losses
from kdrt.losses import (FEATURE_LOSSES, HARD_LOSSES, ChannelKD, IntraClassKD, LovaszLoss, OhemCE, PairKD, RegionLoss,
                         check_feature_loss, check_hard_loss)

HARD_SPECS = {RegionLoss: RegionLoss(), LovaszLoss: LovaszLoss(), OhemCE: OhemCE()}
FEATURE_SPECS = {ChannelKD: ChannelKD(), PairKD: PairKD(), IntraClassKD: IntraClassKD()}

# what parts gains beside "ce" and "kl", per form: the term's own *_seg_loss function (its names in the objective's spelling),
# kd_objective, kd_objective_backward
HARD_PARTS = [
    (None, set(), set(), set()),
    (RegionLoss(), {"focal", "tversky", "class_ti"}, {"focal", "tversky"}, {"focal", "tversky"}),
    (LovaszLoss(), {"lovasz", "class_lovasz"}, {"lovasz", "class_lovasz"}, {"lovasz"}),
    (LovaszLoss(base=RegionLoss()), {"lovasz", "class_lovasz", "focal", "tversky"}, {"lovasz", "class_lovasz", "focal", "tversky"},
     {"lovasz", "focal", "tversky"}),
    (OhemCE(), {"ce_all", "ohem_theta", "ohem_kept"}, {"ce_all", "ohem_theta", "ohem_kept"}, {"ce_all", "ohem_theta", "ohem_kept"}),
]
FEATURE_PARTS = {type(None): ("mse_cam", "mse_lidar"), ChannelKD: ("cwd_cam", "cwd_lidar"), PairKD: ("pair_cam", "pair_lidar"),
                 IntraClassKD: ("ifv_cam", "ifv_lidar")}


def test_every_accepted_class_and_none_has_a_row():
    assert HARD_LOSSES == (RegionLoss, LovaszLoss, OhemCE) and set(HARD_SPECS) == set(HARD_LOSSES)
    assert FEATURE_LOSSES == (ChannelKD, PairKD, IntraClassKD) and set(FEATURE_SPECS) == set(FEATURE_LOSSES)
    assert set(losses._HARD_TERMS) == set(HARD_LOSSES) | {type(None)}
    assert set(losses._FEATURE_TERMS) == set(FEATURE_LOSSES) | {type(None)}
    for table, specs, what in ((losses._HARD_TERMS, HARD_SPECS, "hard_loss"), (losses._FEATURE_TERMS, FEATURE_SPECS, "feature_loss")):
        for cls, spec in {type(None): None, **specs}.items():
            assert losses._term(table, what, spec) is table[cls]


@pytest.mark.parametrize("spec,function,autograd,fused", HARD_PARTS, ids=lambda v: None if isinstance(v, set) else repr(v)[:40])
def test_hard_rows_name_the_documented_parts(spec, function, autograd, fused):
    term = losses._term(losses._HARD_TERMS, "hard_loss", spec)
    for form, want in (("function", function), ("autograd", autograd), ("fused", fused)):
        got = term.names(spec, form)
        assert set(got) == want and len(got) == len(want), (form, got)
    # every part lies inside the buffer it names, per-class vectors with all of the row's classes
    for name, part in term.parts.items():
        assert part.at + (losses.HARD_MAX_NC if part.per_class else 1) <= term.sizes[part.buf], name
    assert term.max_nc == (losses.HARD_MAX_NC if isinstance(spec, (RegionLoss, LovaszLoss)) else None)
    assert term.zeroed == isinstance(spec, LovaszLoss)


def test_feature_rows_name_the_documented_parts():
    for cls, names in FEATURE_PARTS.items():
        assert losses._FEATURE_TERMS[cls].parts == names
    doc = losses.kd_objective.__doc__
    for names in FEATURE_PARTS.values():
        for name in names:
            assert f'"{name}"' in doc
    for _, function, _, _ in HARD_PARTS:
        for name in function - {"class_ti"}:                          # class_ti: region_seg_loss alone
            assert f'"{name}"' in doc


def test_checks_accept_every_member_and_none_and_name_every_class_otherwise():
    for spec in (None, *HARD_SPECS.values(), LovaszLoss(base=RegionLoss())):
        check_hard_loss(spec)
    for spec in (None, *FEATURE_SPECS.values()):
        check_feature_loss(spec)
    for bad in (object(), "ohem", ChannelKD()):
        with pytest.raises(ValueError, match="hard_loss.*RegionLoss.*LovaszLoss.*OhemCE.*None.*got " + type(bad).__name__):
            check_hard_loss(bad)
    for bad in (object(), "cwd", RegionLoss()):
        with pytest.raises(ValueError, match="feature_loss.*ChannelKD.*PairKD.*IntraClassKD.*None.*got " + type(bad).__name__):
            check_feature_loss(bad)


def _message(fn, *a, **kw):
    with pytest.raises(ValueError) as err:
        fn(*a, **kw)
    return str(err.value)


def test_step_and_trainers_refuse_with_the_same_message(tmp_path):
    """the refusals come before the constructors touch their model, optimiser or loaders, so placeholders do"""
    from kdrt.kd import KDStep
    from src.training.trainer import KDTrainer, Trainer
    bad = object()
    hard = _message(check_hard_loss, bad)
    feature = _message(check_feature_loss, bad)
    assert _message(KDStep, None, None, None, hard_loss=bad) == hard
    assert _message(KDStep, None, None, None, feature_loss=bad) == feature
    assert _message(Trainer, None, None, None, "cpu", save_dir=str(tmp_path), hard_loss=bad) == hard
    assert _message(KDTrainer, None, None, None, None, "cpu", save_dir=str(tmp_path), hard_loss=bad) == hard
    assert _message(KDTrainer, None, None, None, None, "cpu", save_dir=str(tmp_path), feature_loss=bad) == feature


def test_class_limit_is_the_rows():
    from kdrt import KDError
    for spec in (RegionLoss(), LovaszLoss(), LovaszLoss(base=RegionLoss())):
        losses.check_hard_classes(spec, 4)
        with pytest.raises(KDError, match=type(spec).__name__ + ": at most 4 classes"):
            losses.check_hard_classes(spec, 5)
    for spec in (None, OhemCE()):
        losses.check_hard_classes(spec, 16)
