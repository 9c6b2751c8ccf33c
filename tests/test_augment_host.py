"""CPU tests of the augmentation's host side: the full Philox-4x32-10 of the numpy mirror (tests/_augment_ref.py) against
Random123's known answers and against the word-0 mirror of the subset sampler, Augment's parse form and range checks, and
kdrt.augment.frame_params -- a pure function of (settings, seed, frame key), inside its ranges, bit-equal to the mirror."""
import numpy as np
import pytest

import _augment_ref as R
from _input_batch_ref import philox_keys

SEED = 0x0BAD_5EED_1234_5678
ALL_ON = dict(rot_deg=20.0, scale=0.1, translate=2.0, flip=0.5, flip_axis="y", jitter=0.02, intensity=0.2, brightness=0.1,
              contrast=0.2, channel_gain=0.05, camera_drop=0.1)


def _keys(n, epoch=3):
    return [(epoch << 32) | i for i in range(n)]


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    from kdrt.augment import philox4x32_10
    for ctr, key, want in kat:
        assert " ".join(f"{int(v):08x}" for v in R.philox([ctr], key)[0]) == want
        assert " ".join(f"{int(v):08x}" for v in philox4x32_10(*ctr, *key)[0]) == want
    # word 0 against the existing mirror of the subset sampler (counter word 1 = 0)
    fk, n = (7 << 32) | 99, 1000
    ctr = [[j, 0, fk & 0xFFFFFFFF, fk >> 32] for j in range(n)]
    assert np.array_equal(R.philox(ctr, (SEED & 0xFFFFFFFF, SEED >> 32))[:, 0], philox_keys(SEED, fk, n))


def test_parse_round_trip_and_errors():
    from kdrt import KDError
    from kdrt.augment import Augment, as_augment
    a = Augment.parse("rot=5,flip=0.5,jitter=0.02")
    assert a == Augment(rot_deg=5.0, flip=0.5, jitter=0.02) and a.flip_axis == "y"
    full = Augment(**ALL_ON)
    for v in (a, full, Augment(flip=1.0, flip_axis="x"), Augment()):
        assert Augment.parse(v.to_string()) == v
    assert Augment.parse("") == Augment() and Augment.parse(" rot_deg = 5 , ") == Augment(rot_deg=5.0)
    assert as_augment(None) is None and as_augment("") is None and as_augment(Augment()) is None
    assert as_augment("flip=0.25") == Augment(flip=0.25)
    for bad in ("rotate=5", "rot", "rot=abc", "rot=5,rot_deg=6", "flip=1.5", "flip=-0.1", "rot=181", "scale=1", "jitter=-1",
                "flip_axis=z", "camera_drop=2", "brightness=nan", "contrast=1.01", "translate=inf"):
        with pytest.raises(KDError):
            Augment.parse(bad)
    with pytest.raises(KDError):
        Augment(channel_gain=-0.5)
    with pytest.raises(KDError):
        as_augment(5)


def test_all_off_is_the_identity_row():
    from kdrt.augment import Augment, frame_params
    rows = frame_params(Augment(), SEED, _keys(9))
    want = np.zeros(16, np.float32)
    want[[0, 2, 5, 6, 7, 8, 9, 10]] = 1.0           # c, scale, sx, sy, gi, a_r, a_g, a_b;  s, tx, ty, b, mirror = 0
    assert rows.dtype == np.float32 and rows.shape == (9, 16)
    assert np.array_equal(rows.view(np.uint32), np.tile(want, (9, 1)).view(np.uint32))
    assert not Augment().enabled


def test_row_depends_on_seed_and_key_only():
    from kdrt.augment import Augment, frame_params
    aug = Augment(**ALL_ON)
    key = (2 << 32) | 41
    batch_a = [key] + _keys(6)
    batch_b = _keys(6, epoch=9) + [key]
    ra, rb = frame_params(aug, SEED, batch_a), frame_params(aug, SEED, batch_b)
    assert np.array_equal(ra[0].view(np.uint32), rb[6].view(np.uint32))
    assert np.array_equal(ra[0].view(np.uint32), frame_params(aug, SEED, [key])[0].view(np.uint32))
    assert not np.array_equal(ra[0], frame_params(aug, SEED, [key + (1 << 32)])[0])        # another epoch word
    assert not np.array_equal(ra[0], frame_params(aug, SEED, [key + 1])[0])
    assert not np.array_equal(ra[0], frame_params(aug, SEED + 1, [key])[0])


def test_fields_stay_in_range_and_flags_agree():
    from kdrt.augment import Augment, frame_params
    for axis in ("x", "y"):
        aug = Augment(**{**ALL_ON, "flip_axis": axis})
        r = frame_params(aug, SEED, _keys(4096)).astype(np.float64)
        yaw = np.degrees(np.arctan2(r[:, 1], r[:, 0]))
        assert np.all(np.abs(yaw) <= 20.0 + 1e-4) and np.allclose(r[:, 0] ** 2 + r[:, 1] ** 2, 1.0, atol=1e-6)
        assert yaw.min() < -15 and yaw.max() > 15
        tol = 1e-6
        assert np.all(np.abs(r[:, 2] - 1.0) <= 0.1 + tol)
        assert np.all(np.abs(r[:, 3]) <= 2.0 + tol) and np.all(np.abs(r[:, 4]) <= 2.0 + tol)
        assert not np.array_equal(r[:, 3], r[:, 4])
        assert np.all(np.abs(r[:, 7] - 1.0) <= 0.2 + tol)
        flipped, fixed = (r[:, 5], r[:, 6]) if axis == "x" else (r[:, 6], r[:, 5])
        assert np.all(np.abs(flipped) == 1.0) and np.all(fixed == 1.0)
        assert np.array_equal(r[:, 12] == 1.0, flipped == -1.0) and np.all((r[:, 12] == 0.0) | (r[:, 12] == 1.0))
        count = int((flipped == -1.0).sum())
        assert abs(count - 2048) <= 160, count                                          # 5 sigma of Binomial(4096, 0.5)
        dropped = np.all(r[:, 8:12] == 0.0, axis=1)
        assert abs(int(dropped.sum()) - 410) <= 96, dropped.sum()                       # 5 sigma of Binomial(4096, 0.1)
        live = r[~dropped]
        assert np.all(live[:, 8:11] >= 0.8 * 0.95 - tol) and np.all(live[:, 8:11] <= 1.2 * 1.05 + tol)
        assert np.all(live[:, 11] >= 0.5 * (1 - 1.2) - 0.1 - tol) and np.all(live[:, 11] <= 0.5 * (1 - 0.8) + 0.1 + tol)
        assert np.all(r[:, 13:] == 0.0)


def test_camera_drop_one_zeroes_gains_and_offset():
    from kdrt.augment import Augment, frame_params
    r = frame_params(Augment(**{**ALL_ON, "camera_drop": 1.0}), SEED, _keys(64))
    assert np.all(r[:, 8:12] == 0.0) and np.all(r[:, 2] > 0.0)
    r = frame_params(Augment(flip=1.0, flip_axis="x"), SEED, _keys(64))
    assert np.all(r[:, 5] == -1.0) and np.all(r[:, 6] == 1.0) and np.all(r[:, 12] == 1.0)


@pytest.mark.parametrize("settings", [ALL_ON, {**ALL_ON, "flip_axis": "x", "rot_deg": 180.0}, dict(rot_deg=180.0), dict(flip=0.3),
                                      dict(camera_drop=0.5, brightness=1.0), {}])
def test_frame_params_equals_the_mirror(settings):
    from kdrt.augment import Augment, frame_params, rows_from_values
    aug = Augment(**settings)
    keys = _keys(257) + [0, 0xFFFFFFFFFFFFFFFF, (5 << 32) | 0xFFFFFFFF]
    for seed in (0, SEED):
        assert np.array_equal(frame_params(aug, seed, keys).view(np.uint32), R.frame_rows(aug, seed, keys).view(np.uint32))
    # a chosen transform: exact at the multiples of 90 degrees
    for deg, (c, s) in ((0.0, (1, 0)), (90.0, (0, 1)), (180.0, (-1, 0)), (-180.0, (-1, 0)), (-90.0, (0, -1))):
        row = rows_from_values(aug, deg, 1.0, 0.0, 0.0, False, 1.0, 0.0, 1.0, [1.0, 1.0, 1.0], False)[0]
        assert (row[0], row[1]) == (c, s)
        assert np.array_equal(row.view(np.uint32), R.make_row(aug, yaw_deg=deg).view(np.uint32))
