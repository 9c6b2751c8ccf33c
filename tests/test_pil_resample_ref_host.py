"""Host tests of the Pillow-exact bilinear resize: the numpy model (tests/_pil_resample_ref.py) against Pillow itself,
byte for byte; the vertical-first mutant must differ (the comparison can tell the pass order); the product's
coefficient-table builder (kdrt/resample.py) against the model's tables."""
import numpy as np
import pytest

import _pil_resample_ref as R

_IDS = [f"{s[0]}x{s[1]}-{t[0]}x{t[1]}" for s, t in R.HOST_PAIRS]


def _pillow(a, H, W):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((W, H), Image.BILINEAR))


@pytest.mark.parametrize("src,dst", R.HOST_PAIRS, ids=_IDS)
def test_model_equals_pillow(src, dst):
    a = R.frame(src[0] * 7 + dst[1], *src)
    want = _pillow(a, *dst)
    assert want.shape == (dst[0], dst[1], 3)
    got = R.resize_bilinear(a, *dst)
    assert got.dtype == np.uint8 and np.array_equal(got, want), int((got != want).sum())


def test_vertical_first_mutant_differs_from_pillow():
    (src, dst) = R.REAL
    a = R.frame(11, *src)
    want = _pillow(a, *dst)
    assert np.array_equal(R.resize_bilinear(a, *dst), want)
    mutant = R.resize_bilinear(a, *dst, vertical_first=True)
    differing = int((mutant != want).sum())
    print(f"vertical-first differs from Pillow in {differing} of {want.size} bytes")
    assert differing > 0


@pytest.mark.parametrize("src,dst", R.HOST_PAIRS, ids=_IDS)
def test_product_tables_equal_the_model(src, dst):
    from kdrt.resample import pil_bilinear_tables
    for n_in, n_out in ((src[1], dst[1]), (src[0], dst[0])):
        bounds, k = pil_bilinear_tables(n_in, n_out)
        wb, wk = R.dense_tables(n_in, n_out)
        assert bounds.dtype == np.int32 and k.dtype == np.int32
        assert np.array_equal(bounds, wb) and np.array_equal(k, wk), (n_in, n_out)
        assert np.all(np.abs(k.astype(np.int64).sum(axis=1) - (1 << 22)) <= k.shape[1])       # rounding: half a unit per tap


def test_tap_counts_at_the_real_shape_and_the_identity_axis():
    from kdrt.resample import pil_bilinear_tables
    n = pil_bilinear_tables(1920, 256)[0][:, 1]
    assert n.min() >= 11 and n.max() <= 15
    n = pil_bilinear_tables(1080, 256)[0][:, 1]
    assert n.min() >= 6 and n.max() <= 9
    bounds, k = pil_bilinear_tables(33, 33)                                   # the pass Pillow skips: the identity
    assert np.array_equal(bounds[:, 0], np.arange(33)) and np.array_equal(k[:, 0], np.full(33, 1 << 22))
    assert not k[:, 1:].any()
