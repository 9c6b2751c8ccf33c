"""GPU tests of the Pillow-exact bilinear resize (kd_image_resize_bilinear_batch) and of the loader's `device_resize`
mode.  No tolerances: every comparison is equality of bytes -- against the numpy model (tests/_pil_resample_ref.py),
against Pillow where it imports, against kd_image_u8hwc_to_f32chw_batch over the resized bytes for the float output,
and against the host-resize loader for `__getitem__`, `prepare_batch` and `DeviceBatchLoader(prefetch=1)`."""
import functools

import numpy as np
import pytest
import torch

import _pil_resample_ref as R

pytestmark = pytest.mark.gpu

try:
    from PIL import Image
except ImportError:                                   # the model is the yardstick then
    Image = None


def _pillow(a, H, W):
    return np.asarray(Image.fromarray(a).resize((W, H), Image.BILINEAR))


@functools.lru_cache(maxsize=None)
def _want(seed, src, dst, kind="random"):
    """(source frame, expected bytes): computed once per case, shared, read-only.  The model and Pillow must agree."""
    if kind == "random":
        a = R.frame(seed, *src)
    elif kind == "checker":
        yy, xx = np.mgrid[:src[0], :src[1]]
        a = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    else:
        a = np.full(src + (3,), int(kind), np.uint8)
    want = R.resize_bilinear(a, *dst)
    if Image is not None:
        assert np.array_equal(want, _pillow(a, *dst))
    a.setflags(write=False)
    want.setflags(write=False)
    return a, want


def _gpu(frames, dst, want_f32=True, want_u8=True, fill=None):
    """The entry point through the C ABI -> (float32 [B,3,H,W] tensor or None, uint8 [B,H,W,3] numpy or None)."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    from kdrt.resample import device_tables
    t = torch.from_numpy(np.stack(frames)).cuda()
    B, Hs, Ws = t.shape[:3]
    H, W = dst
    f = torch.full((B, 3, H, W), -1.0, dtype=torch.float32, device="cuda") if want_f32 else None
    u = torch.full((B, H, W, 3), 77, dtype=torch.uint8, device="cuda") if want_u8 else None
    assert lib.kd_image_resize_bilinear_supported(Hs, Ws, H, W) == 1
    (hb, hk), (vb, vk) = device_tables(Ws, W), device_tables(Hs, H)
    lib.call("kd_image_resize_bilinear_batch", P(t), P(hb), P(hk), hk.shape[1], P(vb), P(vk), vk.shape[1], P(f), P(u),
             B, Hs, Ws, H, W, stream())
    torch.cuda.synchronize()
    return f, (u.cpu().numpy() if want_u8 else None)


def _f32_of_bytes(u8_bhwc):
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    t = torch.from_numpy(np.ascontiguousarray(u8_bhwc)).cuda()
    B, H, W = t.shape[:3]
    out = torch.empty(B, 3, H, W, dtype=torch.float32, device="cuda")
    lib.call("kd_image_u8hwc_to_f32chw_batch", P(t), P(out), B, H, W, stream())
    return out


_CASES = R.SMALL_PAIRS + [((35, 45), (20, 300))]       # + more than one column tile, ragged: 300 = 256 + 44


@pytest.mark.parametrize("src,dst", _CASES, ids=[f"{s[0]}x{s[1]}-{t[0]}x{t[1]}" for s, t in _CASES])
def test_kernel_equals_model_and_pillow(src, dst):
    """Small pairs: both outputs; the byte output alone and the float output alone give the same bits.  Sources of
    37x53, 33x33, 9x11, 35x45: row pitches that are no multiple of 16 bytes (the edge chunks of every staged row)."""
    a, want = _want(3, src, dst)
    f, u = _gpu([a], dst)
    assert np.array_equal(u[0], want), int((u[0] != want).sum())
    assert torch.equal(f, _f32_of_bytes(want[None]))
    _, u_only = _gpu([a], dst, want_f32=False)
    f_only, _ = _gpu([a], dst, want_u8=False)
    assert np.array_equal(u_only, u) and torch.equal(f_only, f)


def test_real_scale_batch_of_three_and_batch_versus_per_frame():
    """(270, 480) -> (36, 64): the real scale of 7.5 per axis, five bands of 8 rows (the last one ragged) per frame;
    B = 3 different frames; frame b of the batch has the bits of the same frame resized alone."""
    src, dst = (270, 480), (36, 64)
    pairs = [_want(seed, src, dst) for seed in (1, 2, 3)]
    f, u = _gpu([p[0] for p in pairs], dst)
    for b, (a, want) in enumerate(pairs):
        assert np.array_equal(u[b], want), b
        f1, u1 = _gpu([a], dst)
        assert np.array_equal(u1[0], u[b]) and torch.equal(f1[0], f[b])
    assert torch.equal(f, _f32_of_bytes(np.stack([p[1] for p in pairs])))


def test_real_size_frame():
    (src, dst) = R.REAL
    a, want = _want(11, src, dst)
    f, u = _gpu([a], dst)
    assert np.array_equal(u[0], want), int((u[0] != want).sum())
    assert torch.equal(f, _f32_of_bytes(want[None]))


@pytest.mark.parametrize("kind", ["255", "0", "checker"])
def test_extreme_inputs(kind):
    """Rounding and the clip: all-255 must stay 255 (coefficient sums are 2^22 +- a few units), all-0 stays 0."""
    for src, dst in (((37, 53), (16, 24)), ((9, 11), (32, 40)), ((135, 240), (9, 16))):
        a, want = _want(0, src, dst, kind)
        if kind != "checker":
            assert (want == int(kind)).all()
        f, u = _gpu([a], dst)
        assert np.array_equal(u[0], want)
        assert torch.equal(f, _f32_of_bytes(want[None]))


def test_helper_and_non_contiguous_batch_positions():
    """resize_images_pil_bilinear, the function the loader calls: size is (width, height) as Pillow takes it."""
    from src.data_loading.pandaset_dataset import resize_images_pil_bilinear
    src, dst = (37, 53), (16, 24)
    pairs = [_want(seed, src, dst) for seed in (5, 6)]
    f, u = resize_images_pil_bilinear(np.stack([p[0] for p in pairs]), (dst[1], dst[0]), want_u8=True)
    assert f.shape == (2, 3, 16, 24) and u.shape == (2, 16, 24, 3)
    assert np.array_equal(u.cpu().numpy(), np.stack([p[1] for p in pairs]))
    assert torch.equal(f, resize_images_pil_bilinear(torch.from_numpy(np.stack([p[0] for p in pairs])), (24, 16)))
    assert torch.equal(f, _f32_of_bytes(u.cpu().numpy()))


def test_unsupported_shape_fails_loudly_and_writes_nothing():
    from kdrt.lib import KDError, lib
    from kdrt.ops import P, stream
    from kdrt.resample import device_tables
    from src.data_loading.pandaset_dataset import resize_images_pil_bilinear
    assert lib.kd_image_resize_bilinear_supported(17, 300, 8, 8) == 0          # 300 -> 8: a factor of 37.5
    assert lib.kd_image_resize_bilinear_supported(4097, 64, 512, 64) == 0
    assert lib.kd_image_resize_bilinear_supported(1080, 1920, 256, 256) == 1
    t = torch.zeros(1, 17, 300, 3, dtype=torch.uint8, device="cuda")
    f = torch.full((1, 3, 8, 8), -1.0, device="cuda")
    u = torch.full((1, 8, 8, 3), 77, dtype=torch.uint8, device="cuda")
    (hb, hk), (vb, vk) = device_tables(300, 8), device_tables(17, 8)
    with pytest.raises(KDError, match="supported range"):
        lib.call("kd_image_resize_bilinear_batch", P(t), P(hb), P(hk), hk.shape[1], P(vb), P(vk), vk.shape[1], P(f), P(u),
                 1, 17, 300, 8, 8, stream())
    torch.cuda.synchronize()
    assert (f == -1.0).all() and (u == 77).all()
    with pytest.raises(KDError):
        resize_images_pil_bilinear(t, (8, 8))


# ---- loader ----------------------------------------------------------------------------------------------------------
def _write_tree(root, n_frames=5, size=(135, 240)):
    """A PandaSet-shaped tree with full-size-ish JPEGs (tests/_fake_pandaset.py writes 37 x 53 ones)."""
    import os

    import pandas as pd
    from PIL import Image
    from _fake_pandaset import frame_arrays
    cam, lid, seg = (os.path.join(root, "001", *p) for p in (("camera", "front_camera"), ("lidar",), ("annotations", "semseg")))
    for d in (cam, lid, seg):
        os.makedirs(d)
    for k in range(n_frames):
        x, y, z, inten, cls, _ = frame_arrays(2000 + k, (300, 700, 64)[k % 3])
        Image.fromarray(R.frame(k, *size)).save(os.path.join(cam, f"{k:02d}.jpg"), quality=92)
        pd.DataFrame({"x": x, "y": y, "z": z, "i": inten}).to_pickle(os.path.join(lid, f"{k:02d}.pkl"))
        pd.DataFrame({"class": cls}).to_pickle(os.path.join(seg, f"{k:02d}.pkl"))
    return ["001"]


def _same_sample(a, b):
    assert a["sample_token"] == b["sample_token"]
    assert a["image"].shape == b["image"].shape and torch.equal(a["image"], b["image"])
    assert torch.equal(a["segmentation"], b["segmentation"])
    assert np.array_equal(a["points"].cpu().numpy(), b["points"].cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize("image_size", [(32, 32), (48, 32)])
def test_loader_device_resize_equals_host_resize(tmp_path, image_size):
    """`device_resize=True` against today's path over the same JPEGs: `__getitem__`, `prepare_batch` and
    DeviceBatchLoader(prefetch=1) under one sample_seed and epoch.  (48, 32) = (width, height): a [3, 32, 48] image."""
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, PandaSetDataset
    scenes = _write_tree(str(tmp_path))
    mk = lambda flag: PandaSetDataset(str(tmp_path), scenes, image_size=image_size, max_points=800, verbose=False,
                                      device_resize=flag)
    host, dev = mk(False), mk(True)
    assert len(host) == len(dev) == 5
    raw = dev.load_raw(0)
    assert torch.is_tensor(raw["image_u8"]) and raw["image_u8"].dtype == torch.uint8 and tuple(raw["image_u8"].shape) == (135, 240, 3)
    assert host.load_raw(0)["image_u8"].shape == (image_size[1], image_size[0], 3)
    for i in range(len(host)):
        a, b = host[i], dev[i]
        assert tuple(b["image"].shape) == (3, image_size[1], image_size[0])
        _same_sample(a, b)
    raws = lambda ds: [ds.load_raw(i) for i in range(3)]
    _same_sample(host.prepare_batch(raws(host)), dev.prepare_batch(raws(dev)))

    def collect(ds, **kw):
        loader = DeviceBatchLoader(ds, batch_size=2, shuffle=False, num_workers=0, prefetch=1, sample_seed=9, **kw)
        loader.set_epoch(3)
        out = [{k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in b.items()} for b in loader]
        torch.cuda.synchronize()
        return out

    want, got = collect(host), collect(dev)
    assert len(want) == len(got) == 3
    for a, b in zip(want, got):
        _same_sample(a, b)
    for a, b in zip(want, collect(mk(False), device_resize=True)):            # the keyword on the loader itself
        _same_sample(a, b)


def test_synthetic_source_frames_both_modes():
    """SyntheticRawPandaSet(source_size=...): full-size frames under device_resize, Pillow-resized ones otherwise; the
    prepared batches agree (long sweeps: the device sampler under the same seed and epoch)."""
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, SyntheticRawPandaSet
    mk = lambda flag: SyntheticRawPandaSet(n_frames=5, sweep_points=[900, 300], image_size=(24, 16), max_points=512, seed=4,
                                           source_size=(53, 37), device_resize=flag)
    host, dev = mk(False), mk(True)
    assert tuple(dev.load_raw(1)["image_u8"].shape) == (37, 53, 3) and host.load_raw(1)["image_u8"].shape == (16, 24, 3)
    for pf in (0, 2):
        a = list(DeviceBatchLoader(host, batch_size=2, shuffle=False, num_workers=0, prefetch=pf, sample_seed=1))
        b = list(DeviceBatchLoader(dev, batch_size=2, shuffle=False, num_workers=0, prefetch=pf, sample_seed=1))
        torch.cuda.synchronize()
        assert len(a) == len(b) == 3
        for x, y in zip(a, b):
            if pf:
                _same_sample(x, y)
            else:
                assert torch.equal(x["image"], y["image"]) and torch.equal(x["segmentation"], y["segmentation"])
