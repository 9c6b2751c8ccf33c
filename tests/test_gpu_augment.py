"""GPU tests of the opt-in training augmentation: kd_points_augment_batch and kd_image_augment_batch through the C ABI,
bit for bit against the numpy mirror (tests/_augment_ref.py); BEV labels that follow the augmented points (the project's
host rasteriser over the mirror's coordinates, exact equality); DeviceBatchLoader(augment=...) on both of its paths; one
Trainer epoch over an augmented loader."""
import numpy as np
import pytest
import torch

import _augment_ref as R
import data_oracle as D
from _input_batch_ref import select_indices

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC
ALL_ON = dict(rot_deg=20.0, scale=0.1, translate=2.0, flip=0.5, flip_axis="y", jitter=0.02, intensity=0.2, brightness=0.1,
              contrast=0.2, channel_gain=0.05, camera_drop=0.1)
LENS = (0, 1, 63, 1000, 4097)                     # + one frame with NaN rows and one on the range's border, see _frames()


def _aug(**kw):
    from kdrt.augment import Augment
    return Augment(**kw)


_FRAMES = None


def _frames():
    """(frames, classes): 7 ragged frames as [x, y, z, i] float32 columns -- LENS, then 300 points with NaN rows, then 64
    points with coordinates exactly on -50 / +50 (and just inside / outside).  5525 points in all: not a multiple of 4.
    Built once and never written to."""
    global _FRAMES
    if _FRAMES is None:
        r = np.random.RandomState(11)
        frames = [[(r.randn(n) * s).astype(np.float32) for s in (30.0, 30.0, 4.0, 1.0)] for n in LENS + (300,)]
        f = frames[-1]
        f[0][0], f[1][2], f[2][1], f[3][5] = np.nan, np.nan, np.nan, np.nan
        f[0][7] = f[1][7] = np.nan
        edge = np.array([-50.0, 50.0, np.nextafter(np.float32(50), np.float32(0)), np.nextafter(np.float32(50), np.float32(99)),
                         np.nextafter(np.float32(-50), np.float32(0)), np.nextafter(np.float32(-50), np.float32(-99)), 0.0, -0.0],
                        np.float32)
        frames.append([np.tile(edge, 8), np.repeat(edge, 8), (r.randn(64) * 4).astype(np.float32), r.rand(64).astype(np.float32)])
        classes = [r.randint(0, 43, len(f[0])).astype(np.int64) for f in frames]
        for f in frames:
            for c in f:
                c.setflags(write=False)
        _FRAMES = (frames, classes)
    return _FRAMES


def _gpu_points(frames, rows, keys, seed, jitter, stride="aligned", keep_device=False):
    """kd_points_augment_batch through the C ABI over the packed columns of `frames` -> per-frame [x', y', z', i'].
    stride: "aligned" = columns 4 * ceil(n / 4) floats apart (16-byte accesses), "packed" = n floats apart."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    B, lens = len(frames), [len(f[0]) for f in frames]
    n = sum(lens)
    ns = -(-n // 4) * 4 if stride == "aligned" else n
    host = np.full(4 * ns + 8, 7.0, np.float32)                               # the slack after each column must stay as it is
    for c in range(4):
        host[c * ns:c * ns + n] = np.concatenate([f[c] for f in frames])
    cols = torch.from_numpy(host.copy()).cuda()
    bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    off = torch.from_numpy(bounds).cuda()
    fk = torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64)).cuda()
    prm = torch.from_numpy(np.ascontiguousarray(rows, np.float32)).cuda()
    v = [cols[c * ns:c * ns + n] for c in range(4)]
    lib.call("kd_points_augment_batch", P(v[0]), P(v[1]), P(v[2]), P(v[3]), P(off), P(fk), P(prm), B, n, seed, float(np.float32(jitter)),
             stream())
    out = cols.cpu().numpy()
    for c in range(4):                                                        # nothing outside the columns was written
        assert np.all(out[c * ns + n:(c + 1) * ns] == 7.0) and np.all(out[4 * ns:] == 7.0)
    per = [[out[c * ns + a:c * ns + b] for c in range(4)] for a, b in zip(bounds[:-1], bounds[1:])]
    return (per, v, off) if keep_device else per


def _check_frames(got, frames, rows, keys, seed, jitter):
    for b, (g, f) in enumerate(zip(got, frames)):
        want = R.augment_points(*f, rows[b], seed, keys[b], jitter)
        for c in range(4):
            assert R.same_bits(g[c], want[c]), (b, "xyzi"[c])


@pytest.mark.parametrize("stride", ["aligned", "packed"])
def test_points_kernel_equals_the_mirror_all_options_on(stride):
    frames, _ = _frames()
    aug = _aug(**ALL_ON)
    keys = [(2 << 32) | (10 + b) for b in range(len(frames))]
    rows = R.frame_rows(aug, SEED, keys)
    assert (rows[:, 6] == -1).any() and (rows[:, 6] == 1).any()               # flipped and unflipped frames in the batch
    got = _gpu_points(frames, rows, keys, SEED, aug.jitter, stride)
    _check_frames(got, frames, rows, keys, SEED, aug.jitter)
    assert np.isnan(got[5][0][0]) and np.isnan(got[5][1][2]) and not np.isnan(got[5][0][1])
    # each frame alone == inside the batch
    for b, f in enumerate(frames):
        alone = _gpu_points([f], rows[b:b + 1], keys[b:b + 1], SEED, aug.jitter, stride)[0]
        for c in range(4):
            assert R.same_bits(alone[c], got[b][c]) or len(f[0]) == 0, b
    # another key or seed: another jitter
    other = _gpu_points(frames[3:4], rows[3:4], [keys[3] + 1], SEED, aug.jitter, stride)[0]
    assert not np.array_equal(other[0], got[3][0]) and np.array_equal(other[3], got[3][3])


@pytest.mark.parametrize("stride", ["aligned", "packed"])
def test_points_kernel_without_jitter_is_the_jitter_free_formula(stride):
    frames, _ = _frames()
    aug = _aug(**{**ALL_ON, "jitter": 0.0})
    keys = list(range(100, 100 + len(frames)))
    rows = R.frame_rows(aug, SEED, keys)
    got = _gpu_points(frames, rows, keys, SEED, 0.0, stride)
    _check_frames(got, frames, rows, keys, SEED, 0.0)
    c, s, sc, tx, ty, sx, sy, gi = (np.float32(v) for v in rows[3][:8])       # spelled out once more for one frame
    x, y, z, i = frames[3]
    xf, yf = sx * x, sy * y
    assert R.same_bits(got[3][0], sc * (c * xf - s * yf) + tx) and R.same_bits(got[3][1], sc * (s * xf + c * yf) + ty)
    assert R.same_bits(got[3][2], sc * z) and R.same_bits(got[3][3], gi * i)
    ident = np.tile(R.make_row(aug), (len(frames), 1))                        # the identity row: the values stay
    same = _gpu_points(frames, ident, keys, SEED, 0.0, stride)
    _check_frames(same, frames, ident, keys, SEED, 0.0)
    for b in (1, 2, 3, 4):                                                    # (x, y: a negative zero leaves as +0; NaN-free frames)
        for c4 in range(4):
            assert R.same_bits(same[b][c4], frames[b][c4] + np.float32(0.0) if c4 < 2 else frames[b][c4])


def _device_raster(x, y, cls, off, B, grid, pc_range=(-50, 50, -50, 50)):
    from kdrt.lib import lib
    from kdrt.ops import P, stream, workspace
    from src.data_loading.pandaset_dataset import _DRIVABLE_BITS
    seg = torch.empty(B, grid[0], grid[1], dtype=torch.int64, device="cuda")
    nbytes = lib.kd_bev_rasterize_ws_bytes(B, grid[0], grid[1])
    ws = workspace(nbytes, seg.device)
    x0, x1, y0, y1 = (float(v) for v in pc_range)
    lib.call("kd_bev_rasterize", P(x), P(y), P(cls), P(off), B, x.numel(), 1, _DRIVABLE_BITS, grid[0], grid[1], x0, x1 - x0, x1, y0,
             y1 - y0, y1, P(ws), nbytes, P(seg), stream())
    return seg.cpu().numpy()


def test_labels_follow_the_points_and_a_half_turn_is_exact_negation():
    """Rasteriser over the device-augmented columns == host rasteriser over the mirror-augmented coordinates, exactly; then
    a row of exactly 180 degrees, everything else off: the kernel negates x and y exactly, so the pinned mask is the host
    rasteriser over (-x, -y)."""
    frames, classes = _frames()
    grid = (64, 64)
    cls = torch.from_numpy(np.concatenate(classes)).cuda()
    aug = _aug(**ALL_ON)
    keys = [(1 << 32) | b for b in range(len(frames))]
    rows = R.frame_rows(aug, SEED, keys)
    _, v, off = _gpu_points(frames, rows, keys, SEED, aug.jitter, keep_device=True)
    got = _device_raster(v[0], v[1], cls, off, len(frames), grid)
    plain = np.stack([D.rasterize_bev(f[0], f[1], D.remap_semantic(c), grid) for f, c in zip(frames, classes)])
    for b, (f, c) in enumerate(zip(frames, classes)):
        x, y, _, _ = R.augment_points(*f, rows[b], SEED, keys[b], aug.jitter)
        assert np.array_equal(got[b], D.rasterize_bev(x, y, D.remap_semantic(c), grid)), b
    assert not np.array_equal(got[4], plain[4])

    half = _aug(rot_deg=180.0)
    row = R.make_row(half, yaw_deg=180.0)
    assert row[0] == -1.0 and row[1] == 0.0
    per, v, off = _gpu_points(frames, np.tile(row, (len(frames), 1)), keys, SEED, 0.0, keep_device=True)
    got = _device_raster(v[0], v[1], cls, off, len(frames), grid)
    for b, (f, c) in enumerate(zip(frames, classes)):
        ok = ~(np.isnan(f[0]) | np.isnan(f[1]))                              # a NaN in x or y makes the pair NaN
        assert np.array_equal(per[b][0][ok], -f[0][ok]) and np.array_equal(per[b][1][ok], -f[1][ok]), b
        assert np.isnan(per[b][0][~ok]).all() and np.isnan(per[b][1][~ok]).all()
        assert R.same_bits(per[b][2], f[2]) and R.same_bits(per[b][3], f[3]), b
        assert np.array_equal(got[b], D.rasterize_bev(-f[0], -f[1], D.remap_semantic(c), grid)), b
    assert got[4].sum() > 0 and not np.array_equal(got[4], plain[4])


def _image_rows(mirror):
    aug = _aug(flip=1.0 if mirror else 0.0)
    rows = np.stack([R.make_row(aug, flipped=mirror, contrast=1.7, brightness=0.15, gains=(1.0, 0.4, 1.2)),     # both clamps
                     R.make_row(aug, flipped=mirror, dropped=True, contrast=1.3, brightness=0.2),              # camera drop
                     R.make_row(aug, flipped=mirror, brightness=0.3),
                     R.make_row(aug, flipped=mirror)])
    assert rows[0][11] < 0 and np.all(rows[1][8:12] == 0) and np.all(rows[:, 12] == (1.0 if mirror else 0.0))
    return rows


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("W", [1, 2, 7, 16, 53])
def test_image_kernel_equals_the_mirror(W, mirror):
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    H, rows = 37, _image_rows(mirror)
    B = len(rows)
    r = np.random.RandomState(W)
    n = B * 3 * H * W
    vals = np.concatenate([np.arange(256), r.randint(0, 256, max(n - 256, 0))])[:n]
    img = (r.permutation(vals).astype(np.float32) / np.float32(255.0)).reshape(B, 3, H, W)
    assert n < 256 or len(np.unique(img)) == 256                             # every byte value / 255 (W = 1, 2: most of them)
    img[0, :, 0, 0], img[0, :, H - 1, W - 1] = 0.0, 1.0                       # both ends in the frame whose row clamps
    t = torch.from_numpy(img).cuda()
    lib.call("kd_image_augment_batch", P(t), P(torch.from_numpy(rows).cuda()), B, H, W, stream())
    got = t.cpu().numpy()
    for b in range(B):
        want = R.augment_image(img[b], rows[b])
        assert np.array_equal(got[b].view(np.uint32), want.view(np.uint32)), b
    assert got[0].min() == 0.0 and got[0].max() == 1.0                       # both clamps were hit
    assert np.all(got[1] == 0.0)                                              # camera drop
    if mirror:
        assert np.array_equal(got[3], img[3][:, :, ::-1])
    else:
        assert np.array_equal(got[3], img[3])


# ---- loader ----------------------------------------------------------------------------------------------------------
def _collect(loader):
    out = []
    for b in loader:
        out.append({k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in b.items()})
    torch.cuda.synchronize()
    return out


def _synthetic(max_points, sweeps, n_frames=7, **kw):
    from src.data_loading.pandaset_dataset import SyntheticRawPandaSet
    return SyntheticRawPandaSet(n_frames=n_frames, sweep_points=sweeps, image_size=(64, 48), max_points=max_points, seed=3, **kw)


def _same_batches(a, b):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x["sample_token"] == y["sample_token"]
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["segmentation"], y["segmentation"])
        assert R.same_bits(x["points"].cpu().numpy(), y["points"].cpu().numpy())


def _check_against_mirror(batches, ds, aug, seed, epoch, bs):
    raws = [ds.load_raw(i) for i in range(len(ds))]
    for k, b in enumerate(batches):
        idx = list(range(k * bs, min((k + 1) * bs, len(ds))))
        img, pts, seg = R.pipeline([raws[i] for i in idx], aug, seed, [(epoch << 32) | i for i in idx], ds.max_points, ds.grid_size,
                                   ds.pc_range)
        assert np.array_equal(b["image"].cpu().numpy().view(np.uint32), img.view(np.uint32)), k
        assert R.same_bits(b["points"].cpu().numpy(), pts), k
        assert np.array_equal(b["segmentation"].cpu().numpy(), seg), k


@pytest.mark.parametrize("settings", [ALL_ON, dict(rot_deg=180.0)], ids=["all_on", "rot180_only"])
def test_loader_paths_agree_and_equal_the_mirror_pipeline(settings):
    """prefetch = 0 and prefetch = 2 give identical batches, equal to the mirror pipeline (segmentation = host rasteriser
    over the mirror-augmented x, y); epoch 1 differs from epoch 0; epoch 0 again is epoch 0."""
    from src.data_loading.pandaset_dataset import DeviceBatchLoader
    aug = _aug(**settings)
    ds = _synthetic(800, [300, 700, 64, 0, 800], nan_frames=[0, 4])
    mk = lambda pf: DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, train=True, prefetch=pf, sample_seed=SEED,
                                      augment=aug)
    sync, pre = mk(0), mk(2)
    s0, p0 = _collect(sync), _collect(pre)
    _same_batches(s0, p0)
    _check_against_mirror(p0, ds, aug, SEED, 0, 3)
    s1, p1 = _collect(sync), _collect(pre)                                    # one epoch per __iter__
    _same_batches(s1, p1)
    _check_against_mirror(p1, ds, aug, SEED, 1, 3)
    assert not torch.equal(p0[0]["points"], p1[0]["points"]) and not torch.equal(p0[0]["segmentation"], p1[0]["segmentation"])
    for loader in (sync, pre):
        loader.set_epoch(0)
        _same_batches(_collect(loader), p0)
    plain = _collect(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, train=True, prefetch=2, sample_seed=SEED))
    assert not torch.equal(plain[0]["segmentation"], p0[0]["segmentation"])
    if "brightness" in settings:
        assert not torch.equal(plain[0]["image"], p0[0]["image"])
    else:
        assert torch.equal(plain[0]["image"], p0[0]["image"])                 # no image setting on: the image keeps its bits


def test_augmentation_does_not_disturb_the_sampler():
    """A 169 000-point sweep cut to 5000 rows under augmentation: the source index rides in the intensity column (no
    intensity gain), and the kept indices are those of the subset sampler's existing mirror."""
    from src.data_loading.pandaset_dataset import DeviceBatchLoader
    n, K = 169000, 5000
    ds = _synthetic(K, [n, 300], n_frames=2)
    for i in range(2):
        ds.load_raw(i)
    ds._made[0]["i"] = np.arange(n, dtype=np.float32)
    aug = _aug(**{**ALL_ON, "intensity": 0.0})
    loader = DeviceBatchLoader(ds, batch_size=2, shuffle=False, num_workers=0, train=True, prefetch=1, sample_seed=SEED, augment=aug)
    loader.set_epoch(4)
    b = _collect(loader)[0]
    key = (4 << 32) | 0
    idx = select_indices(SEED, key, n, K)
    pts = b["points"][0].cpu().numpy()
    assert np.array_equal(pts[:, 3].astype(np.int64), idx)
    raw, row = ds.load_raw(0), R.frame_rows(aug, SEED, [key])[0]
    x, y, z, _ = R.augment_points(raw["x"], raw["y"], raw["z"], raw["i"], row, SEED, key, aug.jitter)
    assert R.same_bits(pts[:, :3], np.stack([x[idx], y[idx], z[idx]], axis=1))
    assert np.array_equal(b["segmentation"][0].cpu().numpy(), D.rasterize_bev(x, y, D.remap_semantic(raw["class"]), ds.grid_size))


@pytest.mark.parametrize("prefetch", [0, 2])
def test_loader_without_augment_keeps_its_bits(prefetch):
    """No augment argument: the batches are the plain preparation of the raw frames (host rasteriser, stack and pad,
    byte / 255), bit for bit, and no augmentation kernel's symbol is needed."""
    from src.data_loading.pandaset_dataset import DeviceBatchLoader
    ds = _synthetic(800, [300, 700, 64, 0, 800], nan_frames=[0, 4])
    got = _collect(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, train=True, prefetch=prefetch))
    raws = [ds.load_raw(i) for i in range(len(ds))]
    assert len(got) == 3
    for k, b in enumerate(got):
        for j, r in enumerate(raws[3 * k:3 * k + 3]):
            assert np.array_equal(b["image"][j].cpu().numpy(), D.image_to_chw(r["image_u8"]))
            assert np.array_equal(b["points"][j].cpu().numpy(), D.prepare_points(r["x"], r["y"], r["z"], r["i"], ds.max_points), equal_nan=True)
            assert np.array_equal(b["segmentation"][j].cpu().numpy(),
                                  D.rasterize_bev(r["x"], r["y"], D.remap_semantic(r["class"]), ds.grid_size, ds.pc_range))


def test_all_off_augment_is_off_and_validation_loaders_refuse():
    from kdrt import KDError
    from src.data_loading.pandaset_dataset import DeviceBatchLoader
    ds = _synthetic(800, [300, 700, 64, 0, 800], nan_frames=[0, 4])
    mk = lambda **kw: DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=1, **kw)
    off = mk(train=True, augment=_aug())
    assert off.augment is None
    _same_batches(_collect(off), _collect(mk(train=True)))
    assert mk(train=True, augment="flip=0.5,rot=3").augment == _aug(flip=0.5, rot_deg=3.0)
    for kw in (dict(train=False), dict()):                                    # shuffle=False alone also means validation
        with pytest.raises(KDError, match="training"):
            mk(augment=_aug(flip=0.5), **kw)
    with pytest.raises(KDError):
        mk(train=True, augment="spin=3")


def test_trainer_epoch_over_an_augmented_loader(tmp_path, monkeypatch, capsys):
    """create_pandaset_dataloaders hands KD_LOADER_AUGMENT to the training loader only; one Trainer epoch over 8 small
    augmented frames: 4 steps, finite loss."""
    from _fake_pandaset import write_tree
    from _gpu_util import build_product
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import Trainer
    scenes = write_tree(str(tmp_path / "data"), scenes=("001", "002"), frames_per_scene=4, n_points=(3000, 700), degenerate=False)
    monkeypatch.setenv("KD_LOADER_AUGMENT", "rot=10,scale=0.05,translate=1,flip=0.5,jitter=0.02,intensity=0.1,brightness=0.1,"
                                            "contrast=0.1,channel_gain=0.05,camera_drop=0.25")
    tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False, prefetch=1)
    assert tl.augment is not None and tl.augment.camera_drop == 0.25 and vl.augment is None
    assert len(tl.dataset) == 8
    torch.manual_seed(0)
    tr = Trainer(build_product("weighted", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / "ck"), class_weights=[0.4, 3.5],
                 num_epochs=1)
    steps, inner = [], tr._step

    def counted(imgs, pts, seg):
        steps.append((float(imgs.min()), float(imgs.max())))
        return inner(imgs, pts, seg)

    monkeypatch.setattr(tr, "_step", counted)
    loss, m = tr.train_epoch()
    assert len(steps) == 4 and np.isfinite(loss) and 0.0 <= m["miou"] <= 1.0
    assert all(lo >= 0.0 and hi <= 1.0 for lo, hi in steps)
    vloss, _ = tr.validate()
    assert np.isfinite(vloss)
    # the explicit argument wins over the environment; the synthetic fallback ignores the setting with one notice
    tl2, _ = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, verbose=False, augment="flip=1")
    assert tl2.augment.flip == 1.0 and tl2.augment.rot_deg == 0.0
    capsys.readouterr()
    create_pandaset_dataloaders(str(tmp_path / "nowhere"), scenes, scenes, batch_size=2, verbose=True)
    assert capsys.readouterr().out.count("augment setting is ignored") == 1
