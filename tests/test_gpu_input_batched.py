"""GPU tests of the batched input preparation: kd_image_u8hwc_to_f32chw_batch and kd_points_prepare_batch through the
C ABI (bit-exact against the per-frame kernels and against the numpy mirror of the device sampler,
tests/_input_batch_ref.py), and DeviceBatchLoader(prefetch >= 1) against the synchronous loader over the same frames."""
import numpy as np
import pytest
import torch

from _input_batch_ref import prepare_points_batch, select_indices

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC


def _frame(r, n, nan=False, const=None):
    if const is not None:
        cols = [np.full(n, const, np.float32) for _ in range(4)]
    else:
        cols = [r.randn(n).astype(np.float32) * s for s in (40.0, 40.0, 4.0, 1.0)]
    if nan and n >= 3:
        cols[0][0], cols[1][2], cols[2][1] = np.nan, np.nan, np.nan
    return cols


def _gpu_points_batch(frames, max_points, seed, keys):
    """kd_points_prepare_batch through the C ABI -> numpy [B, max_points, 4]."""
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    B = len(frames)
    cat = [torch.from_numpy(np.concatenate([f[c] for f in frames])).cuda() for c in range(4)]
    lens = [len(f[0]) for f in frames]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    fk = torch.from_numpy(np.asarray(keys, np.uint64).view(np.int64)).cuda()
    out = torch.full((B, max_points, 4), 7.0, dtype=torch.float32, device="cuda")       # every row must be written
    lib.call("kd_points_prepare_batch", P(cat[0]), P(cat[1]), P(cat[2]), P(cat[3]), P(off), P(fk), B, sum(lens), max_points,
             seed, P(out), stream())
    return out.cpu().numpy()


def _ref_points_batch(frames, max_points, seed, keys):
    return prepare_points_batch(*[[f[c] for f in frames] for c in range(4)], max_points, seed, keys)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_batched_image_kernel_equals_per_frame_kernel(B):
    from kdrt.lib import lib
    from kdrt.ops import P, stream
    from src.data_loading.pandaset_dataset import image_to_chw
    r = np.random.RandomState(B)
    allv = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)      # every byte value: x / 255 as numpy rounds it
    pool = [allv, r.randint(0, 256, (16, 16, 3)).astype(np.uint8), np.zeros((16, 16, 3), np.uint8),
            np.full((16, 16, 3), 255, np.uint8), allv[::-1].copy(), r.randint(0, 2, (16, 16, 3)).astype(np.uint8),
            r.randint(0, 256, (16, 16, 3)).astype(np.uint8), allv.transpose(1, 0, 2).copy()]
    for imgs in (pool[:B], [r.randint(0, 256, (37, 53, 3)).astype(np.uint8) for _ in range(B)]):
        H, W = imgs[0].shape[:2]
        t = torch.from_numpy(np.stack(imgs)).cuda()
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device="cuda")
        lib.call("kd_image_u8hwc_to_f32chw_batch", P(t), P(out), B, H, W, stream())
        for b in range(B):
            one = image_to_chw(imgs[b])
            assert torch.equal(out[b], one)
            assert np.array_equal(one.cpu().numpy(), imgs[b].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0))


def test_padded_frames_equal_per_frame_kernel():
    """n <= max_points (n = 0, n = max_points, NaN rows), mixed in one batch with long frames: the bits of prepare_points."""
    from src.data_loading.pandaset_dataset import prepare_points
    r = np.random.RandomState(5)
    K = 256
    frames = [_frame(r, 1000), _frame(r, 0), _frame(r, K), _frame(r, 300, nan=True), _frame(r, 4000), _frame(r, 5),
              _frame(r, K - 1, nan=True)]
    got = _gpu_points_batch(frames, K, SEED, list(range(len(frames))))
    for b, f in enumerate(frames):
        if len(f[0]) <= K:
            assert np.array_equal(got[b], prepare_points(*f, K).cpu().numpy(), equal_nan=True), b
    assert np.array_equal(got, _ref_points_batch(frames, K, SEED, list(range(len(frames)))), equal_nan=True)


@pytest.mark.parametrize("n,K", [(1000, 256), (169000, 5000), (169000, 80000)])
def test_subsampled_frames_equal_the_mirror(n, K):
    """n > max_points: the rows the numpy mirror selects, bit for bit, in ascending source index -- and the same rows
    whether the frame is prepared alone, first or last in a batch of 7."""
    r = np.random.RandomState(n + K)
    f = _frame(r, n)
    f[0][:5] = np.nan                                                        # NaN coordinates are points like any other
    key = (3 << 32) | 17
    want = _ref_points_batch([f], K, SEED, [key])[0]
    idx = select_indices(SEED, key, n, K)
    assert np.array_equal(want[:, 3], f[3][idx])
    alone = _gpu_points_batch([f], K, SEED, [key])[0]
    assert np.array_equal(alone, want, equal_nan=True)
    others = [_frame(r, m) for m in (K + 1, 0, 300, 2 * K + 7, K, n // 3 + 1)]
    okeys = [100 + i for i in range(6)]
    first = _gpu_points_batch([f] + others, K, SEED, [key] + okeys)
    last = _gpu_points_batch(others + [f], K, SEED, okeys + [key])
    assert np.array_equal(first[0], want, equal_nan=True) and np.array_equal(last[6], want, equal_nan=True)
    assert np.array_equal(first[1:], last[:6])
    assert np.array_equal(first[1:], _ref_points_batch(others, K, SEED, okeys))
    # another seed / frame key: another subset
    assert not np.array_equal(_gpu_points_batch([f], K, SEED + 1, [key])[0], want, equal_nan=True)
    assert not np.array_equal(_gpu_points_batch([f], K, SEED, [key + (1 << 32)])[0], want, equal_nan=True)


def test_many_duplicate_values_still_give_max_points_rows():
    """All points equal in value (ties in value, not in key): still exactly max_points rows, none left as padding."""
    for n, K in ((1000, 256), (169000, 5000)):
        f = _frame(None, n, const=2.5)
        got = _gpu_points_batch([f, f], K, SEED, [1, 2])
        assert np.array_equal(got, np.full((2, K, 4), 2.5, np.float32))
        f[3] = np.arange(n, dtype=np.float32)                                # the index rides in the intensity column
        got = _gpu_points_batch([f], K, SEED, [9])[0]
        assert np.array_equal(got[:, 3].astype(np.int64), select_indices(SEED, 9, n, K))


# ---- loader ----------------------------------------------------------------------------------------------------------
def _collect(loader):
    out = []
    for b in loader:
        out.append({k: (v.clone() if torch.is_tensor(v) else list(v)) for k, v in b.items()})
    torch.cuda.synchronize()
    return out


def _same(a, b, points=True):
    assert len(a) == len(b) and len(a) > 0
    for x, y in zip(a, b):
        assert x["sample_token"] == y["sample_token"]
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["segmentation"], y["segmentation"])
        if points:
            assert x["points"].shape == y["points"].shape
            assert np.array_equal(x["points"].cpu().numpy(), y["points"].cpu().numpy(), equal_nan=True)


def _synthetic(max_points, sweeps, n_frames=7, **kw):
    from src.data_loading.pandaset_dataset import SyntheticRawPandaSet
    return SyntheticRawPandaSet(n_frames=n_frames, sweep_points=sweeps, image_size=(64, 48), max_points=max_points, seed=3, **kw)


@pytest.mark.parametrize("source", ["synthetic", "fake_tree"])
@pytest.mark.parametrize("workers,rank,world", [(0, 0, 1), (2, 0, 1), (0, 1, 2)])
def test_prefetching_loader_equals_synchronous_loader_without_sampling(tmp_path, source, workers, rank, world):
    """Sweeps no longer than max_points (no sampling): tokens, images, points and segmentation bit-identical batch by
    batch, ragged last batch included."""
    from _fake_pandaset import write_tree
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, PandaSetDataset
    if source == "synthetic":
        ds = _synthetic(800, [300, 700, 64, 0, 800], nan_frames=[0, 4])
    else:
        scenes = write_tree(str(tmp_path), scenes=("001", "002", "003"), frames_per_scene=3)
        ds = PandaSetDataset(str(tmp_path), scenes, max_points=800, verbose=False)
        assert len(ds) == 9
    mk = lambda pf: DeviceBatchLoader(ds, batch_size=2, shuffle=False, num_workers=workers, rank=rank, world=world,
                                      train=False, prefetch=pf)
    want, got = _collect(mk(0)), _collect(mk(2))
    assert sum(len(b["sample_token"]) for b in want) == len(range(rank, len(ds), world))
    if world == 1 or source == "synthetic":                                   # 7 or 9 frames, or frames 1, 3, 5 of 7
        assert len(want[-1]["sample_token"]) == 1                             # the ragged last batch
    _same(got, want)
    _same(_collect(mk(1)), want)


def test_prefetching_loader_long_sweeps_follow_the_mirror():
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, _RawFrames
    K = 1024
    ds = _synthetic(K, [6000, 300, 9000, K, 2500], n_frames=7, nan_frames=[2])
    want = _collect(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=0))
    seed = 77

    def expected(epoch):
        raws = [_RawFrames(ds)[i] for i in range(len(ds))]
        pts = _ref_points_batch([[r[c] for c in "xyzi"] for r in raws], K, seed, [(epoch << 32) | i for i in range(len(ds))])
        return [pts[i:i + 3] for i in range(0, len(ds), 3)]

    def check(batches, epoch):
        _same(batches, want, points=False)
        for b, e in zip(batches, expected(epoch)):
            assert np.array_equal(b["points"].cpu().numpy(), e, equal_nan=True)

    loader = DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=2, sample_seed=seed)
    e0, e1 = _collect(loader), _collect(loader)
    check(e0, 0)
    check(e1, 1)                                                               # one epoch per __iter__ ...
    assert not torch.equal(e0[0]["points"], e1[0]["points"])
    loader.set_epoch(5)                                                        # ... unless the trainer names it
    check(_collect(loader), 5)
    again = _collect(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=1, sample_seed=seed))
    check(again, 0)
    other = _collect(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=1, sample_seed=seed + 1))
    assert not torch.equal(other[0]["points"], e0[0]["points"])
    cpu = next(iter(DeviceBatchLoader(ds, batch_size=3, shuffle=False, num_workers=0, prefetch=2, sample_seed=seed, to_cpu=True)))
    assert not cpu["points"].is_cuda and np.array_equal(cpu["points"].numpy(), e0[0]["points"].cpu().numpy(), equal_nan=True)


def test_prefetched_batches_are_safe_on_the_consumer_stream():
    """Each prefetched batch is consumed at once by kernels on the current stream while the next one is being prepared
    on the side stream and an unrelated user fills the shared workspace on the compute stream.  No timing involved: the
    results must equal the synchronous loader's.  Then: break after the first batch, iterate again, compare again."""
    from kdrt import ops
    from src.data_loading.pandaset_dataset import DeviceBatchLoader, rasterize_bev_batch
    K = 20000
    ds = _synthetic(K, [20000, 15000, 18000, 0, 19999], n_frames=24, unique=5)
    want = _collect(DeviceBatchLoader(ds, batch_size=4, shuffle=False, num_workers=0, prefetch=0))
    dev = torch.device("cuda", torch.cuda.current_device())
    r = np.random.RandomState(0)
    bx, by = (r.randn(169000) * 40).astype(np.float32), (r.randn(169000) * 40).astype(np.float32)
    bc = r.randint(0, 43, 169000).astype(np.int64)
    big_want = rasterize_bev_batch([bx] * 4, [by] * 4, [bc] * 4, remap=True).clone()

    def consume(b):
        sums = (b["points"].nan_to_num().double().sum(), b["image"].double().sum(), b["segmentation"].sum())
        ops.workspace(1 << 26, dev).zero_()                                   # a claim table zeroed mid-flight would show
        big = rasterize_bev_batch([bx] * 4, [by] * 4, [bc] * 4, remap=True)
        return sums, big, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()}

    def check(results, ref):
        torch.cuda.synchronize()
        for (sums, big, got), w in zip(results, ref):
            _same([got], [w])
            assert torch.equal(big, big_want)
            assert sums[0].item() == w["points"].nan_to_num().double().sum().item()
            assert sums[1].item() == w["image"].double().sum().item() and sums[2].item() == w["segmentation"].sum().item()

    loader = DeviceBatchLoader(ds, batch_size=4, shuffle=False, num_workers=0, prefetch=2)
    first = []
    for b in loader:
        first.append(consume(b))
        break                                                                  # leaves two prepared batches behind
    check(first, want[:1])
    full = [consume(b) for b in loader]
    assert len(full) == len(want) == 6
    check(full, want)
    with pytest.raises(RuntimeError, match="stop here"):
        for k, b in enumerate(loader):
            if k == 1:
                raise RuntimeError("stop here")
    check([consume(b) for b in loader], want)


def test_trainer_over_the_prefetching_loader_repeats_the_synchronous_run(tmp_path):
    """Trainer.train_epoch() + validate() as in test_trainer_consumes_device_loader; sweeps shorter than max_points and a
    fixed torch seed: same batches, same step, so the epoch loss equals the prefetch = 0 run bit for bit."""
    from _fake_pandaset import write_tree
    from _gpu_util import build_product
    from src.data_loading.pandaset_dataset import create_pandaset_dataloaders
    from src.training.trainer import Trainer
    scenes = write_tree(str(tmp_path / "data"), n_points=(3000, 700), degenerate=False)

    def run(prefetch, tag):
        tl, vl = create_pandaset_dataloaders(str(tmp_path / "data"), scenes, scenes, batch_size=2, num_workers=0, verbose=False,
                                             prefetch=prefetch)
        assert tl.prefetch == vl.prefetch == prefetch
        torch.manual_seed(0)
        tr = Trainer(build_product("weighted", 64), tl, vl, torch.device("cuda"), save_dir=str(tmp_path / tag),
                     class_weights=[0.4, 3.5], num_epochs=2)
        loss, m = tr.train_epoch()
        vloss, vm = tr.validate()
        assert np.isfinite(loss) and np.isfinite(vloss) and 0.0 <= vm["miou"] <= 1.0
        return loss, vloss, vm["miou"]

    base, pre = run(0, "ck0"), run(2, "ck2")
    print("prefetch=0:", base, "prefetch=2:", pre)
    assert pre == base
