"""The subset rule of kd_points_prepare_batch on the CPU, against its numpy mirror alone (tests/_input_batch_ref.py):
shape of the subset, what it depends on, and the statistics of the key generator.  The GPU parity of the kernel with
this mirror is tests/test_gpu_input_batched.py."""
import numpy as np

from _input_batch_ref import philox_keys, prepare_points_batch, select_indices

N, K, FRAMES, SEED = 1024, 256, 4096, 12345


def test_generator_known_answer():
    """Philox-4x32-10: the Random123 known-answer vector for a zero counter and a zero key (word 0)."""
    assert int(philox_keys(0, 0, 1)[0]) == 0x6627E8D5
    k = philox_keys(SEED, 7, 5)
    assert k.dtype == np.uint32 and k.shape == (5,) and len(set(k.tolist())) == 5
    assert np.array_equal(k, philox_keys(SEED, 7, 9)[:5])                  # a key depends on (seed, frame_key, j) only


def test_subset_shape_and_order():
    for n, k in ((1000, 256), (257, 256), (169000, 5000), (169000, 80000)):
        idx = select_indices(SEED, 3, n, k)
        assert idx.dtype == np.int64 and idx.shape == (k,)
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n    # distinct, ascending, in range
    assert np.array_equal(select_indices(SEED, 3, 256, 256), np.arange(256))
    assert np.array_equal(select_indices(SEED, 3, 10, 256), np.arange(10))
    assert select_indices(SEED, 3, 0, 256).shape == (0,)


def test_subset_is_the_smallest_key_index_pairs():
    keys = philox_keys(SEED, 11, 3000)
    order = np.lexsort((np.arange(3000), keys))                            # by key, ties by index
    assert np.array_equal(select_indices(SEED, 11, 3000, 700), np.sort(order[:700]))


def test_subset_depends_on_seed_key_n_and_max_points_only():
    a = select_indices(SEED, 42, 5000, 1200)
    assert np.array_equal(a, select_indices(SEED, 42, 5000, 1200))
    assert not np.array_equal(a, select_indices(SEED + 1, 42, 5000, 1200))
    assert not np.array_equal(a, select_indices(SEED, 43, 5000, 1200))
    assert not np.array_equal(a, select_indices(SEED, 42 + (1 << 32), 5000, 1200))      # next epoch of the same frame
    assert not np.array_equal(a, select_indices(SEED + (1 << 32), 42, 5000, 1200))      # high seed word counts too
    # the point VALUES and the frames around it play no part: a frame's rows are the same alone and inside a batch
    r = np.random.RandomState(0)
    cols = [[r.randn(n).astype(np.float32) for n in (300, 5000, 0)] for _ in range(4)]
    batch = prepare_points_batch(*cols, 1200, SEED, [7, 42, 9])
    alone = prepare_points_batch(*[[c[1]] for c in cols], 1200, SEED, [42])
    assert np.array_equal(batch[1], alone[0]) and np.array_equal(batch[1, :, 0], cols[0][1][a])
    assert np.array_equal(batch[0, :300, 3], cols[3][0]) and not batch[0, 300:].any() and not batch[2].any()


def _counts():
    inc, pairs = np.zeros(N, np.int64), 0
    for fk in range(FRAMES):
        idx = select_indices(SEED, fk, N, K)
        inc[idx] += 1
        pairs += int(np.sum(np.diff(idx) == 1))
    return inc, pairs


def test_uniformity_and_adjacent_index_correlation():
    """n = 1024 -> 256 over frame keys 0..4095.  Every index is kept Binomial(4096, 1/4) times: mean 1024, sigma 27.7, and
    all 1024 counts must lie within 6 sigma (union bound ~2e-6; the test is deterministic anyway).  The pairs (j, j+1) kept
    together are held against p2 = (256/1024) * (255/1023) over 4096 * 1023 pairs with the same 6-sigma rule."""
    inc, pairs = _counts()
    p = K / N
    sigma = np.sqrt(FRAMES * p * (1 - p))
    dev = np.abs(inc - FRAMES * p).max()
    print(f"inclusion counts: largest deviation {dev} (6 sigma = {6 * sigma:.1f})")
    assert inc.sum() == FRAMES * K
    assert dev <= 6 * sigma
    p2 = p * (K - 1) / (N - 1)
    trials = FRAMES * (N - 1)
    sigma2 = np.sqrt(trials * p2 * (1 - p2))
    print(f"adjacent pairs kept together: {pairs}, expected {trials * p2:.0f} (6 sigma = {6 * sigma2:.0f})")
    assert abs(pairs - trials * p2) <= 6 * sigma2
