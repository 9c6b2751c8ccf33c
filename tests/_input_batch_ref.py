"""numpy mirror of the subset rule of kd_points_prepare_batch (include/kd_hip.h): every point index j of a frame gets
the 32-bit key  Philox-4x32-10(counter = (j, 0, frame_key lo, frame_key hi), key = (seed lo, seed hi))[word 0];  the
kept rows are the `max_points` smallest (key, j) pairs, listed in ascending j.  Vectorised, no torch."""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox_keys(seed: int, frame_key: int, n: int) -> np.ndarray:
    """uint32 [n]: the key of every point index 0..n-1 of one frame."""
    c0 = np.arange(n, dtype=np.uint64)
    c1 = np.zeros(n, np.uint64)
    c2 = np.full(n, frame_key & 0xFFFFFFFF, np.uint64)
    c3 = np.full(n, (frame_key >> 32) & 0xFFFFFFFF, np.uint64)
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                                  # 32 x 32 -> 64 bit products
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0.astype(np.uint32)


def select_indices(seed: int, frame_key: int, n: int, max_points: int) -> np.ndarray:
    """int64 [min(n, max_points)], ascending: the kept point indices of a frame of n points."""
    if n <= max_points:
        return np.arange(n, dtype=np.int64)
    pairs = (philox_keys(seed, frame_key, n).astype(np.uint64) << _S32) | np.arange(n, dtype=np.uint64)   # (key, j), distinct
    return np.sort(np.argpartition(pairs, max_points - 1)[:max_points]).astype(np.int64)


def prepare_points_batch(xs, ys, zs, ws, max_points: int, seed: int, frame_keys) -> np.ndarray:
    """float32 [B, max_points, 4]: what kd_points_prepare_batch writes for B ragged frames."""
    out = np.zeros((len(xs), max_points, 4), np.float32)
    for b, (x, y, z, w) in enumerate(zip(xs, ys, zs, ws)):
        idx = select_indices(seed, int(frame_keys[b]), len(x), max_points)
        out[b, : len(idx)] = np.stack([x[idx], y[idx], z[idx], w[idx]], 1)
    return out
