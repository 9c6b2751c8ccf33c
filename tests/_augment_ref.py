"""Independent numpy mirror of the device augmentation (include/kd_hip.h, csrc/kd_augment.hip, kdrt/augment.py):
its own full Philox-4x32-10, the per-frame draw of the 16-word rows, and both kernels in float32 with the specified order
of operations (every product and sum rounded separately).  No torch, no import from the product."""
import numpy as np

F = np.float32
_MUL = (0xD2511F53, 0xCD9E8D57)
_WEYL = (0x9E3779B9, 0xBB67AE85)
_MASK = 0xFFFFFFFF


def philox(counters, key) -> np.ndarray:
    """uint32 [n, 4] output blocks for uint32 counters [n, 4] under key = (k0, k1); ten rounds, Random123's order."""
    x = np.array(counters, dtype=np.uint64).reshape(-1, 4) & np.uint64(_MASK)
    k = [int(key[0]) & _MASK, int(key[1]) & _MASK]
    for _ in range(10):
        prod0 = x[:, 0] * np.uint64(_MUL[0])
        prod1 = x[:, 2] * np.uint64(_MUL[1])
        nxt = np.empty_like(x)
        nxt[:, 0] = (prod1 >> np.uint64(32)) ^ x[:, 1] ^ np.uint64(k[0])
        nxt[:, 1] = prod1 & np.uint64(_MASK)
        nxt[:, 2] = (prod0 >> np.uint64(32)) ^ x[:, 3] ^ np.uint64(k[1])
        nxt[:, 3] = prod0 & np.uint64(_MASK)
        x = nxt
        k = [(k[0] + _WEYL[0]) & _MASK, (k[1] + _WEYL[1]) & _MASK]
    return x.astype(np.uint32)


def _split(v: int):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v & _MASK, v >> 32


def _trig_deg(a: float):
    """cos, sin of `a` degrees: a = 90 q + rest, rest in [-45, 45]; exact at multiples of 90."""
    q = float(np.rint(a / 90.0))
    rest = np.deg2rad(np.float64(a) - 90.0 * q)
    cr, sr = np.cos(rest), np.sin(rest)
    return [(cr, sr), (-sr, cr), (-cr, -sr), (sr, -cr)][int(q) % 4]


def make_row(aug, yaw_deg=0.0, scale=1.0, tx=0.0, ty=0.0, flipped=False, gi=1.0, brightness=0.0, contrast=1.0,
             gains=(1.0, 1.0, 1.0), dropped=False) -> np.ndarray:
    """float32 [16]: c s scale tx ty sx sy gi a_r a_g a_b b mirror 0 0 0, computed in float64 and rounded once."""
    c, s = _trig_deg(float(yaw_deg))
    sign = -1.0 if flipped else 1.0
    keep = 0.0 if dropped else 1.0
    row = [c, s, scale, tx, ty, sign if aug.flip_axis == "x" else 1.0, sign if aug.flip_axis == "y" else 1.0, gi]
    row += [float(g) * contrast * keep for g in gains]
    row += [(0.5 * (1.0 - contrast) + brightness) * keep, 1.0 if flipped else 0.0, 0.0, 0.0, 0.0]
    return (np.asarray(row, np.float64) + 0.0).astype(F)


def frame_rows(aug, seed: int, frame_keys) -> np.ndarray:
    """float32 [B, 16]: words w0..w11 of the blocks at counters (0 | 1 | 2, 1, key lo, key hi) under (seed lo, seed hi);
    w0 yaw, w1 scale, w2 tx, w3 ty, w4 flip, w5 intensity, w6 brightness, w7 contrast, w8-10 channel gains, w11 drop."""
    rows = []
    for fk in frame_keys:
        lo, hi = _split(fk)
        w = philox([[k, 1, lo, hi] for k in range(3)], _split(seed)).reshape(12)
        u = [float(int(v) >> 8) * 2.0 ** -24 for v in w]
        d = lambda r, k: float(r) * (2.0 * u[k] - 1.0)
        rows.append(make_row(aug, yaw_deg=d(aug.rot_deg, 0), scale=1.0 + d(aug.scale, 1), tx=d(aug.translate, 2),
                             ty=d(aug.translate, 3), flipped=u[4] < aug.flip, gi=1.0 + d(aug.intensity, 5),
                             brightness=d(aug.brightness, 6), contrast=1.0 + d(aug.contrast, 7),
                             gains=[1.0 + d(aug.channel_gain, k) for k in (8, 9, 10)], dropped=u[11] < aug.camera_drop))
    return np.stack(rows) if rows else np.zeros((0, 16), F)


def augment_points(x, y, z, i, row, seed: int, frame_key: int, jitter: float):
    """One frame through kd_points_augment_batch's formula -> (x', y', z', i') float32."""
    x, y, z, i = (np.asarray(v, F) for v in (x, y, z, i))
    c, s, sc, tx, ty, sx, sy, gi = (F(v) for v in row[:8])
    with np.errstate(invalid="ignore"):
        xf, yf = sx * x, sy * y
        xr = c * xf - s * yf
        yr = s * xf + c * yf
        xo, yo, zo, io = sc * xr + tx, sc * yr + ty, sc * z, gi * i
        if jitter > 0:
            n = len(x)
            lo, hi = _split(frame_key)
            ctr = np.stack([np.arange(n, dtype=np.uint64), np.full(n, 2, np.uint64), np.full(n, lo, np.uint64),
                            np.full(n, hi, np.uint64)], axis=1)
            w = philox(ctr, _split(seed)) if n else np.zeros((0, 4), np.uint32)
            jit = F(jitter) * ((w[:, :3] >> np.uint32(8)).astype(F) * F(2.0 ** -23) - F(1.0))
            xo, yo, zo = xo + jit[:, 0], yo + jit[:, 1], zo + jit[:, 2]
    assert all(v.dtype == F for v in (xo, yo, zo, io))
    return xo, yo, zo, io


def augment_image(img_chw, row) -> np.ndarray:
    """float32 [3, H, W] through kd_image_augment_batch's formula."""
    img = np.asarray(img_chw, F)
    out = np.empty_like(img)
    for c in range(3):
        out[c] = np.minimum(np.maximum(img[c] * F(row[8 + c]) + F(row[11]), F(0.0)), F(1.0))
    return out[:, :, ::-1].copy() if row[12] != 0 else out


def same_bits(got, want) -> bool:
    """Bit for bit where the reference is a number; NaN exactly where the reference is NaN."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def pipeline(raws, aug, seed: int, frame_keys, max_points: int, grid_size, pc_range):
    """What an augmented loader must deliver for raw frames of at most max_points points: (image [B,3,H,W], points
    [B,max_points,4], segmentation [B,GH,GW]) through the mirror and the project's host rasteriser."""
    import data_oracle as D
    rows = frame_rows(aug, seed, frame_keys)
    imgs, pts, segs = [], [], []
    for r, row, fk in zip(raws, rows, frame_keys):
        x, y, z, i = augment_points(r["x"], r["y"], r["z"], r["i"], row, seed, fk, aug.jitter)
        assert len(x) <= max_points
        p = np.zeros((max_points, 4), F)
        p[:len(x)] = np.stack([x, y, z, i], axis=1)
        pts.append(p)
        segs.append(D.rasterize_bev(x, y, D.remap_semantic(np.asarray(r["class"])), grid_size, pc_range))
        imgs.append(augment_image(D.image_to_chw(np.asarray(r["image_u8"])), row))
    return np.stack(imgs), np.stack(pts), np.stack(segs)
