"""numpy model of Pillow's 8-bit bilinear resample (ImagingResample with the BILINEAR filter), written from the
arithmetic alone: per axis the coefficient tables in IEEE double (Python floats, scalar loops, weights summed in index
order), integer coefficients k = (int)(0.5 + w * 2^22), an output sample clip(0, 255, (2^21 + sum pixel * k) >> 22), the
horizontal pass first and rounded to uint8, the vertical pass over those bytes, a pass whose size does not change
skipped.  `vertical_first=True` is the mutant with the passes swapped."""
import numpy as np

PRECISION_BITS = 22


def tables(n_in: int, n_out: int):
    """-> (xmin [n_out], n [n_out], k: list of n_out lists of Python ints) of one axis."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    xmins, ns, ks = [], [], []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        n = xmax - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmins.append(xmin)
        ns.append(n)
        ks.append([int(0.5 + v * (1 << PRECISION_BITS)) for v in w])
    return xmins, ns, ks


def dense_tables(n_in: int, n_out: int):
    """The same tables in the layout of the product's builder: bounds int32 [n_out, 2], k int32 [n_out, max n], zero tail."""
    xmins, ns, ks = tables(n_in, n_out)
    k = np.zeros((n_out, max(ns)), np.int32)
    for xx, row in enumerate(ks):
        k[xx, :len(row)] = row
    return np.stack([np.asarray(xmins), np.asarray(ns)], axis=1).astype(np.int32), k


def _pass(a: np.ndarray, axis: int, n_out: int) -> np.ndarray:
    """One pass over `axis` (0 or 1) of a uint8 [H, W, C] image."""
    n_in = a.shape[axis]
    if n_in == n_out:
        return a
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    xmins, ns, ks = tables(n_in, n_out)
    out = np.empty((n_out,) + a.shape[1:], np.uint8)
    for xx in range(n_out):
        k = np.asarray(ks[xx], np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, a[xmins[xx]:xmins[xx] + ns[xx]], axes=(0, 0))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_bilinear(a: np.ndarray, H: int, W: int, vertical_first: bool = False) -> np.ndarray:
    """uint8 [Hs, Ws, C] -> uint8 [H, W, C], the bytes of Image.fromarray(a).resize((W, H), Image.BILINEAR)."""
    assert a.dtype == np.uint8 and a.ndim == 3
    if vertical_first:
        return _pass(_pass(a, 0, H), 1, W)
    return _pass(_pass(a, 1, W), 0, H)


def frame(seed: int, Hs: int, Ws: int) -> np.ndarray:
    """Random uint8 frame with an all-255 block and an all-0 block (rounding at the clip, both ends)."""
    a = np.random.RandomState(seed).randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    a[: max(1, Hs // 3), : max(1, Ws // 3)] = 255
    a[Hs - max(1, Hs // 3):, Ws - max(1, Ws // 3):] = 0
    return a


# (Hs, Ws) -> (H, W)
REAL = ((1080, 1920), (256, 256))
SMALL_PAIRS = [((37, 53), (16, 24)),          # small downscale
               ((64, 48), (64, 20)),          # vertical pass skipped
               ((33, 33), (33, 16)),          # vertical pass skipped
               ((9, 11), (32, 40)),           # upscale, fs clamped to 1
               ((135, 240), (9, 16))]         # factor 15, 31 taps
HOST_PAIRS = [REAL, ((1080, 1920), (64, 64))] + SMALL_PAIRS
