"""Coefficient tables of Pillow's 8-bit bilinear resample (ImagingResample: precompute_coeffs + normalize_coeffs_8bpc),
built on the host in IEEE double, cached per (in, out) pair and uploaded once per device.  The kernel behind
kd_image_resize_bilinear_batch does integer work only over these tables, so the device never rounds anything.
tests/_pil_resample_ref.py is the independent scalar model the tests hold this builder to."""
from functools import lru_cache
from typing import Tuple

import numpy as np
import torch

from .lib import KDError

PRECISION_BITS = 22                              # Pillow: 32 - 8 - 2


@lru_cache(maxsize=None)
def pil_bilinear_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (bounds int32 [n_out, 2] = (xmin, n), k int32 [n_out, ksize]) of one axis; k[xx, n:] = 0.  An unchanged axis
    (n_in == n_out) gives n = 2, k = (2^22, 0): the identity, the pass Pillow skips."""
    if n_in < 1 or n_out < 1:
        raise KDError(f"resample axis {n_in} -> {n_out}: sizes must be positive")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)             # astype truncates toward zero, as the C cast does
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    ksize = int(n.max())
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((x + xmin[:, None] - center[:, None] + 0.5) / fs))
    w[np.arange(ksize)[None, :] >= n[:, None]] = 0.0
    ww = np.cumsum(w, axis=1)[:, -1:]                                           # summed in index order, as the C loop does
    w = np.divide(w, ww, out=w, where=ww != 0.0)
    k = (0.5 + w * float(1 << PRECISION_BITS)).astype(np.int64)                 # bilinear weights are never negative
    k[np.arange(ksize)[None, :] >= n[:, None]] = 0
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    k = np.ascontiguousarray(k, dtype=np.int32)
    k.setflags(write=False)
    return bounds, k


_device_tables = {}


def device_tables(n_in: int, n_out: int, device=None):
    """(bounds, k) of `pil_bilinear_tables` as CUDA int32 tensors, uploaded once per (in, out, device) and complete on
    return, so that any stream may read them afterwards."""
    if not torch.cuda.is_available():
        raise KDError("the resample tables are read by a gfx950 kernel; there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (int(n_in), int(n_out), dev.index)
    hit = _device_tables.get(key)
    if hit is None:
        bounds, k = pil_bilinear_tables(int(n_in), int(n_out))
        hit = (torch.from_numpy(bounds.copy()).to(dev), torch.from_numpy(k.copy()).to(dev))
        torch.cuda.current_stream(dev).synchronize()
        _device_tables[key] = hit
    return hit
