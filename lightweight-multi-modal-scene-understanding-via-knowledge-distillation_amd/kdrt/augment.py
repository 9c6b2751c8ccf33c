"""Opt-in training augmentation: the settings and the per-frame draw (host side, numpy only).

`Augment` names the ranges; every field defaults to "off".  `frame_params` turns (settings, seed, frame keys) into one
float32 row of 16 words per frame, which csrc/kd_augment.hip applies on the device: kd_points_augment_batch to the packed
point columns before the rasteriser and the point stacker read them, kd_image_augment_batch to the float32 image batch.

Row layout (word: field), the contract with include/kd_hip.h:
     0 c   1 s   2 scale   3 tx   4 ty   5 sx   6 sy   7 gi   8 a_r   9 a_g   10 a_b   11 b   12 mirror   13..15 padding (0)

The draw.  A row is a pure function of (settings, seed, frame key): not of the batch, the rank or the order.  Twelve
32-bit words w0..w11 = the output blocks of Philox-4x32-10 at the counters (k, 1, key low word, key high word), k = 0, 1,
2, under the key (seed low word, seed high word).  Counter word 1 is 1 here, 0 in the subset sampler of
kd_points_prepare_batch and 2 in the per-point jitter, so the three streams never meet.  u_k = (w_k >> 8) * 2**-24 in
[0, 1), d(r, u) = r * (2u - 1); everything below in float64, each field rounded once to float32:
     w0   yaw = d(rot_deg, u0) degrees;  c, s = cos, sin of it, after reducing the angle to a multiple of 90 degrees plus a
          rest in [-45, 45], so that 0, +-90 and +-180 degrees give exact 0 and +-1
     w1   scale = 1 + d(scale, u1)
     w2   tx = d(translate, u2)                    w3   ty = d(translate, u3)
     w4   flipped = u4 < flip:  the sign of `flip_axis` (sx or sy) is -1 and mirror = 1, else both signs +1 and mirror = 0
     w5   gi = 1 + d(intensity, u5)
     w6   brightness = d(brightness, u6)           w7   contrast = 1 + d(contrast, u7)
     w8, w9, w10   channel gain r, g, b = 1 + d(channel_gain, u)
     w11  dropped = u11 < camera_drop:  a_r = a_g = a_b = b = 0 (the frame's image becomes all zero)
     a_c = gain_c * contrast,   b = 0.5 * (1 - contrast) + brightness
tests/_augment_ref.py holds an independent numpy mirror of this draw and of both kernels.
"""
from dataclasses import dataclass, fields

import numpy as np

from .lib import KDError

ROW = 16
_KEYS = {"rot": "rot_deg"}                       # short forms accepted by Augment.parse


@dataclass(frozen=True)
class Augment:
    rot_deg: float = 0.0          # yaw about the origin, uniform in +-rot_deg
    scale: float = 0.0            # isotropic factor on x, y, z, uniform in 1 +- scale
    translate: float = 0.0        # metres; tx and ty independent, uniform in +-translate
    flip: float = 0.0             # probability of the joint flip: LiDAR `flip_axis` negated AND the image mirrored
    flip_axis: str = "y"          # "x" or "y"
    jitter: float = 0.0           # metres; per point and coordinate, uniform in [-jitter, jitter)
    intensity: float = 0.0        # gain on column i, uniform in 1 +- intensity
    brightness: float = 0.0       # additive on the [0, 1] scale, uniform in +-brightness
    contrast: float = 0.0         # gain about 0.5, uniform in 1 +- contrast
    channel_gain: float = 0.0     # per colour channel, uniform in 1 +- channel_gain
    camera_drop: float = 0.0      # probability that the frame's image becomes all zero

    def __post_init__(self):
        def num(name, lo, hi, hi_open=False):
            v = getattr(self, name)
            try:
                v = float(v)
            except (TypeError, ValueError):
                raise KDError(f"Augment.{name} must be a number, got {getattr(self, name)!r}") from None
            if not (np.isfinite(v) and lo <= v and (v < hi if hi_open else v <= hi)):
                raise KDError(f"Augment.{name} = {v} outside [{lo}, {hi}{')' if hi_open else ']'}")
            object.__setattr__(self, name, v)
        num("rot_deg", 0.0, 180.0)
        num("scale", 0.0, 1.0, hi_open=True)                  # the factor stays positive
        num("translate", 0.0, 1e6)
        num("flip", 0.0, 1.0)
        num("jitter", 0.0, 1e6)
        for name in ("intensity", "brightness", "contrast", "channel_gain", "camera_drop"):
            num(name, 0.0, 1.0)
        if self.flip_axis not in ("x", "y"):
            raise KDError(f"Augment.flip_axis must be 'x' or 'y', got {self.flip_axis!r}")

    @property
    def points_on(self) -> bool:
        return any(v > 0 for v in (self.rot_deg, self.scale, self.translate, self.flip, self.jitter, self.intensity))

    @property
    def image_on(self) -> bool:
        return any(v > 0 for v in (self.flip, self.brightness, self.contrast, self.channel_gain, self.camera_drop))

    @property
    def enabled(self) -> bool:
        return self.points_on or self.image_on

    @classmethod
    def parse(cls, text: str) -> "Augment":
        """"rot=5,flip=0.5,flip_axis=y,jitter=0.02" -> Augment (the KD_LOADER_AUGMENT form).  Keys are the field names, `rot`
        is short for `rot_deg`; an unknown key, a repeated key or an item without `=` is a KDError.  "" is all off."""
        names = {f.name for f in fields(cls)}
        kw = {}
        for item in (v.strip() for v in (text or "").split(",")):
            if not item:
                continue
            if "=" not in item:
                raise KDError(f"augment setting '{item}' is not key=value")
            k, v = (s.strip() for s in item.split("=", 1))
            k = _KEYS.get(k, k)
            if k not in names:
                raise KDError(f"unknown augment setting '{k}' (known: {', '.join(sorted(names))})")
            if k in kw:
                raise KDError(f"augment setting '{k}' given twice")
            if k == "flip_axis":
                kw[k] = v
            else:
                try:
                    kw[k] = float(v)
                except ValueError:
                    raise KDError(f"augment setting '{k}' needs a number, got '{v}'") from None
        return cls(**kw)

    def to_string(self) -> str:
        """The parse form of this setting: Augment.parse(a.to_string()) == a."""
        d = Augment()
        return ",".join(f"{f.name}={getattr(self, f.name)!r}".replace("'", "") for f in fields(self)
                        if getattr(self, f.name) != getattr(d, f.name))


def as_augment(value):
    """None / "" / an all-off Augment -> None; a parse string -> Augment; an Augment -> itself."""
    if value is None:
        return None
    if isinstance(value, str):
        value = Augment.parse(value)
    if not isinstance(value, Augment):
        raise KDError(f"augment must be an Augment, a parse string or None, got {type(value).__name__}")
    return value if value.enabled else None


_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_LO, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int) -> np.ndarray:
    """uint32 [n, 4]: the Philox-4x32-10 output block of every counter (c0[i], c1[i], c2[i], c3[i]) under key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _LO for c in np.broadcast_arrays(*(np.atleast_1d(c) for c in (c0, c1, c2, c3))))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LO, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LO
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _cos_sin_deg(deg: np.ndarray):
    q = np.rint(deg / 90.0)
    r = np.deg2rad(deg - 90.0 * q)
    cr, sr = np.cos(r), np.sin(r)
    k = q.astype(np.int64) % 4
    c = np.choose(k, [cr, -sr, -cr, sr])
    s = np.choose(k, [sr, cr, -sr, -cr])
    return c, s


def rows_from_values(aug: Augment, yaw_deg, scale, tx, ty, flipped, gi, brightness, contrast, gain_rgb, dropped) -> np.ndarray:
    """float32 [B, 16] from the drawn quantities (float64 / bool arrays of length B; gain_rgb [B, 3]): the layout and the
    roundings of the module docstring.  `frame_params` ends here; also the way to build a row for a chosen transform."""
    yaw_deg = np.atleast_1d(np.asarray(yaw_deg, np.float64))
    B = yaw_deg.shape[0]
    full = lambda v: np.broadcast_to(np.asarray(v, np.float64), (B,))
    flipped, dropped = np.broadcast_to(np.asarray(flipped, bool), (B,)), np.broadcast_to(np.asarray(dropped, bool), (B,))
    contrast, keep = full(contrast), np.where(dropped, 0.0, 1.0)
    row = np.zeros((B, ROW), np.float64)
    row[:, 0], row[:, 1] = _cos_sin_deg(yaw_deg)
    row[:, 2], row[:, 3], row[:, 4] = full(scale), full(tx), full(ty)
    sign = np.where(flipped, -1.0, 1.0)
    row[:, 5] = sign if aug.flip_axis == "x" else 1.0
    row[:, 6] = sign if aug.flip_axis == "y" else 1.0
    row[:, 7] = full(gi)
    row[:, 8:11] = np.broadcast_to(np.asarray(gain_rgb, np.float64), (B, 3)) * contrast[:, None] * keep[:, None]
    row[:, 11] = (0.5 * (1.0 - contrast) + full(brightness)) * keep
    row[:, 12] = np.where(flipped, 1.0, 0.0)
    return (row + 0.0).astype(np.float32)                     # + 0.0: a zero range times a negative draw is no negative zero


def frame_params(aug: Augment, seed: int, frame_keys) -> np.ndarray:
    """float32 [B, 16]: one row per frame key, by the draw of the module docstring."""
    keys = [int(k) & 0xFFFFFFFFFFFFFFFF for k in frame_keys]
    lo = np.asarray([k & 0xFFFFFFFF for k in keys], np.uint64)
    hi = np.asarray([k >> 32 for k in keys], np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = np.concatenate([philox4x32_10(np.full(len(keys), k, np.uint64), 1, lo, hi, seed & 0xFFFFFFFF, seed >> 32) for k in range(3)],
                       axis=1)                                  # [B, 12]
    u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    d = lambda r, k: r * (2.0 * u[:, k] - 1.0)
    gains = 1.0 + np.stack([d(aug.channel_gain, 8), d(aug.channel_gain, 9), d(aug.channel_gain, 10)], axis=1)
    return rows_from_values(aug, yaw_deg=d(aug.rot_deg, 0), scale=1.0 + d(aug.scale, 1), tx=d(aug.translate, 2),
                            ty=d(aug.translate, 3), flipped=u[:, 4] < aug.flip, gi=1.0 + d(aug.intensity, 5),
                            brightness=d(aug.brightness, 6), contrast=1.0 + d(aug.contrast, 7), gain_rgb=gains,
                            dropped=u[:, 11] < aug.camera_drop)
