"""PandaSet reader with the per-frame preparation on the MI355X -- drop-in for the reference's
src/data_loading/pandaset_dataset.py (same names, signatures, sample dictionary).

Host side (as in the reference): directory indexing (:71-99), JPEG decode + PIL bilinear resize (:105-107),
pandas pickle reads (:114-118,130-131).  Device side (csrc/kd_input.hip through the C ABI): uint8 HWC -> float32
CHW / 255 (:108-111), point stacking + zero padding or subsample gather (:119-127), remap_semantic (:13-20) and
rasterize_bev (:23-45, the reference's 44 ms/frame Python loop).  `dataset[i]` returns the reference's sample
dictionary with CUDA tensors.  The loaders from `create_pandaset_dataloaders` keep DataLoader worker processes for
the host I/O only (`load_raw`: decode + unpickle, nothing touches the GPU there) and prepare each whole batch on
the device in the consuming process (`DeviceBatchLoader`: one rasteriser launch per batch over ragged frames);
`.to(device)` in the trainer is then a no-op.  `DeviceBatchLoader(prefetch >= 1)` prepares batch k+1 while the step
consumes batch k: one host-to-device copy per tensor from pinned staging buffers and three launches per batch
(`prepare_batch_staged`) on a side stream; long sweeps are then cut by the device sampler of kd_points_prepare_batch,
keyed on (`sample_seed`, epoch, dataset index).

`device_resize=True` (opt-in, default off) moves the resize to the device as well: `load_raw` then only decodes, the
full-size uint8 frames travel to the GPU and kd_image_resize_bilinear_batch produces the float32 [B,3,H,W] batch with
Pillow's exact bytes (integer resample over host-built coefficient tables, kdrt/resample.py).

`augment=Augment(...)` (opt-in, default off, training loader only; kdrt/augment.py) transforms each batch on the device
before anything reads it: kd_points_augment_batch rewrites the packed point columns (joint flip, yaw, scale, translation,
jitter, intensity gain) ahead of the rasteriser and the point stacker, so BEV labels and points agree by construction,
and kd_image_augment_batch adjusts the float32 image batch (gains, offset, clamp, the flip's mirror, camera dropout).
Every frame's transform is a function of (`sample_seed`, epoch, dataset index) alone.

`label_rule=LabelRule(...)` (opt-in, default off, with a `class_map` only): a BEV cell takes the majority or the highest-priority
class of its points (kd_bev_rasterize_vote) and not the class of its first labelled point in sweep order; `label_counts()` and
kdrt.losses.class_weights_from_counts turn the rasterised labels into class weights.

`SyntheticPandaSet` serves frames of the same contract when there is no dataset on disk:
    image        float32 [3, 256, 256] in [0, 1]
    points       float32 [max_points, 4]  (x, y, z, intensity), zero-padded tail
    segmentation int64   [64, 64]   2-class BEV mask
"""
import gc
import os
from collections import deque
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

from kdrt import KDError
from kdrt.augment import Augment, as_augment, frame_params
from kdrt.lib import lib
from kdrt.ops import P, stream, workspace
from kdrt.resample import device_tables

_DRIVABLE = {6, 7, 8, 9, 10, 12}          # Ground, Road, Lane markings, Stop lines, Other markings, Driveway (:13)
_DRIVABLE_BITS = sum(1 << k for k in _DRIVABLE)


def _dev(t, dtype):
    """numpy array / tensor -> contiguous CUDA tensor of `dtype` (the dtype conversion is the reference's host-side
    `to_numpy(dtype=...)`; everything after it runs on the device)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.require(t, requirements=["C", "W"]))
    t = t.to(dtype)
    if not torch.cuda.is_available():
        raise KDError("input preparation runs on the MI355X; there is no CPU fallback")
    return t.cuda().contiguous()


def _f32(v) -> float:
    return float(np.float32(v))


def _vote_launch(rule: "LabelRule", rank_dev, num_classes: int, x, y, lab, off, B: int, n: int, H: int, W: int, pc_range, ws,
                 nbytes: int, mask, votes, s: int):
    """kd_bev_rasterize_vote on stream `s`: the cell rule of `rule` over class indices (`rank_dev`: rule.ranks() on the device)."""
    x0, x1, y0, y1 = pc_range
    lib.call("kd_bev_rasterize_vote", P(x), P(y), P(lab), P(off), B, n, num_classes, rule.code, P(rank_dev), rule.min_points, H, W,
             _f32(x0), _f32(x1 - x0), _f32(x1), _f32(y0), _f32(y1 - y0), _f32(y1), P(ws), nbytes, P(mask), P(votes), s)


def rasterize_bev_batch(xs: Sequence, ys: Sequence, classes: Sequence, grid_size=(64, 64), pc_range=(-50, 50, -50, 50),
                        remap: bool = False, rule: "LabelRule" = None, num_classes: int = None, want_votes: bool = False):
    """B ragged frames in one launch -> int64 [B, H, W] on the device.  remap=True applies remap_semantic first.
    `rule` (a LabelRule; None: the first labelled point of a cell wins, the call as it always was): majority or priority per cell
    over class indices in [0, num_classes - 1] -- it needs remap=False and `num_classes`.  want_votes=True (with a rule) also
    returns the winner's point count per cell, int32 [B, H, W]."""
    if rule is not None:
        if not isinstance(rule, LabelRule):
            raise ValueError(f"rule must be a LabelRule or None, got {type(rule).__name__}")
        if remap or num_classes is None:
            raise ValueError("a label rule votes over class indices: it needs remap=False and num_classes")
        rank = rule.ranks(num_classes)                     # validates num_classes and the ranks' classes (ValueError)
    elif want_votes:
        raise ValueError("want_votes needs a label rule: the first-point rule counts nothing")
    B = len(xs)
    if B == 0:
        raise KDError("rasterize_bev_batch needs at least one frame")
    lens = [int(np.shape(x)[0]) for x in xs]
    x = torch.cat([_dev(v, torch.float32).reshape(-1) for v in xs])
    y = torch.cat([_dev(v, torch.float32).reshape(-1) for v in ys])
    c = torch.cat([_dev(v, torch.int64).reshape(-1) for v in classes])
    if not (x.numel() == y.numel() == c.numel() == sum(lens)):
        raise KDError("x, y and labels must have the same length per frame")
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64).cuda()
    H, W = int(grid_size[0]), int(grid_size[1])
    x0, x1, y0, y1 = pc_range
    mask = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
    if rule is not None:
        votes = torch.empty(B, H, W, dtype=torch.int32, device="cuda") if want_votes else None
        nbytes = lib.kd_bev_rasterize_vote_ws_bytes(B, H, W, num_classes)
        _vote_launch(rule, torch.from_numpy(rank).cuda(), num_classes, x, y, c, off, B, x.numel(), H, W, pc_range,
                     workspace(nbytes, mask.device), nbytes, mask, votes, stream())
        return (mask, votes) if want_votes else mask
    nbytes = lib.kd_bev_rasterize_ws_bytes(B, H, W)
    ws = workspace(nbytes, mask.device)
    lib.call("kd_bev_rasterize", P(x), P(y), P(c), P(off), B, x.numel(), 1 if remap else 0, _DRIVABLE_BITS, H, W,
             _f32(x0), _f32(x1 - x0), _f32(x1), _f32(y0), _f32(y1 - y0), _f32(y1), P(ws), nbytes, P(mask), stream())
    return mask


def remap_semantic(raw_ids):
    """PandaSet raw class ids -> {0 = background, 1 = drivable incl. lanes}.  numpy in -> numpy out (as the
    reference), tensor in -> CUDA tensor out; computed on the device either way."""
    ids = _dev(raw_ids, torch.int64)
    flat = ids.reshape(-1)
    out = torch.empty_like(flat)
    lib.call("kd_semantic_remap", P(flat), flat.numel(), _DRIVABLE_BITS, P(out), stream())
    out = out.reshape(ids.shape)
    return out.cpu().numpy() if isinstance(raw_ids, np.ndarray) else out


MAX_CLASSES = 16          # the widest head the loss, classifier and metric kernels take


def class_map_table(class_map) -> np.ndarray:
    """`class_map` -> the int64 lookup table of kd_semantic_remap_table: table[raw id] = class index, ids the map does not name -> 0.
    A dict {raw id: class} or a sequence indexed by raw id; raw ids are integers >= 0, classes integers in [0, 15] with 0 the
    background.  Anything else is a ValueError."""
    def _int(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"class_map: {what} must be an integer, got {v!r}")
        return int(v)
    if isinstance(class_map, dict):
        items = [(_int(k, "a raw id"), _int(v, "a class index")) for k, v in class_map.items()]
    elif isinstance(class_map, (list, tuple, np.ndarray)) and np.ndim(class_map) == 1:
        items = [(i, _int(v, "a class index")) for i, v in enumerate(list(class_map))]
    else:
        raise ValueError(f"class_map must be a dict {{raw id: class}} or a sequence indexed by raw id, got {type(class_map).__name__}")
    if not items:
        raise ValueError("class_map is empty")
    for k, v in items:
        if k < 0 or k >= (1 << 20):
            raise ValueError(f"class_map: raw id {k} outside [0, 2^20)")
        if v < 0 or v >= MAX_CLASSES:
            raise ValueError(f"class_map: class index {v} (raw id {k}) outside [0, {MAX_CLASSES - 1}]")
    table = np.zeros(max(k for k, _ in items) + 1, np.int64)
    for k, v in items:
        table[k] = v
    return table


_RULE_CODES = {"majority": 1, "priority": 2}           # the `rule` argument of kd_bev_rasterize_vote


def _rank_int(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"LabelRule: {what} must be an integer, got {v!r}")
    v = int(v)
    if not -(1 << 31) <= v < (1 << 31):
        raise ValueError(f"LabelRule: {what} {v} outside int32")
    return v


@dataclass(frozen=True)
class LabelRule:
    """How a BEV cell with points of several classes gets its label (kd_bev_rasterize_vote; classes are the indices of a class map,
    0 = background, which never votes).  A class is eligible in a cell with at least `min_points` points there.
    kind="majority": the eligible class with the most points; equal counts go to the higher rank, then to the lower class index.
    kind="priority": the eligible class of the highest rank; equal ranks go to the larger count, then to the lower class index.
    `priority`: None (every rank 0), a sequence of one integer rank per class (index 0 is ignored), or a dict {class: rank} whose
    unnamed classes have rank 0.  Validated here (ValueError); that the classes lie inside a map's range is checked where the map is
    known (`ranks`, the dataset's constructor).  Without a rule a cell takes the class of its first labelled point in input order."""
    kind: str = "majority"
    priority: object = None
    min_points: int = 1

    def __post_init__(self):
        if self.kind not in _RULE_CODES:
            raise ValueError(f"LabelRule: kind must be 'majority' or 'priority', got {self.kind!r}")
        if isinstance(self.min_points, bool) or not isinstance(self.min_points, (int, np.integer)) or not 1 <= self.min_points < (1 << 31):
            raise ValueError(f"LabelRule: min_points must be an integer >= 1, got {self.min_points!r}")
        object.__setattr__(self, "min_points", int(self.min_points))
        pr = self.priority
        if pr is None:
            return
        if isinstance(pr, dict):
            items = tuple(sorted((_rank_int(k, "a class index"), _rank_int(v, f"the rank of class {k}")) for k, v in pr.items()))
            for c, _ in items:
                if not 0 <= c < MAX_CLASSES:
                    raise ValueError(f"LabelRule: class index {c} outside [0, {MAX_CLASSES - 1}]")
            object.__setattr__(self, "priority", dict(items))
        elif isinstance(pr, (list, tuple, np.ndarray)) and np.ndim(pr) == 1:
            ranks = tuple(_rank_int(v, f"the rank of class {c}") for c, v in enumerate(list(pr)))
            if not 2 <= len(ranks) <= MAX_CLASSES:
                raise ValueError(f"LabelRule: a priority sequence has one rank per class, 2 to {MAX_CLASSES}; got {len(ranks)}")
            object.__setattr__(self, "priority", ranks)
        else:
            raise ValueError(f"LabelRule: priority must be None, a sequence of ranks or a dict {{class: rank}}, got {type(pr).__name__}")

    @property
    def code(self) -> int:
        return _RULE_CODES[self.kind]

    def ranks(self, num_classes: int) -> np.ndarray:
        """int32 [num_classes]: the `rank` array of kd_bev_rasterize_vote.  ValueError when the rule does not fit `num_classes`
        classes: a sequence of another length, a dict that names a class outside [0, num_classes - 1]."""
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 2 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"LabelRule: num_classes must be an integer in [2, {MAX_CLASSES}], got {num_classes!r}")
        out = np.zeros(int(num_classes), np.int32)
        if isinstance(self.priority, dict):
            for c, r in self.priority.items():
                if c >= num_classes:
                    raise ValueError(f"LabelRule: priority names class {c}, the class map has classes 0..{num_classes - 1}")
                out[c] = r
        elif self.priority is not None:
            if len(self.priority) != num_classes:
                raise ValueError(f"LabelRule: priority has {len(self.priority)} ranks, the class map has {num_classes} classes")
            out[:] = self.priority
        return out


def remap_semantic_table(raw_ids, table, s: int = None):
    """raw class ids -> table[raw id] on the device (ids outside the table -> 0): numpy in -> numpy out, tensor in -> CUDA tensor
    out, like remap_semantic.  `table`: what class_map_table returns, or its CUDA copy; `s`: the stream (default the current one)."""
    ids = _dev(raw_ids, torch.int64)
    tab = _dev(table, torch.int64).reshape(-1)
    if tab.numel() == 0:
        raise KDError("remap_semantic_table needs a table of at least one entry")
    flat = ids.reshape(-1)
    out = torch.empty_like(flat)
    lib.call("kd_semantic_remap_table", P(flat), flat.numel(), P(tab), tab.numel(), P(out), stream() if s is None else s)
    out = out.reshape(ids.shape)
    return out.cpu().numpy() if isinstance(raw_ids, np.ndarray) else out


def rasterize_bev(x, y, labels, grid_size: Tuple[int, int] = (64, 64),
                  pc_range: Tuple[float, float, float, float] = (-50, 50, -50, 50)):
    """Per-point labels -> BEV mask, first non-zero label per cell in point order.  numpy in -> numpy out."""
    m = rasterize_bev_batch([x], [y], [labels], grid_size, pc_range, remap=False)[0]
    return m.cpu().numpy() if isinstance(x, np.ndarray) else m


def prepare_points(x, y, z, i, max_points: int, generator=None) -> torch.Tensor:
    """float32 [max_points, 4]: zero-padded, or a uniform subset without replacement when the sweep is longer."""
    x, y, z, i = (_dev(v, torch.float32) for v in (x, y, z, i))
    n = x.numel()
    out = torch.empty(max_points, 4, dtype=torch.float32, device="cuda")
    choice = None
    if n > max_points:
        choice = torch.randperm(n, device="cuda", generator=generator)[:max_points].contiguous()
    lib.call("kd_points_prepare", P(x), P(y), P(z), P(i), P(choice), n, max_points, P(out), stream())
    return out


def image_to_chw(img_u8_hwc) -> torch.Tensor:
    t = _dev(np.asarray(img_u8_hwc), torch.uint8)
    if t.dim() != 3 or t.shape[2] != 3:
        raise KDError(f"expected an HxWx3 uint8 image, got {tuple(t.shape)}")
    H, W = int(t.shape[0]), int(t.shape[1])
    out = torch.empty(3, H, W, dtype=torch.float32, device="cuda")
    lib.call("kd_image_u8hwc_to_f32chw", P(t), P(out), H, W, stream())
    return out


def _resize_launch(src: torch.Tensor, size: Tuple[int, int], out_f32, out_u8, s: int):
    """kd_image_resize_bilinear_batch over src uint8 [B,Hs,Ws,3] on stream `s`; size = (width, height) as Image.resize."""
    B, Hs, Ws = int(src.shape[0]), int(src.shape[1]), int(src.shape[2])
    W, H = int(size[0]), int(size[1])
    if not lib.kd_image_resize_bilinear_supported(Hs, Ws, H, W):
        raise KDError(f"device resize of {Ws}x{Hs} -> {W}x{H} (width x height) is outside the kernel's range: sources up to "
                      "4096x4096, downscale up to a factor of 16 per axis")
    hb, hk = device_tables(Ws, W, src.device)
    vb, vk = device_tables(Hs, H, src.device)
    lib.call("kd_image_resize_bilinear_batch", P(src), P(hb), P(hk), int(hk.shape[1]), P(vb), P(vk), int(vk.shape[1]),
             P(out_f32), P(out_u8), B, Hs, Ws, H, W, s)


def resize_images_pil_bilinear(img_u8_bhwc, size: Tuple[int, int], want_u8: bool = False):
    """uint8 [B,Hs,Ws,3] frames of one size -> float32 [B,3,H,W] on the device, the bits of
    `image_to_chw(Image.fromarray(frame).resize(size, Image.BILINEAR))` per frame; size = (width, height) as Pillow takes
    it.  want_u8=True also returns the resized bytes, uint8 [B,H,W,3]."""
    t = _dev(img_u8_bhwc if torch.is_tensor(img_u8_bhwc) else np.asarray(img_u8_bhwc), torch.uint8)
    if t.dim() != 4 or t.shape[3] != 3 or t.shape[0] == 0:
        raise KDError(f"expected B x H x W x 3 uint8 images, got {tuple(t.shape)}")
    W, H = int(size[0]), int(size[1])
    out = torch.empty(t.shape[0], 3, H, W, dtype=torch.float32, device="cuda")
    u8 = torch.empty(t.shape[0], H, W, 3, dtype=torch.uint8, device="cuda") if want_u8 else None
    _resize_launch(t, (W, H), out, u8, stream())
    return (out, u8) if want_u8 else out


def _u64(v: int) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _augment_launches(aug: Augment, params, x, y, z, w, off, keys, B: int, n: int, sample_seed: int, s: int):
    """kd_points_augment_batch over the packed columns of a batch, in place, on stream `s` (skipped when no point
    setting is on: the columns then keep their bits)."""
    if aug.points_on and n > 0:
        lib.call("kd_points_augment_batch", P(x), P(y), P(z), P(w), P(off), P(keys), P(params), B, n, _u64(sample_seed),
                 _f32(aug.jitter), s)


def _augment_image_launch(aug: Augment, params, img: torch.Tensor, s: int):
    """kd_image_augment_batch over float32 [B,3,H,W], in place, on stream `s` (skipped when no image setting is on)."""
    if aug.image_on:
        lib.call("kd_image_augment_batch", P(img), P(params), int(img.shape[0]), int(img.shape[2]), int(img.shape[3]), s)


class StagingSet:
    """Pinned host buffers of ONE batch in flight (grow-only) + the event after its host-to-device copies: the buffers
    are not refilled before that event has completed."""

    def __init__(self):
        self.cols = self.cls = self.img = self.meta = self.aug = None
        self.copied = None

    def _fit(self, name: str, numel: int, dtype) -> np.ndarray:
        buf = getattr(self, name)
        if buf is None or buf.numel() < numel:
            buf = torch.empty(max(numel, 1), dtype=dtype).pin_memory()
            setattr(self, name, buf)
        return buf.numpy()

    def fill(self, raws: Sequence[Dict[str, object]], frame_keys: Sequence[int], col_align: int = 1, params: np.ndarray = None):
        """-> (lens, image shape) after packing the batch: cols = x | y | z | i (each n_total float32, column c at
        c * stride, stride = n_total rounded up to `col_align`: kept in `self.stride`), cls (n_total int64), img [B,H,W,3]
        uint8, meta = offsets [B+1] | frame keys [B] (int64), and -- with `params` -- aug = the float32 [B,16] rows."""
        if self.copied is not None:
            self.copied.synchronize()
        B = len(raws)
        lens = [int(np.shape(r["x"])[0]) for r in raws]
        n = sum(lens)
        if any(int(np.shape(r[k])[0]) != m for r, m in zip(raws, lens) for k in ("y", "z", "i", "class")):
            raise KDError("x, y, z, i and class must have the same length per frame")
        ns = self.stride = -(-n // col_align) * col_align
        cols = self._fit("cols", 4 * ns, torch.float32)
        for c, k in enumerate("xyzi"):
            np.concatenate([np.asarray(r[k], np.float32).reshape(-1) for r in raws], out=cols[c * ns:c * ns + n])
        np.concatenate([np.asarray(r["class"], np.int64).reshape(-1) for r in raws], out=self._fit("cls", n, torch.int64)[:n])
        shape = tuple(np.shape(raws[0]["image_u8"]))
        if len(shape) != 3 or shape[2] != 3 or any(tuple(np.shape(r["image_u8"])) != shape for r in raws):
            raise KDError(f"expected HxWx3 uint8 images of one size per batch, got {[np.shape(r['image_u8']) for r in raws]}")
        img = self._fit("img", B * shape[0] * shape[1] * 3, torch.uint8)[: B * shape[0] * shape[1] * 3].reshape(B, *shape)
        for b, r in enumerate(raws):
            img[b] = np.asarray(r["image_u8"])
        meta = self._fit("meta", 2 * B + 1, torch.int64)
        meta[0] = 0
        np.cumsum(lens, out=meta[1:B + 1])
        meta[B + 1:2 * B + 1] = np.asarray([k & 0xFFFFFFFFFFFFFFFF for k in frame_keys], np.uint64).view(np.int64)
        if params is not None:
            self._fit("aug", params.size, torch.float32)[:params.size] = params.reshape(-1)
        return lens, shape


class PandaSetDataset(Dataset):
    """2-class version: background (0) and drivable (1, includes lanes).  `class_map` (a dict or sequence raw id -> class index
    in [0, NC-1], 0 = background; see class_map_table): the multi-class version -- every prepare path then runs the table remap as
    one extra launch and rasterises the class indices (first point in input order with a non-zero class wins, as before).
    `label_rule` (a LabelRule; needs a class map): the cell takes the majority or the highest-priority class of its points -- the
    rasteriser launch of every prepare path is then kd_bev_rasterize_vote, after the same table remap."""

    def __init__(self, root: str, scene_ids: List[str], image_size: Tuple[int, int] = (256, 256),
                 grid_size: Tuple[int, int] = (64, 64), max_points: int = 5000, verbose: bool = True,
                 device_resize: bool = False, label_rule: LabelRule = None, class_map=None):
        self.root, self.scene_ids = root, scene_ids
        self.image_size, self.grid_size, self.max_points = image_size, grid_size, max_points
        self.device_resize = bool(device_resize)
        self.set_class_map(class_map)
        self.set_label_rule(label_rule)
        self.pc_range = (-50, 50, -50, 50)
        self.samples = self._index_scenes(verbose=verbose)
        if verbose:
            print(f"Indexed {len(self.samples)} valid samples from {len(scene_ids)} scenes")

    def _index_scenes(self, verbose: bool = True):
        found = []
        for sid in self.scene_ids:
            dirs = {"image": os.path.join(self.root, sid, "camera", "front_camera"),
                    "lidar": os.path.join(self.root, sid, "lidar"),
                    "semseg": os.path.join(self.root, sid, "annotations", "semseg")}
            if not all(os.path.isdir(d) for d in dirs.values()):
                continue
            frames = sorted(f[:-4] for f in os.listdir(dirs["image"]) if f.endswith(".jpg"))
            usable = 0
            for fid in frames:
                paths = {"image": os.path.join(dirs["image"], fid + ".jpg"), "lidar": os.path.join(dirs["lidar"], fid + ".pkl"),
                         "semseg": os.path.join(dirs["semseg"], fid + ".pkl")}
                if all(os.path.exists(p) for p in paths.values()):
                    found.append({"scene": sid, "frame": fid, **paths})
                    usable += 1
            if verbose:
                print(f"Scene {sid}: {usable}/{len(frames)} frames usable")
        return found

    def __len__(self):
        return len(self.samples)

    class_table = _table_dev = None                # a subclass with its own constructor stays 2-class

    def set_class_map(self, class_map):
        """None: the 2-class drivable remap inside the rasteriser (the default).  Else validated here (ValueError)."""
        self.class_table = None if class_map is None else class_map_table(class_map)
        self._table_dev = None

    label_rule = _rank_dev = None                  # a subclass with its own constructor keeps the first-point rule

    def set_label_rule(self, label_rule):
        """None: a cell takes the class of its first labelled point (the default).  A LabelRule: majority or priority per cell, on
        every prepare path; it needs a class map (under the 2-class drivable remap every rule gives the same mask) and is checked
        against the map's classes here (ValueError)."""
        if label_rule is not None:
            if not isinstance(label_rule, LabelRule):
                raise ValueError(f"label_rule must be a LabelRule or None, got {type(label_rule).__name__}")
            if self.class_table is None:
                raise ValueError("label_rule needs a class_map: with the 2-class drivable labels every rule gives the same mask")
            label_rule.ranks(self._vote_classes())
        self.label_rule, self._rank_dev = label_rule, None

    def _vote_classes(self) -> int:
        return max(2, self.num_classes)            # a map of background alone still has the 2 classes the kernel starts at

    def __getstate__(self):                        # a pickled copy (spawned DataLoader workers) carries no device tensor
        return {**self.__dict__, "_table_dev": None, "_rank_dev": None}

    @property
    def num_classes(self) -> int:
        return 2 if self.class_table is None else int(self.class_table.max()) + 1

    def _labels(self, cls: torch.Tensor, n: int, s: int):
        """(labels, remap flag) for kd_bev_rasterize on stream `s`: the raw ids and the drivable remap, or -- with a class map --
        the table-remapped ids (one more launch) and no remap."""
        if self.class_table is None:
            return cls, 1
        if self._table_dev is None:                # copied once, on the first batch (the workers never touch the GPU)
            self._table_dev = torch.from_numpy(self.class_table).cuda()
        out = torch.empty_like(cls)
        lib.call("kd_semantic_remap_table", P(cls), n, P(self._table_dev), self._table_dev.numel(), P(out), s)
        return out, 0

    def _raster_ws_bytes(self, B: int, GH: int, GW: int) -> int:
        if self.label_rule is None:
            return lib.kd_bev_rasterize_ws_bytes(B, GH, GW)
        return lib.kd_bev_rasterize_vote_ws_bytes(B, GH, GW, self._vote_classes())

    def _rasterize(self, x, y, lab, remap: int, off, B: int, n: int, GH: int, GW: int, ws, nbytes: int, seg, s: int):
        """The rasteriser launch of the batched prepare paths on stream `s`: kd_bev_rasterize, or -- with a label rule --
        kd_bev_rasterize_vote over the table-remapped classes (`ws`: at least _raster_ws_bytes(B, GH, GW) bytes)."""
        x0, x1, y0, y1 = self.pc_range
        if self.label_rule is None:
            lib.call("kd_bev_rasterize", P(x), P(y), P(lab), P(off), B, n, remap, _DRIVABLE_BITS, GH, GW, _f32(x0), _f32(x1 - x0),
                     _f32(x1), _f32(y0), _f32(y1 - y0), _f32(y1), P(ws), nbytes, P(seg), s)
            return
        if self._rank_dev is None:                 # copied once, like the table
            self._rank_dev = torch.from_numpy(self.label_rule.ranks(self._vote_classes())).cuda()
        _vote_launch(self.label_rule, self._rank_dev, self._vote_classes(), x, y, lab, off, B, n, GH, GW, self.pc_range, ws, nbytes,
                     seg, None, s)

    def load_raw(self, idx: int) -> Dict[str, object]:
        """Host I/O only (safe in DataLoader workers): decoded + resized uint8 image, float32 point columns,
        int64 raw class ids.  With `device_resize` the image is the decoded full-size frame as a torch.uint8 tensor
        (DataLoader workers hand tensors over through shared memory; the resize happens in prepare_batch*)."""
        import pandas as pd
        from PIL import Image
        s = self.samples[idx]
        img = Image.open(s["image"]).convert("RGB")
        img = torch.from_numpy(np.array(img)) if self.device_resize else img.resize(self.image_size, Image.BILINEAR)
        lidar = pd.read_pickle(s["lidar"])
        cols = {c: lidar[c].to_numpy(dtype=np.float32) for c in ("x", "y", "z", "i")}
        raw_ids = pd.read_pickle(s["semseg"])["class"].to_numpy(dtype=np.int64)
        return {"image_u8": img if self.device_resize else np.asarray(img), **cols, "class": raw_ids,
                "sample_token": f"{s['scene']}_{s['frame']}"}

    def _needs_resize(self, shape) -> bool:
        """A frame of (height, width) = shape[:2] goes through the device resize: opted in and not yet image_size."""
        return self.device_resize and (int(shape[1]), int(shape[0])) != (int(self.image_size[0]), int(self.image_size[1]))

    def _image_chw(self, img_u8) -> torch.Tensor:
        if self._needs_resize(np.shape(img_u8)):
            return resize_images_pil_bilinear(img_u8[None], self.image_size)[0]
        return image_to_chw(img_u8)

    def prepare_batch(self, raws: Sequence[Dict[str, object]], augment: Augment = None, frame_keys: Sequence[int] = None,
                      sample_seed: int = 0) -> Dict[str, object]:
        """Device stage for a list of `load_raw` results -> the collated batch the trainers consume.  With `augment`
        (and the frames' keys) the batch is transformed as in `prepare_batch_staged`, on the current stream."""
        if augment is not None:
            return self._prepare_batch_augmented(raws, augment, frame_keys, sample_seed)
        xs = [_dev(r["x"], torch.float32) for r in raws]
        ys = [_dev(r["y"], torch.float32) for r in raws]
        if self.class_table is None:
            seg = rasterize_bev_batch(xs, ys, [r["class"] for r in raws], self.grid_size, self.pc_range, remap=True)
        else:
            raw = torch.cat([_dev(r["class"], torch.int64).reshape(-1) for r in raws])
            if raw.numel() != sum(int(x.numel()) for x in xs):
                raise KDError("x, y and labels must have the same length per frame")
            lab, _ = self._labels(raw, raw.numel(), stream())
            bounds = np.concatenate([[0], np.cumsum([int(x.numel()) for x in xs])]).tolist()
            vote = {} if self.label_rule is None else {"rule": self.label_rule, "num_classes": self._vote_classes()}
            seg = rasterize_bev_batch(xs, ys, [lab[a:b] for a, b in zip(bounds[:-1], bounds[1:])], self.grid_size, self.pc_range,
                                      remap=False, **vote)
        pts = torch.stack([prepare_points(x, y, r["z"], r["i"], self.max_points) for x, y, r in zip(xs, ys, raws)])
        img = torch.stack([self._image_chw(r["image_u8"]) for r in raws])
        return {"image": img, "points": pts, "segmentation": seg, "sample_token": [r["sample_token"] for r in raws]}

    def _prepare_batch_augmented(self, raws, aug: Augment, frame_keys, sample_seed: int) -> Dict[str, object]:
        """The synchronous path under augmentation: the frames' columns are concatenated on the device, transformed in
        place by kd_points_augment_batch, then rasterised and stacked from there; the stacked images are adjusted by
        kd_image_augment_batch.  Same kernels, rows and keys as the staged path: for sweeps of at most max_points points
        the two paths give identical bits (longer sweeps are cut by torch.randperm here, by the device sampler there)."""
        B = len(raws)
        if B == 0 or frame_keys is None or len(frame_keys) != B:
            raise KDError("an augmented batch needs at least one frame and one frame key per frame")
        lens = [int(np.shape(r["x"])[0]) for r in raws]
        if any(int(np.shape(r[k])[0]) != m for r, m in zip(raws, lens) for k in ("y", "z", "i", "class")):
            raise KDError("x, y, z, i and class must have the same length per frame")
        n = sum(lens)
        ns = -(-n // 4) * 4                                    # column stride: 16-byte accesses in the kernel
        cols = torch.empty(max(4 * ns, 1), dtype=torch.float32, device="cuda")
        for c, k in enumerate("xyzi"):
            if n:
                torch.cat([_dev(r[k], torch.float32).reshape(-1) for r in raws], out=cols[c * ns:c * ns + n])
        x, y, z, w = (cols[c * ns:c * ns + n] for c in range(4))
        cls = torch.cat([_dev(r["class"], torch.int64).reshape(-1) for r in raws]) if n else torch.empty(1, dtype=torch.int64, device="cuda")
        bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        off = torch.from_numpy(bounds).cuda()
        keys = torch.from_numpy(np.asarray([_u64(k) for k in frame_keys], np.uint64).view(np.int64)).cuda()
        params = torch.from_numpy(frame_params(aug, sample_seed, frame_keys)).cuda()
        s = stream()
        _augment_launches(aug, params, x, y, z, w, off, keys, B, n, sample_seed, s)
        GH, GW = int(self.grid_size[0]), int(self.grid_size[1])
        seg = torch.empty(B, GH, GW, dtype=torch.int64, device="cuda")
        nbytes = self._raster_ws_bytes(B, GH, GW)
        ws = workspace(nbytes, seg.device)
        lab, remap = self._labels(cls, n, s)
        self._rasterize(x, y, lab, remap, off, B, n, GH, GW, ws, nbytes, seg, s)
        pts = torch.stack([prepare_points(*(v[a:b] for v in (x, y, z, w)), self.max_points)
                           for a, b in zip(bounds[:-1].tolist(), bounds[1:].tolist())])
        img = torch.stack([self._image_chw(r["image_u8"]) for r in raws])
        _augment_image_launch(aug, params, img, s)
        return {"image": img, "points": pts, "segmentation": seg, "sample_token": [r["sample_token"] for r in raws]}

    def prepare_batch_staged(self, raws: Sequence[Dict[str, object]], staging: StagingSet, side: "torch.cuda.Stream",
                             frame_keys: Sequence[int], sample_seed: int = 0, ws_holder: list = None,
                             augment: Augment = None) -> Dict[str, object]:
        """`prepare_batch` for a whole batch at once, enqueued on the stream `side`: one host-to-device copy per tensor
        from the pinned `staging` set (packed point columns, class ids, uint8 images, offsets + frame keys), then three
        launches (rasteriser, batched points, batched images -- with `device_resize` and full-size frames the image
        launch is the Pillow-exact resize; with a class map one more, the table remap ahead of the rasteriser).  Sweeps longer than max_points are cut by the device
        sampler of kd_points_prepare_batch under (`sample_seed`, frame key).  The tensors returned belong to `side`:
        a consumer on another stream waits for an event recorded after this call and tells the allocator
        (`record_stream`).  `ws_holder`: a one-element list that keeps the rasteriser's workspace of this stream.
        `augment`: one more copy (the frames' float32 [B,16] rows) and up to two more launches, kd_points_augment_batch
        ahead of the rasteriser and kd_image_augment_batch after the image launch."""
        if not torch.cuda.is_available():
            raise KDError("input preparation runs on the MI355X; there is no CPU fallback")
        B = len(raws)
        if B == 0:
            raise KDError("prepare_batch_staged needs at least one frame")
        if augment is None:
            lens, (H, W, _) = staging.fill(raws, frame_keys)
        else:                                                  # column stride a multiple of 4: 16-byte accesses in the kernel
            lens, (H, W, _) = staging.fill(raws, frame_keys, col_align=4, params=frame_params(augment, sample_seed, frame_keys))
        n, ns = sum(lens), staging.stride
        GH, GW = int(self.grid_size[0]), int(self.grid_size[1])
        ws_holder = [None] if ws_holder is None else ws_holder
        with torch.cuda.stream(side):
            cols = torch.empty(max(4 * ns, 1), dtype=torch.float32, device="cuda")
            cls = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")
            img8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
            meta = torch.empty(2 * B + 1, dtype=torch.int64, device="cuda")
            cols[:4 * ns].copy_(staging.cols[:4 * ns], non_blocking=True)
            cls[:n].copy_(staging.cls[:n], non_blocking=True)
            img8.view(-1).copy_(staging.img[:img8.numel()], non_blocking=True)
            meta.copy_(staging.meta[:2 * B + 1], non_blocking=True)
            params = None
            if augment is not None:
                params = torch.empty(B * 16, dtype=torch.float32, device="cuda")
                params.copy_(staging.aug[:B * 16], non_blocking=True)
            staging.copied = torch.cuda.Event()
            staging.copied.record(side)
            x, y, z, w = (cols[c * ns:c * ns + n] for c in range(4))
            off, keys = meta[:B + 1], meta[B + 1:]
            seg = torch.empty(B, GH, GW, dtype=torch.int64, device="cuda")
            pts = torch.empty(B, self.max_points, 4, dtype=torch.float32, device="cuda")
            resize = self._needs_resize((H, W))
            OW, OH = (int(self.image_size[0]), int(self.image_size[1])) if resize else (W, H)
            img = torch.empty(B, 3, OH, OW, dtype=torch.float32, device="cuda")
            nbytes = self._raster_ws_bytes(B, GH, GW)
            if ws_holder[0] is None or ws_holder[0].numel() < nbytes:      # this stream's own claim table: ops.workspace()
                ws_holder[0] = torch.empty(nbytes, dtype=torch.uint8, device="cuda")   # is the compute stream's
            s = side.cuda_stream
            if augment is not None:
                _augment_launches(augment, params, x, y, z, w, off, keys, B, n, sample_seed, s)
            lab, remap = self._labels(cls, n, s)
            self._rasterize(x, y, lab, remap, off, B, n, GH, GW, ws_holder[0], nbytes, seg, s)
            lib.call("kd_points_prepare_batch", P(x), P(y), P(z), P(w), P(off), P(keys), B, n, self.max_points,
                     int(sample_seed) & 0xFFFFFFFFFFFFFFFF, P(pts), s)
            if resize:
                _resize_launch(img8, (OW, OH), img, None, s)
            else:
                lib.call("kd_image_u8hwc_to_f32chw_batch", P(img8), P(img), B, H, W, s)
            if augment is not None:
                _augment_image_launch(augment, params, img, s)
        return {"image": img, "points": pts, "segmentation": seg, "sample_token": [r["sample_token"] for r in raws]}

    def label_counts(self, indices: Sequence[int] = None, batch_size: int = 16) -> np.ndarray:
        """Host int64 [num_classes]: how many BEV cells of the frames `indices` (None: all) carry each class, under the dataset's
        class map and label rule.  The labels path alone -- remap, rasterise, kd_label_histogram per batch of frames, one copy to
        the host at the end -- and never augmented: what class_weights_from_counts (kdrt/losses.py) weighs the classes by."""
        indices = list(range(len(self))) if indices is None else [int(i) for i in indices]
        if batch_size < 1:
            raise ValueError(f"label_counts: batch_size must be at least 1, got {batch_size}")
        if not torch.cuda.is_available():
            raise KDError("input preparation runs on the MI355X; there is no CPU fallback")
        NC = self._vote_classes()
        counts = torch.zeros(NC + 1, dtype=torch.int64, device="cuda")
        GH, GW = int(self.grid_size[0]), int(self.grid_size[1])
        s = stream()
        for k in range(0, len(indices), batch_size):
            raws = [self.load_raw(i) for i in indices[k:k + batch_size]]
            B = len(raws)
            lens = [int(np.shape(r["x"])[0]) for r in raws]
            if any(int(np.shape(r[c])[0]) != m for r, m in zip(raws, lens) for c in ("y", "class")):
                raise KDError("x, y and class must have the same length per frame")
            n = sum(lens)
            x, y = (torch.cat([_dev(r[c], torch.float32).reshape(-1) for r in raws]) for c in "xy")
            cls = torch.cat([_dev(r["class"], torch.int64).reshape(-1) for r in raws])
            off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
            seg = torch.empty(B, GH, GW, dtype=torch.int64, device="cuda")
            nbytes = self._raster_ws_bytes(B, GH, GW)
            lab, remap = self._labels(cls, n, s)
            self._rasterize(x, y, lab, remap, off, B, n, GH, GW, workspace(nbytes, seg.device), nbytes, seg, s)
            lib.call("kd_label_histogram", P(seg), seg.numel(), NC, P(counts), s)
        return counts[:NC].cpu().numpy()

    def __getitem__(self, idx: int) -> Dict[str, torch.Tensor]:
        b = self.prepare_batch([self.load_raw(idx)])
        return {"image": b["image"][0], "points": b["points"][0], "segmentation": b["segmentation"][0],
                "sample_token": b["sample_token"][0]}


class _RawFrames(Dataset):
    """What the worker processes see: host I/O only."""

    def __init__(self, ds: PandaSetDataset):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, idx):
        raw = self.ds.load_raw(idx)
        raw["index"] = int(idx)                   # the dataset index: low word of the frame key of the device sampler
        return raw


class RankShardSampler(torch.utils.data.Sampler):
    """Frame indices of ONE rank of a data-parallel job.  `equal=True` (training): every rank gets exactly
    floor(n / world) frames per epoch -- the epoch's permutation (seeded by `seed + epoch`, identical on all ranks) is cut
    to a multiple of `world` and dealt round-robin -- so that, with drop_last batching, all ranks run the SAME number of
    steps and none is left waiting in a gradient all-reduce.  `equal=False` (validation: no collectives inside the
    loop): rank r takes indices r, r + world, ... of the unshuffled set; every frame is seen exactly once job-wide."""

    def __init__(self, n: int, rank: int, world: int, shuffle: bool, equal: bool, seed: int = 0):
        if not 0 <= rank < world:
            raise KDError(f"rank {rank} outside world of {world}")
        self.n, self.rank, self.world, self.shuffle, self.equal, self.seed, self.epoch = n, rank, world, shuffle, equal, seed, 0

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def _order(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            return torch.randperm(self.n, generator=g).tolist()
        return list(range(self.n))

    def __len__(self):
        if self.equal:
            return self.n // self.world
        return (self.n - self.rank + self.world - 1) // self.world

    def __iter__(self):
        order = self._order()
        if self.equal:
            order = order[: (self.n // self.world) * self.world]
        return iter(order[self.rank::self.world])


def _dist_rank_world():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _collect_before_fork(loader: DataLoader):
    """Run the cycle collector HERE before `loader` forks its worker processes.  A forked worker inherits this process's
    uncollected cyclic garbage (e.g. a finished trainer: its loss criterion closes over it), and its own collector would
    free it there -- including CUDA tensors that took part in a collective, whose release records HIP events, which a
    forked child of a process with a HIP context cannot do (the workers died with SIGSEGV at the first epoch of the
    second fusion variant under torchrun)."""
    if loader.num_workers > 0:
        gc.collect()


class _EpochLoader:
    """DataLoader + `set_epoch` forwarded to a RankShardSampler (the trainers call it once per epoch)."""

    def __init__(self, loader: DataLoader, sampler=None):
        self._loader, self._sampler = loader, sampler
        self.dataset, self.batch_size = loader.dataset, loader.batch_size

    def set_epoch(self, epoch: int):
        if self._sampler is not None:
            self._sampler.set_epoch(epoch)

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        _collect_before_fork(self._loader)
        return iter(self._loader)


class DeviceBatchLoader:
    """DataLoader over raw host frames (any num_workers) + per-batch device preparation in the consumer.
    With `world > 1` the frames are sharded over ranks (RankShardSampler); the training loader then also drops the
    ragged last batch, so every rank runs the same number of steps.

    `prefetch = 0`: each batch is prepared synchronously on the current stream between two steps (`prepare_batch`).
    `prefetch >= 1`: that many prepared batches are kept in flight on a side stream, each with its own pinned staging
    set (`prepare_batch_staged`), so batch k+1 is copied and prepared while the caller's step consumes batch k.  The
    yielded tensors are safe on the caller's current stream as they are: that stream waits for the side stream's event
    and the allocator is told of the cross-stream use.  Sweeps longer than max_points are then cut by the device sampler
    under the frame key (epoch << 32) | dataset index and `sample_seed`: a frame gets a new subset every epoch
    (`set_epoch`, else one epoch per `__iter__`) and the same one whenever (sample_seed, epoch, index) recur, on any
    rank and in any batch.

    `device_resize` (None: the dataset's own setting): the workers only decode and the full-size uint8 frames are
    resized on the device (kd_image_resize_bilinear_batch, Pillow's bytes); the pinned staging set then holds the
    full-size frames of a batch (6.2 MB per 1920x1080 frame).

    `augment` (an `Augment`, its parse string, or None = off): training loaders only -- on a validation loader it is a
    KDError.  Every batch is then transformed on the device (see the module docstring), on either path, each frame by
    the row that `frame_params` draws for (`sample_seed`, (epoch << 32) | dataset index): a new transform every epoch, the
    same one whenever the triple recurs.  Off: no extra launch, copy or bit."""

    def __init__(self, ds: PandaSetDataset, batch_size: int, shuffle: bool, num_workers: int, to_cpu: bool = False,
                 rank: int = 0, world: int = 1, train: bool = None, prefetch: int = 0, sample_seed: int = 0,
                 device_resize: bool = None, augment=None):
        if prefetch < 0:
            raise KDError(f"prefetch must be >= 0, got {prefetch}")
        if device_resize is not None:            # None: as the dataset was built; the workers' load_raw reads the flag
            ds.device_resize = bool(device_resize)
        self.dataset = ds
        self.batch_size = batch_size
        self.to_cpu = to_cpu
        self.prefetch, self.sample_seed = int(prefetch), int(sample_seed)
        self._epoch, self._epoch_set = -1, None
        self._side = self._staging = None
        self._ws = [None]
        train = shuffle if train is None else train
        if augment is not None and not train:
            raise KDError("augment is for training loaders only: a validation loader never augments")
        self.augment = as_augment(augment)
        self._sampler = None
        if world > 1:
            self._sampler = RankShardSampler(len(ds), rank, world, shuffle=shuffle, equal=train)
            self._loader = DataLoader(_RawFrames(ds), batch_size=batch_size, sampler=self._sampler, num_workers=num_workers,
                                      collate_fn=list, drop_last=train)
        else:
            self._loader = DataLoader(_RawFrames(ds), batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                                      collate_fn=list)

    def set_epoch(self, epoch: int):
        self._epoch_set = int(epoch)
        if self._sampler is not None:
            self._sampler.set_epoch(epoch)

    def __len__(self):
        return len(self._loader)

    def __iter__(self):
        self._epoch, self._epoch_set = (self._epoch + 1 if self._epoch_set is None else self._epoch_set), None
        _collect_before_fork(self._loader)
        if self.prefetch > 0:
            yield from self._iter_prefetch(self._epoch)
            return
        for raws in self._loader:
            if self.augment is None:
                b = self.dataset.prepare_batch(raws)
            else:
                b = self.dataset.prepare_batch(raws, self.augment, self._frame_keys(self._epoch, raws), self.sample_seed)
            if self.to_cpu:                 # for host-side analysis scripts that call .numpy() on the batch tensors
                b = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}
            yield b

    @staticmethod
    def _frame_keys(epoch: int, raws) -> List[int]:
        return [(epoch << 32) | (int(r["index"]) & 0xFFFFFFFF) for r in raws]

    def _deliver(self, item):
        """Hand a batch prepared on the side stream to the caller's current stream."""
        b, ready = item
        cur = torch.cuda.current_stream()
        cur.wait_event(ready)
        for v in b.values():
            if torch.is_tensor(v):
                v.record_stream(cur)
        if self.to_cpu:
            b = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in b.items()}
        return b

    def _iter_prefetch(self, epoch: int):
        if not torch.cuda.is_available():
            raise KDError("input preparation runs on the MI355X; there is no CPU fallback")
        if self._side is None:
            self._side = torch.cuda.Stream()
            self._staging = [StagingSet() for _ in range(self.prefetch)]
        side, inflight, k = self._side, deque(), 0
        try:
            for raws in self._loader:
                keys = self._frame_keys(epoch, raws)
                b = self.dataset.prepare_batch_staged(raws, self._staging[k % self.prefetch], side, keys, self.sample_seed, self._ws,
                                                      augment=self.augment)
                ready = torch.cuda.Event()
                ready.record(side)
                inflight.append((b, ready))
                k += 1
                if len(inflight) > self.prefetch:
                    yield self._deliver(inflight.popleft())
            while inflight:
                yield self._deliver(inflight.popleft())
        finally:
            # left early (break, exception) or done: nothing stays pending on the side stream or in the staging sets
            inflight.clear()
            side.synchronize()


class SyntheticPandaSet(Dataset):
    """`num_classes` (default 2: the frames as they always were): labels drawn in [0, num_classes - 1], background (0) at the same
    ~87 % and the other classes sharing the rest evenly."""

    def __init__(self, n_frames=64, num_points=5000, image_size=256, bev_size=64, seed=0, pad_tail=250, num_classes=2):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 2 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"SyntheticPandaSet: num_classes must be an integer in [2, {MAX_CLASSES}], got {num_classes!r}")
        self.n, self.N, self.hw, self.g, self.seed, self.pad = n_frames, num_points, image_size, bev_size, seed, pad_tail
        self.num_classes = num_classes

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        pts = torch.randn(self.N, 4, generator=g)
        pts[:, :2] *= 40.0
        pts[:, 2] = pts[:, 2] * 4.0 - 1.0
        pts[:, 3] = torch.sigmoid(pts[:, 3])
        if self.pad:
            pts[self.N - self.pad:] = 0.0
        seg = (torch.rand(self.g, self.g, generator=g) < 0.13).long()        # ~87 % background (real data)
        img = torch.rand(3, self.hw, self.hw, generator=g)
        if self.num_classes > 2:                   # the last draw: image, points and the foreground mask keep their values
            seg = seg * torch.randint(1, self.num_classes, (self.g, self.g), generator=g)
        return {"image": img, "points": pts, "segmentation": seg, "sample_token": f"synthetic_{i:06d}"}


class SyntheticRawPandaSet(PandaSetDataset):
    """In-memory raw source of the real shape, for measurement and tests without files: `load_raw(i)` returns a seeded
    dictionary with an uint8 image, float32 x / y / z / i columns of a chosen sweep length and int64 raw class ids in
    PandaSet's range (0..42).  `sweep_points`: one length or a sequence cycled over the frames (0 = an empty sweep);
    `nan_frames`: indices whose first points get NaN coordinates; `unique`: frames i and i + unique share their arrays
    (generated once and kept), so a long run does not time the generator.  `source_size` (width, height; None: frames are
    born at image_size, as before): the camera frame is generated at that size, and `load_raw` serves it whole as a
    torch.uint8 tensor under `device_resize`, else resized on the host by Pillow as the real reader does."""

    def __init__(self, n_frames: int = 64, sweep_points=169000, image_size: Tuple[int, int] = (256, 256),
                 grid_size: Tuple[int, int] = (64, 64), max_points: int = 5000, seed: int = 0, nan_frames: Sequence[int] = (),
                 unique: int = None, source_size: Tuple[int, int] = None, device_resize: bool = False,
                 label_rule: LabelRule = None, class_map=None):
        self.root, self.scene_ids = None, []
        self.image_size, self.grid_size, self.max_points = image_size, grid_size, max_points
        self.source_size, self.device_resize = source_size, bool(device_resize)
        self.set_class_map(class_map)
        self.set_label_rule(label_rule)
        self.pc_range = (-50, 50, -50, 50)
        self.seed, self.nan_frames = seed, set(int(i) for i in nan_frames)
        self.sweeps = [int(sweep_points)] if np.isscalar(sweep_points) else [int(v) for v in sweep_points]
        self.unique = n_frames if unique is None else int(unique)
        self.samples = [{"scene": "synthetic", "frame": f"{i:06d}"} for i in range(n_frames)]
        self._made = {}

    def load_raw(self, idx: int) -> Dict[str, object]:
        u = idx % self.unique
        if u not in self._made:
            r = np.random.RandomState(self.seed * 100003 + u)
            n = self.sweeps[u % len(self.sweeps)]
            x, y = (r.randn(n) * 40.0).astype(np.float32), (r.randn(n) * 40.0).astype(np.float32)
            z = (r.randn(n) * 4.0 - 1.0).astype(np.float32)
            inten = r.randint(0, 256, n).astype(np.float32)
            if u in self.nan_frames and n >= 2:
                x[0], y[1] = np.nan, np.nan
            fw, fh = self.image_size if self.source_size is None else self.source_size
            self._made[u] = {"image_u8": r.randint(0, 256, (fh, fw, 3)).astype(np.uint8),
                             "x": x, "y": y, "z": z, "i": inten, "class": r.randint(0, 43, n).astype(np.int64)}
        raw = {**self._made[u], "sample_token": f"synthetic_{idx:06d}"}
        if self.source_size is not None:
            if self.device_resize:
                raw["image_u8"] = torch.from_numpy(raw["image_u8"])
            else:
                from PIL import Image
                raw["image_u8"] = np.asarray(Image.fromarray(raw["image_u8"]).resize(self.image_size, Image.BILINEAR))
        return raw


def create_pandaset_dataloaders(root: str, train_scenes: List[str], val_scenes: List[str], batch_size: int = 4,
                                num_workers: int = 0, verbose: bool = True, to_cpu: bool = None, prefetch: int = None,
                                device_resize: bool = None, augment=None, label_rule: LabelRule = None, class_map=None):
    """Reference signature (pandaset_dataset.py:144-160) plus `to_cpu`: batches stay on the GPU by default (the trainers'
    `.to(device)` is then free); to_cpu=True (or KD_LOADER_TO_CPU=1) returns host tensors for the reference's analysis
    scripts, which call `.numpy()` on them (test_dataset_distribution.py:22, verify_2class_distribution.py).
    `prefetch` (None: KD_LOADER_PREFETCH, default 0): batches prepared ahead of the step on a side stream, see
    DeviceBatchLoader; KD_LOADER_SAMPLE_SEED seeds its device sampler.  `device_resize` (None: KD_LOADER_DEVICE_RESIZE=1,
    default off): the workers only decode and the bilinear resize runs on the device with Pillow's bytes.  `augment` (an
    `Augment`, or its parse form "rot=5,flip=0.5,..."; None: KD_LOADER_AUGMENT, empty or unset = off): opt-in training
    augmentation on the device, see DeviceBatchLoader; it goes to the TRAINING loader only.  The synthetic fallback serves
    ready-made tensors and ignores the setting.  `class_map` (None: the 2-class drivable labels): raw id -> class index for
    multi-class labels, see PandaSetDataset (ValueError if malformed); the synthetic fallback then draws labels in the map's
    range of classes.  `label_rule` (None: a cell takes the class of its first labelled point): a LabelRule, majority or priority per
    cell, for both datasets; it needs `class_map` (ValueError without one, or when it names a class outside the map's).  The synthetic
    fallback serves ready-made masks and only validates it."""
    if to_cpu is None:
        to_cpu = os.environ.get("KD_LOADER_TO_CPU") == "1"
    if prefetch is None:
        prefetch = int(os.environ.get("KD_LOADER_PREFETCH", "0"))
    if device_resize is None:
        device_resize = os.environ.get("KD_LOADER_DEVICE_RESIZE") == "1"
    if augment is None:
        augment = os.environ.get("KD_LOADER_AUGMENT", "")
    augment = as_augment(augment)
    table = None if class_map is None else class_map_table(class_map)
    if label_rule is not None:
        if not isinstance(label_rule, LabelRule):
            raise ValueError(f"label_rule must be a LabelRule or None, got {type(label_rule).__name__}")
        if table is None:
            raise ValueError("label_rule needs a class_map: with the 2-class drivable labels every rule gives the same mask")
        label_rule.ranks(max(2, int(table.max()) + 1))
    pf = {"prefetch": prefetch, "sample_seed": int(os.environ.get("KD_LOADER_SAMPLE_SEED", "0"))}
    # under torch.distributed (one process per GPU) the FRAMES are sharded over ranks, equal counts per rank for training
    rank, world = _dist_rank_world()
    if os.path.isdir(root):
        rule = {} if label_rule is None else {"label_rule": label_rule}
        train_ds = PandaSetDataset(root, train_scenes, verbose=verbose, device_resize=device_resize, class_map=class_map, **rule)
        val_ds = PandaSetDataset(root, val_scenes, verbose=verbose, device_resize=device_resize, class_map=class_map, **rule)
        return (DeviceBatchLoader(train_ds, batch_size, shuffle=True, num_workers=num_workers, to_cpu=to_cpu, rank=rank, world=world,
                                  augment=augment, **pf),
                DeviceBatchLoader(val_ds, batch_size, shuffle=False, num_workers=num_workers, to_cpu=to_cpu, rank=rank, world=world, **pf))
    if verbose:
        print(f"[data] '{root}' not found: serving synthetic PandaSet-shaped frames")
        if augment is not None:
            print("[data] the synthetic frames are ready-made tensors: the augment setting is ignored")
    nc = {} if table is None else {"num_classes": max(2, int(table.max()) + 1)}
    train = SyntheticPandaSet(n_frames=max(8, 8 * len(train_scenes)), seed=1, **nc)
    val = SyntheticPandaSet(n_frames=max(4, 4 * len(val_scenes)), seed=2, **nc)
    if world > 1:
        ts = RankShardSampler(len(train), rank, world, shuffle=True, equal=True)
        vs = RankShardSampler(len(val), rank, world, shuffle=False, equal=False)
        return (_EpochLoader(DataLoader(train, batch_size=batch_size, sampler=ts, num_workers=num_workers, pin_memory=True, drop_last=True), ts),
                _EpochLoader(DataLoader(val, batch_size=batch_size, sampler=vs, num_workers=num_workers, pin_memory=True), vs))
    return (DataLoader(train, batch_size=batch_size, shuffle=True, num_workers=num_workers, pin_memory=True, drop_last=True),
            DataLoader(val, batch_size=batch_size, shuffle=False, num_workers=num_workers, pin_memory=True))
