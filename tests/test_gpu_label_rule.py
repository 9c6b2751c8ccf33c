"""kd_bev_rasterize_vote (majority / priority per BEV cell) and kd_label_histogram through the C ABI, and the label rule through
the loader.  Everything is integers: masks, votes and histograms are compared with `array_equal` against the numpy mirror of
tests/_label_rule_ref.py.  Every output starts as a sentinel, and the workspace carries a guard region that must stay intact."""
import numpy as np
import pytest
import torch

import _label_rule_ref as R
import data_oracle as D

pytestmark = pytest.mark.gpu

RANGE = (-50, 50, -50, 50)
SENT, GUARD = -77, 4096


def _lib():
    from kdrt.lib import KDError, lib
    from kdrt.ops import P, stream
    return lib, P, stream, KDError


def _f32(v):
    return float(np.float32(v))


def _pack(xs, ys, cs):
    x = torch.from_numpy(np.concatenate([np.asarray(v, np.float32) for v in xs])).cuda()
    y = torch.from_numpy(np.concatenate([np.asarray(v, np.float32) for v in ys])).cuda()
    c = torch.from_numpy(np.concatenate([np.asarray(v, np.int64) for v in cs])).cuda()
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(v) for v in xs])]).astype(np.int64)).cuda()
    return x, y, c, off


def _vote(xs, ys, cs, NC, rule, rank=None, min_points=1, grid=(8, 12), pc_range=RANGE, votes=True):
    """-> (mask [B, H, W] int64, votes [B, H, W] int32 or None) as numpy, after the guard check"""
    lib, P, stream, _ = _lib()
    B, (H, W) = len(xs), grid
    x, y, c, off = _pack(xs, ys, cs)
    x0, x1, y0, y1 = pc_range
    nbytes = lib.kd_bev_rasterize_vote_ws_bytes(B, H, W, NC)
    assert nbytes == B * H * W * (4 if NC <= 4 else 8 if NC <= 8 else 16) * 4
    ws = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    mask = torch.full((B, H, W), SENT, dtype=torch.int64, device="cuda")
    vt = torch.full((B, H, W), SENT, dtype=torch.int32, device="cuda") if votes else None
    rk = None if rank is None else torch.from_numpy(np.asarray(rank, np.int32)).cuda()
    lib.call("kd_bev_rasterize_vote", P(x), P(y), P(c), P(off), B, x.numel(), NC, rule, P(rk), min_points, H, W, _f32(x0),
             _f32(x1 - x0), _f32(x1), _f32(y0), _f32(y1 - y0), _f32(y1), P(ws), nbytes, P(mask), P(vt), stream())
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the guard region after the workspace was written"
    return mask.cpu().numpy(), None if vt is None else vt.cpu().numpy()


def _first(xs, ys, cs, grid=(8, 12), pc_range=RANGE):
    """kd_bev_rasterize with remap = 0: the shipped first-point rule over class indices"""
    lib, P, stream, _ = _lib()
    B, (H, W) = len(xs), grid
    x, y, c, off = _pack(xs, ys, cs)
    x0, x1, y0, y1 = pc_range
    nbytes = lib.kd_bev_rasterize_ws_bytes(B, H, W)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    mask = torch.full((B, H, W), SENT, dtype=torch.int64, device="cuda")
    lib.call("kd_bev_rasterize", P(x), P(y), P(c), P(off), B, x.numel(), 0, 0, H, W, _f32(x0), _f32(x1 - x0), _f32(x1), _f32(y0),
             _f32(y1 - y0), _f32(y1), P(ws), nbytes, P(mask), stream())
    torch.cuda.synchronize()
    return mask.cpu().numpy()


def _scene(seed, lens, NC, sigma=30.0, hi=None):
    """ragged frames with every class 0 .. hi-1 (default NC) drawn evenly"""
    r = np.random.RandomState(seed)
    xs = [(r.randn(n) * sigma).astype(np.float32) for n in lens]
    ys = [(r.randn(n) * sigma).astype(np.float32) for n in lens]
    cs = [r.randint(0, hi or NC, n).astype(np.int64) for n in lens]
    return xs, ys, cs


def _check(xs, ys, cs, NC, rank=None, min_points=1, grid=(8, 12), pc_range=RANGE):
    out = {}
    for rule in (R.MAJORITY, R.PRIORITY):
        m, v = _vote(xs, ys, cs, NC, rule, rank, min_points, grid, pc_range)
        wm, wv = R.rasterize_vote_batch(xs, ys, cs, grid, pc_range, NC, rule, rank, min_points)
        assert np.array_equal(m, wm), (rule, np.argwhere(m != wm)[:5])
        assert np.array_equal(v, wv), (rule, np.argwhere(v != wv)[:5])
        assert v.dtype == np.int32 and m.dtype == np.int64
        out[rule] = (m, v)
    return out


# ---- shapes -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("NC", [2, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("grid", [(1, 1), (8, 12), (64, 64), (200, 200)], ids=lambda g: "%dx%d" % g)
def test_shapes_and_class_buckets(grid, NC):
    """B = 3 with an empty frame and a one-point frame (200 x 200: one frame); ranks drawn with repeats, so every tie level occurs"""
    lens = [6000] if grid == (200, 200) else [2500, 0, 1]
    xs, ys, cs = _scene(NC * 10 + grid[0], lens, NC)
    rank = np.random.RandomState(NC).randint(-2, 3, NC)
    out = _check(xs, ys, cs, NC, rank, 1, grid)
    m, v = out[R.MAJORITY]
    assert 1 <= m.max() <= NC - 1 and m.min() >= 0 and v.max() >= 1
    if len(lens) == 3:
        assert m[1].sum() == 0 and v[1].sum() == 0 and v[2].sum() == (1 if cs[2][0] != 0 and abs(xs[2][0]) <= 50 and abs(ys[2][0]) <= 50 else 0)
    # the votes are optional
    m2, none = _vote(xs, ys, cs, NC, R.MAJORITY, rank, 1, grid, votes=False)
    assert none is None and np.array_equal(m2, m)


def test_no_points_at_all():
    e = np.zeros(0)
    for B in (1, 3):
        m, v = _vote([e] * B, [e] * B, [e] * B, 8, R.MAJORITY, grid=(8, 12))
        assert m.shape == (B, 8, 12) and not m.any() and not v.any()


def test_refusals_leave_the_mask_alone():
    lib, P, stream, _ = _lib()
    xs, ys, cs = _scene(1, [50], 4)
    x, y, c, off = _pack(xs, ys, cs)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    mask = torch.full((1, 8, 12), SENT, dtype=torch.int64, device="cuda")
    votes = torch.full((1, 8, 12), SENT, dtype=torch.int32, device="cuda")
    def call(NC, rule, min_points=1):
        return lib.kd_bev_rasterize_vote(P(x), P(y), P(c), P(off), 1, 50, NC, rule, None, min_points, 8, 12, -50.0, 100.0, 50.0, -50.0,
                                         100.0, 50.0, P(ws), ws.numel(), P(mask), P(votes), stream())
    assert call(17, 1) == -4 and b"num_classes=17" in lib.kd_last_error_string()
    assert call(4, 0) == -1 and b"kd_bev_rasterize" in lib.kd_last_error_string()
    assert call(4, 1, min_points=0) == -1
    torch.cuda.synchronize()
    assert bool((mask == SENT).all()) and bool((votes == SENT).all())
    assert call(4, 1) == 0
    torch.cuda.synchronize()
    assert not bool((mask == SENT).any())


# ---- range and class edges ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("NC", [4, 7, 16])
def test_range_and_class_edges(NC):
    lo, hi = np.float32(-50), np.float32(50)
    edge = np.array([lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf)), np.nan, np.inf, -np.inf,
                     np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(0)), 0.0, -0.0, 49.999, 12.5], np.float32)
    bad_cls = np.array([-1, 0, NC, 1 << 40, -(1 << 40), NC + 1, 1 << 31, (1 << 32) + 1], np.int64)     # (1 << 32) + 1 is not class 1
    r = np.random.RandomState(NC)
    x = np.concatenate([np.repeat(edge, len(edge)), r.choice(edge, 400), (r.randn(400) * 40).astype(np.float32)])
    y = np.concatenate([np.tile(edge, len(edge)), r.choice(edge, 400), (r.randn(400) * 40).astype(np.float32)])
    c = r.randint(1, NC, x.size).astype(np.int64)
    where = r.rand(x.size) < 0.35
    c[where] = r.choice(bad_cls, int(where.sum()))
    out = _check([x, x[::-1].copy()], [y, y.copy()], [c, c.copy()], NC, None, 1, (8, 12))
    assert out[R.MAJORITY][1].sum() == sum(int(R.cell_counts(xx, y, c, (8, 12), RANGE, NC).max(1).sum()) for xx in (x, x[::-1]))
    # a range that is not symmetric and not the grid's multiple
    _check([x], [y], [c], NC, None, 1, (5, 7), (-12.5, 50, -50, 0.25))


# ---- ties ---------------------------------------------------------------------------------------------------------------------

def _cells_scene(spec, grid=(2, 3)):
    """spec: one [(class, count), ...] list per cell of a 2 x 3 grid -> points at the cell centres, classes interleaved"""
    H, W = grid
    xs, ys, cs = [], [], []
    for k, cell in enumerate(spec):
        row, col = divmod(k, W)
        # cell = trunc((v + 50) / 100 * (n - 1)): v = -50 + 100 * (i + 0.5) / (n - 1) lands in cell i for i < n - 1
        px = -50 + 100 * (col + 0.5) / (W - 1) if col < W - 1 else 50.0
        py = -50 + 100 * (row + 0.5) / (H - 1) if row < H - 1 else 50.0
        for cl, cnt in cell:
            xs += [px] * cnt; ys += [py] * cnt; cs += [cl] * cnt
    order = np.random.RandomState(len(cs)).permutation(len(cs))
    return (np.asarray(xs, np.float32)[order], np.asarray(ys, np.float32)[order], np.asarray(cs, np.int64)[order])


TIES = [[(1, 4), (2, 4), (3, 1)],          # equal counts of 1 and 2; 3 has the highest rank but fewer points
        [(2, 5), (3, 5), (4, 5)],          # a three-way tie
        [(1, 2), (3, 7), (4, 7)],          # ranks of 3 and 4 equal and the count ties too -> the smaller class (majority)
        [(4, 9), (1, 1)],                  # priority: a single point of the top rank wins at min_points = 1
        [(2, 6), (3, 5), (1, 2)],          # min_points moves the winner 2 -> (5 < min) ... see below
        []]                                # an empty cell


def test_ties_by_rank_then_class_and_priority_by_count():
    x, y, c = _cells_scene(TIES)
    rank = [0, 9, 1, 5, 5]                                                    # NC = 5
    out = _check([x], [y], [c], 5, rank, 1, (2, 3))
    assert out[R.MAJORITY][0].reshape(-1).tolist() == [1, 3, 3, 4, 2, 0]      # 1 outranks 2; 3 = 4 outrank 2; 3 before 4; count; count
    assert out[R.MAJORITY][1].reshape(-1).tolist() == [4, 5, 7, 9, 6, 0]
    assert out[R.PRIORITY][0].reshape(-1).tolist() == [1, 3, 1, 1, 1, 0]      # rank 9 wherever class 1 has a point
    assert out[R.PRIORITY][1].reshape(-1).tolist() == [4, 5, 2, 1, 2, 0]
    flat = _check([x], [y], [c], 5, None, 1, (2, 3))                          # no ranks: counts, then the smaller class
    assert flat[R.MAJORITY][0].reshape(-1).tolist() == [1, 2, 3, 4, 2, 0]
    assert np.array_equal(flat[R.MAJORITY][0], flat[R.PRIORITY][0])


@pytest.mark.parametrize("min_points, majority, priority", [(1, [1, 3, 3, 4, 2, 0], [1, 3, 1, 1, 1, 0]),
                                                            (2, [1, 3, 3, 4, 2, 0], [1, 3, 1, 4, 1, 0]),
                                                            (5, [0, 3, 3, 4, 2, 0], [0, 3, 3, 4, 3, 0])])
def test_min_points_moves_the_winner_to_the_runner_up_and_then_to_background(min_points, majority, priority):
    x, y, c = _cells_scene(TIES)
    out = _check([x], [y], [c], 5, [0, 9, 1, 5, 5], min_points, (2, 3))
    assert out[R.MAJORITY][0].reshape(-1).tolist() == majority
    assert out[R.PRIORITY][0].reshape(-1).tolist() == priority


# ---- counters and run merging -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block", [1, 63, 64, 65, 4096])
def test_one_hot_cell_counts_exactly(block):
    """70 001 points of class 2 and 70 000 of class 1 in ONE cell, interleaved in runs of `block`: 16-bit counters would wrap and a
    run length that is off by one at a wave edge would change the winner or the votes"""
    na, nb, parts = 70001, 70000, []
    while na or nb:
        t = min(block, na); parts.append(np.full(t, 2, np.int64)); na -= t
        t = min(block, nb); parts.append(np.full(t, 1, np.int64)); nb -= t
    c = np.concatenate(parts)
    assert c.size == 140001 and int((c == 2).sum()) == 70001
    x = np.full(c.size, 3.0, np.float32)
    y = np.full(c.size, -7.0, np.float32)
    for NC in (3, 16):
        m, v = _vote([x], [y], [c], NC, R.MAJORITY, grid=(8, 12))
        assert int(v.sum()) == 70001 and int(v.max()) == 70001 and int(m.max()) == 2 and int((m != 0).sum()) == 1
        m, v = _vote([x], [y], [c], NC, R.PRIORITY, [0, 1] + [0] * (NC - 2), grid=(8, 12))
        assert int(v.sum()) == 70000 and int(m.max()) == 1 and int((m != 0).sum()) == 1
        m, v = _vote([x], [y], [c], NC, R.MAJORITY, min_points=70001, grid=(8, 12))
        assert int(v.sum()) == 70001 and int(m.max()) == 2
        m, v = _vote([x], [y], [c], NC, R.MAJORITY, min_points=70002, grid=(8, 12))
        assert not m.any() and not v.any()


@pytest.mark.parametrize("first", [1, 63, 64, 65])
def test_a_run_ends_at_a_frame_boundary(first):
    """the last points of frame 0 and the first of frame 1 share cell and class; the boundary falls inside or on the edge of a wave"""
    n = 200
    x, y, c = np.full(n, 10.0, np.float32), np.full(n, 10.0, np.float32), np.full(n, 3, np.int64)
    xs, ys, cs = [x[:first], x[first:]], [y[:first], y[first:]], [c[:first], c[first:]]
    out = _check(xs, ys, cs, 4, None, 1, (8, 12))
    v = out[R.MAJORITY][1]
    assert int(v[0].sum()) == first and int(v[1].sum()) == n - first
    # three frames, the middle one empty: offsets repeat
    out = _check([x[:first], x[:0], x[first:]], [y[:first], y[:0], y[first:]], [c[:first], c[:0], c[first:]], 4, None, 1, (8, 12))
    assert [int(f.sum()) for f in out[R.MAJORITY][1]] == [first, 0, n - first]


@pytest.mark.parametrize("at", [1, 31, 63, 64, 65])
def test_a_run_is_broken_by_a_point_that_counts_nowhere(at):
    n = 192
    for kind in ("class 0", "out of range", "NaN", "class NC", "another class", "another cell"):
        x, y, c = np.full(n, -20.0, np.float32), np.full(n, 33.0, np.float32), np.full(n, 2, np.int64)
        if kind == "class 0":
            c[at] = 0
        elif kind == "out of range":
            x[at] = 50.001
        elif kind == "NaN":
            y[at] = np.nan
        elif kind == "class NC":
            c[at] = 6
        elif kind == "another class":
            c[at] = 5
        else:
            x[at] = 20.0
        out = _check([x], [y], [c], 6, None, 1, (8, 12))
        v = out[R.MAJORITY][1]
        assert int(v.max()) == n - 1 and int(v.sum()) == (n if kind == "another cell" else n - 1), kind


# ---- agreement with the shipped rule ------------------------------------------------------------------------------------------

def test_one_class_per_cell_equals_kd_bev_rasterize_after_the_table_remap():
    lib, P, stream, _ = _lib()
    grid, NC = (16, 16), 8
    r = np.random.RandomState(5)
    table = np.zeros(43, np.int64)
    table[2:] = (np.arange(2, 43) * 5) % NC
    xs, ys, raws = [], [], []
    for n in (1500, 0, 700):
        x, y = (r.randn(n) * 30).astype(np.float32), (r.randn(n) * 30).astype(np.float32)
        keep, row, col = D.bev_cells(x, y, grid, RANGE)
        cell_raw = r.randint(0, 43, grid[0] * grid[1])                 # one raw id per cell, some of them background
        raw = r.choice([0, 1, 50, -3], n).astype(np.int64)            # elsewhere: ids that map to background
        raw[keep] = np.where(r.rand(int(keep.sum())) < 0.8, cell_raw[row * grid[1] + col], raw[keep])
        xs.append(x); ys.append(y); raws.append(raw)
    flat = torch.from_numpy(np.concatenate(raws)).cuda()
    mapped = torch.empty_like(flat)
    tab = torch.from_numpy(table).cuda()
    lib.call("kd_semantic_remap_table", P(flat), flat.numel(), P(tab), 43, P(mapped), stream())
    mapped = mapped.cpu().numpy()
    cs = [mapped[:1500], mapped[1500:1500], mapped[1500:]]
    want = _first(xs, ys, cs, grid)
    assert len(np.unique(want)) == NC
    for rule in (R.MAJORITY, R.PRIORITY):
        for rank in (None, r.randint(-5, 6, NC)):
            assert np.array_equal(_vote(xs, ys, cs, NC, rule, rank, 1, grid)[0], want)


def test_rasterize_bev_batch_with_and_without_a_rule():
    from src.data_loading.pandaset_dataset import LabelRule, rasterize_bev_batch
    xs, ys, cs = _scene(9, [800, 3, 0, 1200], 6)
    direct = _first(xs, ys, cs, (8, 12))
    for kw in ({}, {"rule": None}, {"rule": None, "num_classes": 6}):
        got = rasterize_bev_batch(xs, ys, cs, (8, 12), RANGE, **kw)
        assert torch.is_tensor(got) and np.array_equal(got.cpu().numpy(), direct)
    rank = [0, 3, 3, 1, 0, 2]
    for kind, code in (("majority", R.MAJORITY), ("priority", R.PRIORITY)):
        wm, wv = R.rasterize_vote_batch(xs, ys, cs, (8, 12), RANGE, 6, code, rank, 2)
        rule = LabelRule(kind, rank, min_points=2)
        m = rasterize_bev_batch(xs, ys, cs, (8, 12), RANGE, rule=rule, num_classes=6)
        m2, v = rasterize_bev_batch(xs, ys, cs, (8, 12), RANGE, rule=rule, num_classes=6, want_votes=True)
        assert np.array_equal(m.cpu().numpy(), wm) and np.array_equal(m2.cpu().numpy(), wm) and np.array_equal(v.cpu().numpy(), wv)
        assert not np.array_equal(wm, direct)


# ---- determinism --------------------------------------------------------------------------------------------------------------

def test_the_order_of_the_points_does_not_matter_but_it_does_under_the_first_point_rule():
    xs, ys, cs = _scene(21, [3000, 1, 2000], 8)
    r = np.random.RandomState(0)
    perms = [r.permutation(len(x)) for x in xs]
    sx, sy, sc = ([v[p] for v, p in zip(vs, perms)] for vs in (xs, ys, cs))
    rank = [0, 1, 1, 2, 0, 0, 2, 1]
    for rule in (R.MAJORITY, R.PRIORITY):
        a = _vote(xs, ys, cs, 8, rule, rank, 1, (8, 12))
        b = _vote(sx, sy, sc, 8, rule, rank, 1, (8, 12))
        c = _vote(sx, sy, sc, 8, rule, rank, 1, (8, 12))
        for u, v in zip(a + b, b + c):
            assert np.array_equal(u, v)
    # what the feature is for: the shipped rule follows the sweep's point order
    assert not np.array_equal(_first(xs, ys, cs), _first(sx, sy, sc))


# ---- kd_label_histogram -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 100003])
@pytest.mark.parametrize("NC", [1, 5, 16])
def test_label_histogram_accumulates(n, NC):
    lib, P, stream, _ = _lib()
    r = np.random.RandomState(n % 1000 + NC)
    pool = np.concatenate([np.arange(NC), np.arange(NC), [-1, -1, NC, NC + 3, 1 << 40, -(1 << 35), (1 << 32)]]).astype(np.int64)
    a, b = r.choice(pool, n), r.choice(pool, n)
    counts = torch.full((NC + 1 + 8,), 1000, dtype=torch.int64, device="cuda")          # starts non-zero; an 8-entry guard tail
    for m in (a, b):
        t = torch.from_numpy(m).cuda()
        lib.call("kd_label_histogram", P(t), n, NC, P(counts), stream())
    torch.cuda.synchronize()
    want = 1000 + R.label_histogram(a, NC) + R.label_histogram(b, NC)
    got = counts.cpu().numpy()
    assert np.array_equal(got[:NC + 1], want) and bool((got[NC + 1:] == 1000).all())
    inside = lambda m: np.bincount(m[(m >= 0) & (m < NC)], minlength=NC)
    assert np.array_equal(got[:NC] - 1000, inside(a) + inside(b)) and int(got[:NC + 1].sum()) == 1000 * (NC + 1) + 2 * n


# ---- loader -------------------------------------------------------------------------------------------------------------------

G, HW, NC8 = 16, 64, 8
CLASS_MAP = {raw: (raw * 5) % NC8 for raw in range(2, 43)}
SWEEPS = [400, 350, 0, 500]


def _dataset(rule, **kw):
    from src.data_loading.pandaset_dataset import SyntheticRawPandaSet
    return SyntheticRawPandaSet(n_frames=4, sweep_points=SWEEPS, image_size=(HW, HW), grid_size=(G, G), max_points=600, seed=3,
                                nan_frames=(1,), class_map=CLASS_MAP, label_rule=rule, **kw)


def _rules():
    from src.data_loading.pandaset_dataset import LabelRule
    return [LabelRule("majority"), LabelRule("priority", {3: 5, 6: 5, 1: 2}), LabelRule("majority", [0, 1, 0, 3, 0, 0, 3, 0], min_points=2)]


def _want_seg(ds, raws, rule):
    from src.data_loading.pandaset_dataset import class_map_table
    table = class_map_table(CLASS_MAP)
    mapped = [np.where((r["class"] >= 0) & (r["class"] < table.size), table[np.clip(r["class"], 0, table.size - 1)], 0) for r in raws]
    return R.rasterize_vote_batch([r["x"] for r in raws], [r["y"] for r in raws], mapped, (G, G), ds.pc_range, NC8, rule.code,
                                  rule.ranks(NC8), rule.min_points)[0]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_every_prepare_path_honours_the_rule(k):
    from kdrt.augment import Augment
    from src.data_loading.pandaset_dataset import StagingSet
    rule = _rules()[k]
    ds = _dataset(rule)
    raws = [ds.load_raw(i) for i in range(4)]
    keys = [7, 8, 9, 10]
    want = _want_seg(ds, raws, rule)
    first = _dataset(None).prepare_batch(raws)["segmentation"].cpu().numpy()
    assert not np.array_equal(want, first) and len(np.unique(want)) > (4 if rule.min_points == 1 else 1)
    a = ds.prepare_batch(raws)
    b = ds.prepare_batch(raws, Augment(), keys, 5)                           # all settings off: the points keep their bits
    side = torch.cuda.Stream()
    holder = [None]
    c = ds.prepare_batch_staged(raws, StagingSet(), side, keys, 5, holder)
    d = ds.prepare_batch_staged(raws, StagingSet(), side, keys, 5, holder, augment=Augment())
    side.synchronize()
    torch.cuda.synchronize()
    assert holder[0].numel() >= 4 * G * G * 8 * 4                            # the stream's own workspace, sized for the counters
    for name, got in (("prepare_batch", a), ("augmented", b), ("staged", c), ("staged + augment", d)):
        seg = got["segmentation"].cpu().numpy()
        assert seg.shape == (4, G, G) and seg.dtype == np.int64 and np.array_equal(seg, want), name
        assert torch.equal(got["points"].view(torch.int32), a["points"].view(torch.int32)) and torch.equal(got["image"], a["image"]), name
    assert int(want[2].sum()) == 0


def test_prefetching_loader_equals_the_synchronous_one_and_label_counts():
    from src.data_loading.pandaset_dataset import DeviceBatchLoader
    rule = _rules()[1]
    ds = _dataset(rule)
    sync = list(DeviceBatchLoader(ds, 2, shuffle=False, num_workers=0))
    ahead = list(DeviceBatchLoader(ds, 2, shuffle=False, num_workers=0, prefetch=1))
    assert len(sync) == len(ahead) == 2
    for s, a in zip(sync, ahead):
        assert torch.equal(s["segmentation"], a["segmentation"])
        assert torch.equal(s["points"].view(torch.int32), a["points"].view(torch.int32))        # frame 1 carries NaN coordinates
    seg = torch.cat([s["segmentation"] for s in sync]).cpu().numpy()
    assert np.array_equal(seg, _want_seg(ds, [ds.load_raw(i) for i in range(4)], rule))
    counts = ds.label_counts()
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == (NC8,)
    assert np.array_equal(counts, np.bincount(seg.reshape(-1), minlength=NC8))
    assert np.array_equal(ds.label_counts(batch_size=3), counts) and np.array_equal(ds.label_counts(batch_size=1), counts)
    assert np.array_equal(ds.label_counts([3, 0]), np.bincount(seg[[0, 3]].reshape(-1), minlength=NC8))
    # the rule shows in the histogram: the first-point labels of the same frames count differently
    first = _dataset(None)
    fseg = first.prepare_batch([first.load_raw(i) for i in range(4)])["segmentation"].cpu().numpy()
    assert np.array_equal(first.label_counts(), np.bincount(fseg.reshape(-1), minlength=NC8))
    assert not np.array_equal(first.label_counts(), counts)
    from kdrt.losses import class_weights_from_counts
    w = class_weights_from_counts(counts)
    assert len(w) == NC8 and all(np.isfinite(w)) and w == R.median_freq_weights(counts)


def test_one_kd_step_on_a_batch_labelled_by_the_rule():
    import test_gpu_multiclass_step as MS
    from kdrt.kd import KDStep
    from kdrt.losses import class_weights_from_counts
    from kdrt.optim import FusedAdamW
    ds = _dataset(_rules()[0])
    b = ds.prepare_batch([ds.load_raw(i) for i in (0, 3)])                   # the two frames without NaN coordinates or an empty sweep
    teacher, _ = MS._model("concat", 11)
    student, _ = MS._model("weighted", 12)
    student.train()
    cw = torch.tensor(class_weights_from_counts(ds.label_counts()), dtype=torch.float32).cuda()
    opt = FusedAdamW(student.parameters(), lr=1e-3, weight_decay=1e-3)
    parts = KDStep(student, teacher, opt, cw)(b["image"], b["points"], b["segmentation"])
    torch.cuda.synchronize()
    for k in ("total", "ce", "kl", "mse_cam", "mse_lidar"):
        assert bool(torch.isfinite(parts[k]).all()), k
    assert tuple(parts["logits"].shape) == (2, NC8, G, G) and bool(torch.isfinite(parts["logits"]).all())
