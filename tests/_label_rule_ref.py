"""Independent numpy mirror of kd_bev_rasterize_vote and kd_label_histogram (include/kd_hip.h carries the specification).
Cells come from oracle/data_oracle.py's bev_cells (the arithmetic the first-point oracle uses), counts from np.add.at, and the
winner of a cell from an explicit sort of (count, rank, -class) for the majority rule or (rank, count, -class) for priority."""
import numpy as np

import data_oracle as D

MAJORITY, PRIORITY = 1, 2


def cell_counts(x, y, cls, grid, pc_range, NC):
    """int64 [H * W, NC]: n_c per cell; column 0 stays 0 (the background never votes), classes outside 1 .. NC-1 count nowhere"""
    H, W = grid
    x, y, cls = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(cls, np.int64)
    keep, row, col = D.bev_cells(x, y, grid, pc_range)
    c = cls[keep]
    cell = row.astype(np.int64) * W + col
    ok = (c >= 1) & (c < NC)
    cnt = np.zeros((H * W, NC), np.int64)
    np.add.at(cnt, (cell[ok], c[ok]), 1)
    return cnt


def resolve(cnt, rule, rank=None, min_points=1):
    """(mask int64 [cells], votes int32 [cells]) from per-cell counts"""
    ncell, NC = cnt.shape
    rank = np.zeros(NC, np.int64) if rank is None else np.asarray(rank, np.int64)
    assert rule in (MAJORITY, PRIORITY) and rank.shape == (NC,) and min_points >= 1
    mask, votes = np.zeros(ncell, np.int64), np.zeros(ncell, np.int32)
    for k in np.flatnonzero(cnt[:, 1:].sum(1) > 0):
        cand = [c for c in range(1, NC) if cnt[k, c] >= min_points]
        if not cand:
            continue
        if rule == MAJORITY:
            keys = sorted((int(cnt[k, c]), int(rank[c]), -c) for c in cand)
        else:
            keys = sorted((int(rank[c]), int(cnt[k, c]), -c) for c in cand)
        win = -keys[-1][2]
        mask[k], votes[k] = win, cnt[k, win]
    return mask, votes


def rasterize_vote(x, y, cls, grid, pc_range, NC, rule, rank=None, min_points=1):
    """one frame -> (mask int64 [H, W], votes int32 [H, W])"""
    mask, votes = resolve(cell_counts(x, y, cls, grid, pc_range, NC), rule, rank, min_points)
    return mask.reshape(grid), votes.reshape(grid)


def rasterize_vote_batch(xs, ys, cs, grid, pc_range, NC, rule, rank=None, min_points=1):
    out = [rasterize_vote(x, y, c, grid, pc_range, NC, rule, rank, min_points) for x, y, c in zip(xs, ys, cs)]
    return np.stack([m for m, _ in out]), np.stack([v for _, v in out])


def label_histogram(mask, NC):
    """int64 [NC + 1]: counts[c] = #{mask == c} for 0 <= c < NC, counts[NC] = every other value"""
    m = np.asarray(mask, np.int64).reshape(-1)
    inside = (m >= 0) & (m < NC)
    return np.bincount(np.where(inside, m, NC), minlength=NC + 1).astype(np.int64)


def median_freq_weights(counts):
    """float64 list: w_c = median{f_k : counts[k] > 0} / f_c, 0 for an absent class"""
    c = np.asarray(counts, np.float64)
    f = c / c.sum()
    med = np.median(f[c > 0])
    return [float(med / v) if v > 0 else 0.0 for v in f]
