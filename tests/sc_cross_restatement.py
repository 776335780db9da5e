"""NumPy restatement of the cross-database Scan Context calls (include/gorio_sc_cross.h), on top of tests/sc_restatement.py: the same
distance, with the query descriptor from one database and the candidate descriptor from another; the K best per row as a plain sort;
the detect over lists with neither the early return nor the recent-keyframe filter.  An extension; the Go-RIO sources have no
counterpart."""
import numpy as np

from sc_restatement import BIG, distance, yaw_rad

__all__ = ["cross_matrix", "top_from_matrix", "cross_detect"]


def cross_matrix(descs_q, descs_d, rows=None, cols=None):
    """(dist [n_rows, n_cols] float64, shift int32) with entry (i, j) = distance(descs_q[rows[i]], descs_d[cols[j]]), the query side
    unshifted; None = every scan of that side.  Each distinct pair is computed once."""
    rows = list(range(len(descs_q))) if rows is None else [int(r) for r in rows]
    cols = list(range(len(descs_d))) if cols is None else [int(c) for c in cols]
    dist, shift = np.zeros((len(rows), len(cols))), np.zeros((len(rows), len(cols)), np.int32)
    memo = {}
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if (r, c) not in memo:
                memo[(r, c)] = distance(descs_q[r], descs_d[c])
            dist[i, j], shift[i, j] = memo[(r, c)]
    return dist, shift


def top_from_matrix(dist, shift, col_end, k):
    """The row-wise selection from a matrix whose column j is database index j: per row i the columns 0 .. col_end[i] - 1 (None: all)
    that score below 1e7, in a stable sort by distance (so ties keep the lower column first), cut to k -> (index [n, k] int32,
    dist [n, k] float64, shift [n, k] int32) with unused slots (-1, 1e7, 0)."""
    assert k >= 1
    n = dist.shape[0]
    idx, best, arg = np.full((n, k), -1, np.int32), np.full((n, k), BIG), np.zeros((n, k), np.int32)
    for i in range(n):
        e = dist.shape[1] if col_end is None else int(col_end[i])
        assert 0 <= e <= dist.shape[1]
        live = [c for c in range(e) if dist[i, c] < BIG]
        live.sort(key=lambda c: dist[i, c])  # list.sort is stable: equal distances stay in column order
        for j, c in enumerate(live[:k]):
            idx[i, j], best[i, j], arg[i, j] = c, dist[i, c], shift[i, c]
    return idx, best, arg


def cross_detect(descs_q, descs_d, thresh, azimuth_range, query, candidates):
    """SC:341-371 over the whole list: the strict minimum from 1e7 in list order, the threshold, the yaw -> (loop_id, yaw (float32),
    min_dist).  No early return (SC:284-288) and no filter (SC:294-306)."""
    candidates = [int(c) for c in candidates]
    if not candidates:
        raise ValueError("empty candidate list")
    min_dist, nn_align, nn_idx = BIG, 0, 0
    for c in candidates:
        d, s = distance(descs_q[query], descs_d[c])
        if d < min_dist:
            min_dist, nn_align, nn_idx = d, s, c
    loop_id = nn_idx if min_dist < thresh else -1
    return loop_id, yaw_rad(nn_align, azimuth_range), min_dist
