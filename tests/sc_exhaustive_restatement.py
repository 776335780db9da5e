"""NumPy restatement of the exhaustive Scan Context calls (include/gorio_sc_pairs.h), on top of tests/sc_restatement.py: the same
distance, the same filter, early return, decision rule and yaw as SCManagerRef.detect, with the tree stage (SC:294-338) replaced by
every candidate.  The exhaustive mode is an extension; the Go-RIO sources have no counterpart."""
import numpy as np

from sc_restatement import BIG, EXCLUDE_RECENT, SCManagerRef, distance, yaw_rad

__all__ = ["distance_matrix", "best_matches", "best_matches_from_matrix", "detect_exhaustive", "SCManagerRef"]


def distance_matrix(descs, rows=None, cols=None):
    """(dist [n_rows, n_cols] float64, shift int32) with entry (i, j) = distance(descs[rows[i]], descs[cols[j]]); None = every scan.
    Each distinct pair is computed once."""
    rows = list(range(len(descs))) if rows is None else [int(r) for r in rows]
    cols = list(range(len(descs))) if cols is None else [int(c) for c in cols]
    dist, shift = np.zeros((len(rows), len(cols))), np.zeros((len(rows), len(cols)), np.int32)
    memo = {}
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            if (r, c) not in memo:
                memo[(r, c)] = distance(descs[r], descs[c])
            dist[i, j], shift[i, j] = memo[(r, c)]
    return dist, shift


def best_matches_from_matrix(dist, shift, rows, min_gap):
    """The row-wise reduction of a matrix whose column j is database index j: per row the strict minimum from 1e7 over the columns
    0 .. rows[i] - min_gap in ascending order (so ties go to the lower column); (-1, 1e7, 0) when nothing scores below 1e7."""
    assert min_gap >= 1
    idx, best, arg = np.full(len(rows), -1, np.int32), np.full(len(rows), BIG), np.zeros(len(rows), np.int32)
    for i, r in enumerate(rows):
        for c in range(0, int(r) - min_gap + 1):
            if dist[i, c] < best[i]:
                idx[i], best[i], arg[i] = c, dist[i, c], shift[i, c]
    return idx, best, arg


def best_matches(descs, rows=None, min_gap=EXCLUDE_RECENT):
    rows = list(range(len(descs))) if rows is None else [int(r) for r in rows]
    dist, shift = distance_matrix(descs, rows, None)
    return best_matches_from_matrix(dist, shift, rows, min_gap)


def detect_exhaustive(ref, query, candidates):
    """detectLoopClosureID (SC:272-373) of the SCManagerRef `ref` with every candidate scored -> (loop_id, yaw (float32), min_dist).
    Reads ref.descs, ref.thresh and ref.range only: the counter and the snapshot are neither read nor written."""
    candidates = [int(c) for c in candidates]
    if not candidates:
        raise ValueError("empty candidate list")
    if query < EXCLUDE_RECENT:  # SC:284-288
        return -1, np.float32(0.0), BIG
    kept = [c for c in candidates if (query - c) % (1 << 64) >= EXCLUDE_RECENT]  # SC:300 on the current list, size_t arithmetic
    min_dist, nn_align, nn_idx = BIG, 0, 0
    for c in kept:  # SC:341-348: strict, in list order
        d, s = distance(ref.descs[query], ref.descs[c])
        if d < min_dist:
            min_dist, nn_align, nn_idx = d, s, c
    loop_id = nn_idx if min_dist < ref.thresh else -1  # SC:354-356
    return loop_id, yaw_rad(nn_align, ref.range), min_dist
