"""What the exhaustive Scan Context mode (include/gorio_sc_pairs.h) buys over the tree stage, on the restatements alone (no GPU), and the
rules of best_matches on a hand-made database.  Scene: sc_scenes.loop_sequence(n_lap=12, seed=11, n_points=400) with candidate_lists(24)."""
import numpy as np
import pytest

import sc_exhaustive_restatement as sx
import sc_restatement as sr
import sc_scenes as ss

N_LAP = 12


@pytest.fixture(scope="module")
def scene():
    scans, info = ss.loop_sequence(n_lap=N_LAP, seed=11, n_points=400)
    cands = ss.candidate_lists(len(scans))
    ref = sr.SCManagerRef()
    for x, i in scans:
        ref.add_scan(x, i)
    tree = [ref.detect(q, cands[q]) for q in range(len(scans))]
    state = (ref.counter, list(ref.snapshot))
    full = [sx.detect_exhaustive(ref, q, cands[q]) for q in range(len(scans))]
    assert (ref.counter, list(ref.snapshot)) == state  # stateless
    return info, cands, ref, tree, full


def _place_found(info, q, loop_id):
    """A second-lap keyframe found the place it revisits: a first-lap keyframe within one place of its own, modulo the lap."""
    lap, place, _ = info[q]
    if lap != 1 or loop_id < 0 or info[loop_id][0] != 0:
        return False
    return (info[loop_id][1] - place) % N_LAP in (0, 1, N_LAP - 1)


def test_exhaustive_minimum_never_exceeds_the_trees(scene):
    """For every query: what the tree picks passes through the current candidate list (SC:330-338), and the early returns agree.  (A
    stale snapshot position can name a candidate of the current list that the filter of SC:300 would drop -- query 21 here has such a
    pick; the exhaustive mode does not score those, and none of them is the tree's minimum on this scene.)"""
    _, cands, _, tree, full = scene
    smaller = unfiltered = 0
    for q, (t, f) in enumerate(zip(tree, full)):
        assert f[2] <= t[2], (q, f[2], t[2])
        if t[3]["early_return"]:
            assert f == (-1, np.float32(0.0), sr.BIG)
        smaller += f[2] < t[2]
        unfiltered += any(k >= 0 and (q - int(k)) % (1 << 64) < sr.EXCLUDE_RECENT for k in t[3]["keyframe"])
    print("exhaustive minimum strictly smaller in", smaller, "of", sum(1 for t in tree if not t[3]["early_return"]), "queries;", unfiltered,
          "queries whose tree scored a candidate the filter drops")
    assert smaller > 0


def test_exhaustive_accepts_more_loops_and_finds_more_places(scene):
    """Today's restatement: 9 loops accepted against the tree's 4, and 8 against 2 of the 12 second-lap keyframes matched to the place
    they revisit (+-1, modulo the lap).  The assertion is the strict inequality; the figures are printed."""
    info, _, _, tree, full = scene
    acc_t = sum(1 for t in tree if t[0] >= 0)
    acc_f = sum(1 for f in full if f[0] >= 0)
    hit_t = sum(_place_found(info, q, t[0]) for q, t in enumerate(tree))
    hit_f = sum(_place_found(info, q, f[0]) for q, f in enumerate(full))
    print("loops accepted: exhaustive", acc_f, "tree", acc_t, "; revisited places found: exhaustive", hit_f, "tree", hit_t)
    assert acc_f > acc_t
    assert hit_f > hit_t
    # an accepted loop carries the minimum's own candidate and a distance below the threshold
    for f in full:
        assert (f[0] >= 0) == (f[2] < 0.5)


def _numpy_rowmin(dist, shift, rows, min_gap):
    """Independent of the restatement's loop: a masked argmin (numpy returns the first of equal minima)."""
    idx, best, arg = [], [], []
    for i, r in enumerate(rows):
        n = r - min_gap + 1
        ok = n > 0 and dist[i, :n].min() < sr.BIG
        c = int(np.argmin(dist[i, :n])) if ok else -1
        idx.append(c)
        best.append(dist[i, c] if ok else sr.BIG)
        arg.append(shift[i, c] if ok else 0)
    return np.array(idx), np.array(best), np.array(arg)


def test_best_matches_is_the_row_reduction_of_the_matrix(scene):
    _, _, ref, _, _ = scene
    rows = list(range(len(ref.descs)))
    dist, shift = sx.distance_matrix(ref.descs)
    for min_gap in (1, sr.EXCLUDE_RECENT, len(rows) - 1, len(rows) + 3):
        got = sx.best_matches(ref.descs, None, min_gap)
        want = _numpy_rowmin(dist, shift, rows, min_gap)
        for g, w in zip(got, want):
            assert g.tolist() == w.tolist(), min_gap
    got = sx.best_matches(ref.descs, [20, 3, 20, 11], 2)  # rows out of order and repeated
    want = _numpy_rowmin(dist[[20, 3, 20, 11]], shift[[20, 3, 20, 11]], [20, 3, 20, 11], 2)
    for g, w in zip(got, want):
        assert g.tolist() == w.tolist()


def test_tie_rule_and_min_gap_edges_on_duplicated_descriptors():
    """Database A B A B Z A: duplicates tie exactly, Z is all zero (1e7 against everything)."""
    rng = np.random.default_rng(3)
    A, B = rng.uniform(0.1, 9.0, (2, sr.RINGS, sr.SECTORS))
    Z = np.zeros((sr.RINGS, sr.SECTORS))
    descs = [A, B, A, B, Z, A]
    d_aa, d_ab = sr.distance(A, A)[0], sr.distance(A, B)[0]
    assert d_aa < d_ab < 1.0 and sr.distance(A, Z) == (sr.BIG, 0) and sr.distance(Z, Z) == (sr.BIG, 0)
    idx, best, arg = sx.best_matches(descs, None, 1)
    assert idx.tolist() == [-1, 0, 0, 1, -1, 0]  # row 5 (A) ties with columns 0 and 2: the lower wins; row 4 (Z) finds nothing
    assert best.tolist() == [sr.BIG, sr.distance(B, A)[0], d_aa, sr.distance(B, B)[0], sr.BIG, d_aa]
    assert arg[0] == 0 and arg[4] == 0
    idx, best, _ = sx.best_matches(descs, None, 3)  # r - min_gap < 0 for rows 0..2, == 0 for row 3
    assert idx.tolist() == [-1, -1, -1, 0, -1, 0]
    assert best[3] == sr.distance(B, A)[0] and best[5] == d_aa  # row 5: columns 0..2, A at 0 and 2
    idx, _, _ = sx.best_matches(descs, [5, 2, 5], 5)  # row 5: r - min_gap == 0; row 2: < 0
    assert idx.tolist() == [0, -1, 0]
    idx, best, arg = sx.best_matches(descs, None, 6)  # larger than every row
    assert idx.tolist() == [-1] * 6 and best.tolist() == [sr.BIG] * 6 and arg.tolist() == [0] * 6
    with pytest.raises(AssertionError):
        sx.best_matches(descs, None, 0)
