"""The restatement of the cross-database Scan Context calls (tests/sc_cross_restatement.py) on the two databases of
tests/sc_cross_scenes.py, no GPU: the scene has the cases it exists for, and top_from_matrix is gorio_sc_best_matches' reduction when
asked for one match per row of a same-database triangle."""
import numpy as np
import pytest

import sc_cross_restatement as cx
import sc_cross_scenes as cs
import sc_exhaustive_restatement as sx
import sc_restatement as sr


@pytest.fixture(scope="module")
def world():
    return cs.world()


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def test_scene_has_the_cases_it_exists_for(world):
    dist, shift = world["axb"]
    assert dist.shape == (cs.N_A, cs.N_B) == (29, 19)
    assert (world["descs_a"][cs.A_EMPTY] == 0).all() and (world["descs_b"][cs.B_EMPTY] == 0).all()
    assert sorted(np.nonzero(sr.col_norms(world["descs_b"][cs.B_NARROW]))[0]) == [5, 6, 7]
    # B's two copies of A's keyframe 1 tie exactly against every query, at adjacent ranks wherever they make the list
    t0, t1 = cs.B_TIED
    assert _same_bits(dist[:, t0], dist[:, t1]) and (shift[:, t0] == shift[:, t1]).all()
    idx, best, _ = cx.top_from_matrix(dist, shift, None, 3)
    adjacent = 0
    for i in range(cs.N_A):
        row = idx[i].tolist()
        assert (t0 in row) == (t1 in row) or row[2] == t0  # t1 only drops off behind t0
        if t1 in row:
            assert row.index(t1) == row.index(t0) + 1 and best[i, row.index(t0)] == best[i, row.index(t1)]
            adjacent += 1
    assert adjacent >= 3 and idx[1, :2].tolist() == [t0, t1] and idx[26, :2].tolist() == [t0, t1]
    # the empty scans: nothing scores against them on either side; the 3-sector scan scores for several rows
    assert (dist[cs.A_EMPTY] == sr.BIG).all() and (dist[:, cs.B_EMPTY] == sr.BIG).all()
    assert (shift[cs.A_EMPTY] == 0).all() and (shift[:, cs.B_EMPTY] == 0).all()
    assert (dist[:, cs.B_NARROW] < sr.BIG).sum() >= 3
    assert (idx[cs.A_EMPTY] == -1).all() and (best[cs.A_EMPTY] == sr.BIG).all() and not (idx == cs.B_EMPTY).any()
    # shifts occur, and d is not symmetric
    assert (shift != 0).sum() > 30
    da, _ = world["axa"]
    db, _ = world["bxa"]
    assert not (da == da.T).all() and not (dist == db.T).all()


def test_rows_with_fewer_than_k_live_columns(world):
    dist, shift = world["axb"]
    col_end = np.full(cs.N_A, cs.N_B)
    col_end[:3] = [0, 1, 2]
    idx, best, arg = cx.top_from_matrix(dist, shift, col_end, 3)
    assert idx[0].tolist() == [-1, -1, -1] and best[0].tolist() == [sr.BIG] * 3 and arg[0].tolist() == [0, 0, 0]
    assert idx[1].tolist() == [0, -1, -1] and best[1, 0] == dist[1, 0] and arg[1, 0] == shift[1, 0]
    assert sorted(idx[2, :2].tolist()) == [0, 1] and idx[2, 2] == -1 and best[2, 0] <= best[2, 1] < sr.BIG
    assert (idx[cs.A_EMPTY] == -1).all()
    # k = 8 with 3 admissible columns leaves 5 unused slots
    idx, best, _ = cx.top_from_matrix(dist, shift, np.full(cs.N_A, 3), 8)
    assert (idx[0, :3] >= 0).all() and (idx[0, 3:] == -1).all() and (best[0, 3:] == sr.BIG).all()
    # every list ascends in (d, c)
    idx, best, _ = cx.top_from_matrix(dist, shift, None, 8)
    for i in range(cs.N_A):
        keys = [(best[i, j], idx[i, j]) for j in range(8) if idx[i, j] >= 0]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("min_gap", [1, 10, 29])
def test_one_match_over_the_triangle_is_best_matches(world, min_gap):
    dist, shift = world["axa"]
    rows = list(range(cs.N_A))
    col_end = [max(0, r - min_gap + 1) for r in rows]
    want = sx.best_matches_from_matrix(dist, shift, rows, min_gap)
    got = cx.top_from_matrix(dist, shift, col_end, 1)
    assert got[0][:, 0].tolist() == want[0].tolist() and _same_bits(got[1][:, 0], want[1]) and got[2][:, 0].tolist() == want[2].tolist()


def test_cross_matrix_subsets_and_detect(world):
    da, db = world["descs_a"], world["descs_b"]
    dist, shift = world["axb"]
    rows, cols = [cs.A_NARROW, 3, 3, 27], [cs.B_NARROW, 0, 15]
    d, s = cx.cross_matrix(da, db, rows, cols)
    assert _same_bits(d, dist[np.ix_(rows, cols)]) and (s == shift[np.ix_(rows, cols)]).all()
    # list order wins among exact ties; no early return for queries below 10; a list of only the empty scan
    t0, t1 = cs.B_TIED
    assert cx.cross_detect(da, db, 0.5, 56.5, 1, [t1, t0, 3])[0] == t1 and cx.cross_detect(da, db, 0.5, 56.5, 1, [t0, t1, 3])[0] == t0
    assert cx.cross_detect(da, db, 0.5, 56.5, 1, [t1, t0])[2] == dist[1, t0] < 0.5
    assert cx.cross_detect(da, db, 0.5, 56.5, 5, [cs.B_EMPTY]) == (-1, sr.yaw_rad(0, 56.5), sr.BIG)
    lid, yaw, md = cx.cross_detect(da, db, 0.0, 56.5, 1, [t0])
    assert lid == -1 and md == dist[1, t0] and yaw == sr.yaw_rad(shift[1, t0], 56.5)  # the threshold is the query side's
    with pytest.raises(ValueError):
        cx.cross_detect(da, db, 0.5, 56.5, 1, [])
