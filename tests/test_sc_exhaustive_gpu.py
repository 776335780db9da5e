"""The exhaustive Scan Context calls (include/gorio_sc_pairs.h) on the MI355X: every distance bit for bit what gorio_sc_distance and
the restatement (tests/sc_restatement.py) give, at the extents where the tile kernel's partial tiles begin; best matches, the detect
without the tree, statelessness against a twin handle, and the launch structure through the counters.

Database (29 keyframes of <= 400 points): the 24 of sc_scenes.loop_sequence(n_lap=12, seed=11, n_points=400), an empty scan (24, all-zero
descriptor: 1e7 against everything), a scan confined to 3 sectors (25: most column norms 0 on its side), and keyframes 1, 1 and 14 added
again (26, 27, 28: exact ties)."""
import ctypes as C

import numpy as np
import pytest

import sc_exhaustive_restatement as sx
import sc_restatement as sr
import sc_scenes as ss

pytestmark = pytest.mark.gpu
F = np.float32
EMPTY, NARROW, DUPS = 24, 25, {26: 1, 27: 1, 28: 14}


def _narrow_scan():
    """300 points in sectors 6..8 of 20: azimuth = atan2(x, y) - 90 deg, so x = r cos(az), y = -r sin(az)."""
    rng = np.random.default_rng(5)
    unit = 113.0 / 20.0
    az = np.deg2rad(rng.uniform(-56.5 + 5 * unit + 0.2, -56.5 + 8 * unit - 0.2, 300))
    r = rng.uniform(2.0, 78.0, 300)
    xyz = np.stack([r * np.cos(az), -r * np.sin(az), np.zeros(300)], 1).astype(F)
    return xyz, rng.uniform(1.0, 30.0, 300).astype(F)


@pytest.fixture(scope="module")
def world(gorio, gpu):
    """(scans, info, descs, reference matrix (dist, shift) over the whole database, SCManagerRef).  Computed once, never modified."""
    scans, info = ss.loop_sequence(n_lap=12, seed=11, n_points=400)
    scans = list(scans) + [(np.zeros((0, 3), F), np.zeros(0, F)), _narrow_scan()] + [scans[k] for k in DUPS.values()]
    ref = sr.SCManagerRef()
    for x, i in scans:
        ref.add_scan(x, i)
    assert (ref.descs[EMPTY] == 0).all()
    assert sorted(np.nonzero(sr.col_norms(ref.descs[NARROW]))[0]) == [5, 6, 7]
    dist, shift = sx.distance_matrix(ref.descs)
    dist.setflags(write=False), shift.setflags(write=False)
    return scans, info, ref.descs, dist, shift, ref


@pytest.fixture()
def sc(gorio, world):
    s = gorio.ScanContext()
    assert s.add_scans(world[0]) == 0
    yield s
    s.close()


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def test_tile_shape_is_the_documented_one(gorio):
    S = gorio.scan_context
    txt = open(gorio.INCLUDE_DIR + "/gorio_sc_pairs.h").read()
    for name, v in (("GORIO_SC_TILE_ROWS", S.TILE_ROWS), ("GORIO_SC_TILE_COLS", S.TILE_COLS), ("GORIO_SC_PAIRS_PER_GROUP", S.PAIRS_PER_GROUP)):
        assert f"#define {name} {v}\n" in txt


def test_reference_has_the_cases_it_is_there_for(world):
    _, _, _, dist, shift, _ = world
    assert (dist[EMPTY] == sr.BIG).all() and (dist[:, EMPTY] == sr.BIG).all() and (shift[EMPTY] == 0).all() and (shift[:, EMPTY] == 0).all()
    live = np.delete(np.arange(29), EMPTY)
    assert (dist[NARROW, live] < sr.BIG).sum() > 0 and (dist[np.ix_(live, live)] < sr.BIG).all()
    assert (shift != 0).sum() > 50 and not (dist == dist.T).all()  # shifts occur, and d is not symmetric
    for d, o in DUPS.items():
        assert _same_bits(dist[d], dist[o]) and _same_bits(dist[:, d], dist[:, o])


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 19])
def test_matrix_bits_at_tile_edges(gorio, world, sc, n_rows):
    """Rows and columns of 1, TR - 1, TR, TR + 1 and 2 TR + 3 entries against the restatement, bit for bit, equal on shift."""
    T = gorio.scan_context.TILE_ROWS
    assert (T, gorio.scan_context.TILE_COLS) == (8, 8) and [1, T - 1, T, T + 1, 2 * T + 3] == [1, 7, 8, 9, 19]
    _, _, _, dist, shift, _ = world
    rng = np.random.default_rng(n_rows)
    for n_cols in [1, 7, 8, 9, 19]:
        rows = rng.permutation(29)[:n_rows]
        cols = rng.permutation(29)[:n_cols]
        if n_rows > 8 and n_cols > 8:  # every special scan on both sides at least once
            rows[:3], cols[:3] = [EMPTY, NARROW, 27], [NARROW, EMPTY, 1]
        d, s = sc.distance_matrix(rows, cols)
        assert d.shape == (n_rows, n_cols) and s.dtype == np.int32
        assert _same_bits(d, dist[np.ix_(rows, cols)]), (n_rows, n_cols)
        assert (s == shift[np.ix_(rows, cols)]).all(), (n_rows, n_cols)


def test_matrix_equals_distance_pair_by_pair(sc):
    rows = [EMPTY, NARROW, 0, 13, 27, 5, 22, 9, 16]
    cols = [3, NARROW, 27, EMPTY, 1, 13, 20, 8, 11]
    d, s = sc.distance_matrix(rows, cols)
    for i, r in enumerate(rows):
        for j, c in enumerate(cols):
            wd, ws = sc.distance(r, c)
            assert _same_bits(d[i, j], wd) and s[i, j] == ws, (r, c, d[i, j], wd)


def test_matrix_null_indices_outputs_and_repeats(world, sc):
    _, _, _, dist, shift, _ = world
    d, s = sc.distance_matrix()  # both NULL: the whole database
    assert _same_bits(d, dist) and (s == shift).all()
    d, s = sc.distance_matrix(None, [4, 4, EMPTY, 4])
    assert _same_bits(d, dist[:, [4, 4, EMPTY, 4]]) and (s == shift[:, [4, 4, EMPTY, 4]]).all()
    d, s = sc.distance_matrix([7, 7, 7, 2, 7, 7, 7, 7, 7, 2], None, want_shift=False)  # repeated rows across a tile edge, shift not wanted
    assert s is None and _same_bits(d, dist[[7, 7, 7, 2, 7, 7, 7, 7, 7, 2]])
    d, s = sc.distance_matrix([11, 12], [12, 11, 11], want_dist=False)  # a row equal to a column
    assert d is None and (s == shift[np.ix_([11, 12], [12, 11, 11])]).all()
    d, s = sc.distance_matrix([], [1, 2])  # an empty extent touches nothing
    assert d.shape == (0, 2)


@pytest.mark.parametrize("count", [1, 7, 4, 0])
def test_distance_pairs_equal_the_matrix_entries(gorio, world, sc, count):
    assert 7 % gorio.scan_context.PAIRS_PER_GROUP != 0
    _, _, _, dist, shift, _ = world
    rng = np.random.default_rng(count)
    q, c = rng.integers(0, 29, count), rng.integers(0, 29, count)
    if count == 7:
        q[:3], c[:3] = [EMPTY, 3, NARROW], [3, EMPTY, 27]
    m, ms = sc.distance_matrix(q, c) if count else (np.zeros((0, 0)), np.zeros((0, 0), np.int32))
    d, s = sc.distance_pairs(q, c)
    assert d.shape == (count,) and _same_bits(d, dist[q, c]) and (s == shift[q, c]).all()
    assert _same_bits(d, np.diagonal(m)) and (s == np.diagonal(ms)).all()


def test_best_matches_equal_the_restatement(world, sc):
    _, _, _, dist, shift, _ = world
    every = list(range(29))
    for rows, min_gap in [(None, 1), (None, 10), (None, 28), (None, 29), (None, 1000), ([27, 3, 28, 0, 26, 27, 12, 9, 10, 11, 5], 1), ([28, 2, 26], 2), ([9, 10, 11], 10)]:
        r = every if rows is None else rows
        want = sx.best_matches_from_matrix(dist[r], shift[r], r, min_gap)
        got = sc.best_matches(rows, min_gap)
        assert got[0].tolist() == want[0].tolist(), (rows, min_gap)
        assert _same_bits(got[1], want[1]) and got[2].tolist() == want[2].tolist(), (rows, min_gap)
    idx, best, _ = sc.best_matches(None, 1)
    assert idx[27] == 1 and idx[26] == 1 and idx[28] == 14  # keyframes added twice tie exactly: the lower index wins
    assert _same_bits(best[27], dist[27, 26])               # (26 scores the same as 1 and loses)
    assert idx[0] == -1 and best[0] == sr.BIG                # no candidate
    assert idx[EMPTY] == -1 and best[EMPTY] == sr.BIG        # candidates, none below 1e7
    idx, best, shift_ = sc.best_matches(None, 1000)          # min_gap larger than every row: nothing reaches the device
    assert (idx == -1).all() and (best == sr.BIG).all() and (shift_ == 0).all()


def test_best_matches_over_several_column_tiles_per_workgroup(gorio, world):
    """400 keyframes (the 29 descriptors in rotation): 50 row tiles, so a workgroup walks 2 column tiles per run and 25 runs are folded
    per row.  Every row past 28 has exact ties among the copies of its own descriptor."""
    scans, _, _, dist, shift, _ = world
    n = 400
    sc = gorio.ScanContext()
    sc.add_scans([scans[k % 29] for k in range(n)])
    m = np.arange(n) % 29
    big_d, big_s = dist[np.ix_(m, m)], shift[np.ix_(m, m)]
    for rows, min_gap in [(None, 1), (None, 10), (list(range(399, 0, -7)), 3)]:
        r = list(range(n)) if rows is None else rows
        want = sx.best_matches_from_matrix(big_d[r], big_s[r], r, min_gap)
        got = sc.best_matches(rows, min_gap)
        assert got[0].tolist() == want[0].tolist() and _same_bits(got[1], want[1]) and got[2].tolist() == want[2].tolist(), (rows is None, min_gap)
    sc.close()


def _lists(n):
    """candidate_lists, with the cases the filter is there for: all-recent lists (16, 20) and candidates after the query (15, 21)."""
    cands = [np.asarray(c, np.int32) for c in ss.candidate_lists(n)]
    cands[16] = np.arange(7, 16, dtype=np.int32)                       # all within 10 of query 16: nothing is kept
    cands[20] = np.array([20, 19, 11], np.int32)                       # the query itself and recent ones
    cands[15] = np.array([22, 3, 16, 5, 28, 1], np.int32)              # 22, 16, 28 come after the query and are kept (size_t wrap)
    cands[21] = np.array([23, 27, 26, 1, 12], np.int32)                # after the query, and one recent (12) that is dropped
    cands[13] = np.array([27, 26, 1, 0], np.int32)                     # keyframe 1 and its two copies tie exactly: list order decides
    return cands


def test_detect_exhaustive_equals_the_restatement_in_one_call(world, sc):
    _, _, _, dist, _, ref = world
    cands = _lists(29)
    want = [sx.detect_exhaustive(ref, q, cands[q]) for q in range(29)]
    before = sc.pairs_counters()
    got = sc.detect_exhaustive(list(range(29)), cands)
    after = sc.pairs_counters()
    assert after["calls"] - before["calls"] == 1 and after["synchronisations"] - before["synchronisations"] == 1
    for q in range(29):
        assert got[q][0] == want[q][0] and got[q][1] == want[q][1] and _same_bits(got[q][2], want[q][2]), (q, got[q], want[q])
    assert all(g == (-1, F(0.0), sr.BIG) for g in got[:10])       # the early return
    assert got[16] == (-1, F(0.0), sr.BIG) and got[20] == (-1, F(0.0), sr.BIG)  # all recent: nothing scored, the yaw of shift 0
    assert _same_bits(got[15][2], min(dist[15, c] for c in (22, 3, 16, 5, 28, 1)))
    assert got[13][0] == 27 and got[13][2] < 0.5                   # strict minimum in LIST order: 27 before its equals 26 and 1
    assert sum(g[0] >= 0 for g in got) >= 5 and sum(g[0] < 0 for g in got[10:]) >= 3
    # one query at a time gives the same
    for q in (12, 15, 16, 21, 28):
        assert sc.detect_exhaustive([q], [cands[q]])[0] == got[q]


def _diag_equal(a, b):
    assert a[:3] == b[:3]
    for k in a[3]:
        x, y = np.asarray(a[3][k]), np.asarray(b[3][k])
        assert x.tobytes() == y.tobytes(), k


def test_stateless_beside_detect_batch(gorio, world):
    scans = world[0]
    cands = [np.asarray(c, np.int32) for c in ss.candidate_lists(29)]
    a, b = gorio.ScanContext(), gorio.ScanContext()
    a.add_scans(scans), b.add_scans(scans)
    parts = [list(range(0, 13)), list(range(13, 17)), list(range(17, 29))]
    for part in parts:
        ra = a.detect_batch(part, [cands[q] for q in part])
        a.detect_exhaustive(list(range(29)), _lists(29))
        a.distance_matrix([1, 2, 3], None)
        a.best_matches(None, 3)
        a.distance_pairs([5, 6], [7, 8])
        rb = b.detect_batch(part, [cands[q] for q in part])
        for x, y in zip(ra, rb):
            _diag_equal(x, y)
        sa, sb = a.state(), b.state()
        assert sa["counter"] == sb["counter"] and list(sa["snapshot"]) == list(sb["snapshot"]) and sa["n_scans"] == sb["n_scans"]
    assert a.state()["counter"] > 10  # at least one rebuild happened along the way
    _diag_equal(a.detect(28, cands[20]), b.detect(28, cands[20]))
    assert a.distance(3, 17) == b.distance(3, 17)
    assert b.pairs_counters() == dict(calls=0, pairs=0, launches=0, synchronisations=0)
    a.close(), b.close()


def test_counters_pin_the_launch_structure(sc):
    cands = _lists(29)

    def step(fn):
        c0 = sc.pairs_counters()
        fn()
        c1 = sc.pairs_counters()
        return {k: c1[k] - c0[k] for k in c0}

    assert sc.pairs_counters() == dict(calls=0, pairs=0, launches=0, synchronisations=0)
    assert step(lambda: sc.distance_pairs([1], [2])) == dict(calls=1, pairs=1, launches=1, synchronisations=1)
    assert step(lambda: sc.distance_pairs(list(range(23)), list(range(23)))) == dict(calls=1, pairs=23, launches=1, synchronisations=1)
    assert step(lambda: sc.distance_matrix([1, 2, 3], [4, 5])) == dict(calls=1, pairs=6, launches=1, synchronisations=1)
    assert step(lambda: sc.distance_matrix()) == dict(calls=1, pairs=841, launches=1, synchronisations=1)
    assert step(lambda: sc.best_matches([12], 1)) == dict(calls=1, pairs=12, launches=2, synchronisations=1)
    assert step(lambda: sc.best_matches(None, 1)) == dict(calls=1, pairs=29 * 28 // 2, launches=2, synchronisations=1)
    kept = int((18 - cands[18] >= 10).sum())
    assert kept > 0 and step(lambda: sc.detect_exhaustive([18], [cands[18]])) == dict(calls=1, pairs=kept, launches=2, synchronisations=1)
    d = step(lambda: sc.detect_exhaustive(list(range(29)), cands))
    assert (d["calls"], d["launches"], d["synchronisations"]) == (1, 2, 1) and d["pairs"] > 100
    # nothing to compute: nothing reaches the device
    zero = dict(calls=0, pairs=0, launches=0, synchronisations=0)
    assert step(lambda: sc.distance_pairs([], [])) == zero and step(lambda: sc.distance_matrix([], None)) == zero
    assert step(lambda: sc.best_matches(None, 1000)) == zero and step(lambda: sc.detect_exhaustive([3, 16], [cands[3], cands[16]])) == zero


def test_errors_change_nothing(gorio, sc):
    lib, h = sc.lib, sc.h
    INVALID, UNSUPPORTED = -1, -5
    cands = _lists(29)
    sc.detect_batch(list(range(20)), [cands[q] for q in range(20)])
    before, cbefore = sc.state(), sc.pairs_counters()

    def refused(fn, code, *words):
        with pytest.raises(gorio.GorioError) as e:
            fn()
        assert e.value.code == code, str(e.value)
        for w in words:
            assert w in str(e.value), str(e.value)

    refused(lambda: sc.distance_pairs([1, 29], [2, 3]), INVALID, "pair 1", "29")
    refused(lambda: sc.distance_pairs([1, 2], [2, -1]), INVALID, "pair 1")
    refused(lambda: sc.distance_matrix([1, 2, 40], None), INVALID, "rows[2]", "40")
    refused(lambda: sc.distance_matrix(None, [-3]), INVALID, "cols[0]")
    refused(lambda: sc.distance_matrix([1], [2], want_dist=False, want_shift=False), INVALID, "null")
    refused(lambda: sc.best_matches(None, 0), INVALID, "min_gap")
    refused(lambda: sc.best_matches([3, 99], 1), INVALID, "rows[1]")
    refused(lambda: sc.detect_exhaustive([15, 16], [[1], []]), INVALID, "empty candidate list", "query 1")
    refused(lambda: sc.detect_exhaustive([15, 29], [[1], [2]]), INVALID, "query index 29")
    refused(lambda: sc.detect_exhaustive([15, 16], [[1], [2, 77]]), INVALID, "candidate 1 = 77", "query 1")
    # raw calls: a null extent list needs the whole database, negative counts, and the 2^31 - 1 bound (nothing is allocated or written)
    out = np.full(4, 7.0)
    ptr = C.c_void_p(out.__array_interface__["data"][0])
    assert lib.gorio_sc_distance_matrix(h, None, 5, None, 29, ptr, None) == INVALID and b"rows" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_distance_matrix(h, None, -1, None, 29, ptr, None) == INVALID
    assert lib.gorio_sc_distance_pairs(h, None, None, -1, ptr, None) == INVALID
    assert lib.gorio_sc_best_matches(h, None, 29, 1, None, ptr, None) == INVALID
    assert lib.gorio_sc_detect_exhaustive(h, -1, None, None, None, None, None, None) == INVALID
    rows, cols = np.zeros(65536, np.int32), np.zeros(32768, np.int32)
    pr, pc = C.c_void_p(rows.__array_interface__["data"][0]), C.c_void_p(cols.__array_interface__["data"][0])
    assert lib.gorio_sc_distance_matrix(h, pr, 65536, pc, 32768, ptr, None) == UNSUPPORTED and b"2^31" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_distance_matrix(h, pr, 0, pc, 32768, None, None) == 0 and lib.gorio_sc_distance_pairs(h, None, None, 0, None, None) == 0
    assert lib.gorio_sc_best_matches(h, None, 0, 0, None, None, None) == 0 and lib.gorio_sc_detect_exhaustive(h, 0, None, None, None, None, None, None) == 0
    assert (out == 7.0).all()
    after = sc.state()
    assert after["counter"] == before["counter"] and list(after["snapshot"]) == list(before["snapshot"]) and after["n_scans"] == 29
    assert sc.pairs_counters() == cbefore
