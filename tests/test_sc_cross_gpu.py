"""The cross-database Scan Context calls (include/gorio_sc_cross.h) on the MI355X, over the two databases of tests/sc_cross_scenes.py
(A: 29 keyframes, the query side unless said otherwise; B: 19 keyframes): every distance bit for bit what the restatement
(tests/sc_cross_restatement.py) and a merged handle give, the K best per row against a plain stable sort of the matrix, the detect over
lists, statelessness of both handles against twins, a database that grows between calls, the launch structure through the counters,
the calls of both headers in two orders on one pair of handles, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import sc_cross_restatement as cx
import sc_cross_scenes as cs
import sc_restatement as sr
import sc_scenes as ss

pytestmark = pytest.mark.gpu
F = np.float32
INVALID, UNSUPPORTED = -1, -5
ZERO = dict(calls=0, pairs=0, launches=0, synchronisations=0)


@pytest.fixture(scope="module")
def world(gorio, gpu):
    return cs.world()


@pytest.fixture(scope="module")
def handles(gorio, world):
    """(A, B): read-only for the tests that take them (their cross counters move; tests that pin counters take differences)."""
    a, b = gorio.ScanContext(), gorio.ScanContext()
    assert a.add_scans(world["scans_a"]) == 0 and b.add_scans(world["scans_b"]) == 0
    yield a, b
    a.close(), b.close()


@pytest.fixture()
def fresh(gorio, world):
    a, b = gorio.ScanContext(), gorio.ScanContext()
    a.add_scans(world["scans_a"]), b.add_scans(world["scans_b"])
    yield a, b
    a.close(), b.close()


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def _top_equal(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32
    assert got[0].tolist() == want[0].tolist(), what
    assert _same_bits(got[1], want[1]), what
    assert got[2].tolist() == want[2].tolist(), what


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 19])
def test_matrix_bits_at_tile_edges(gorio, world, handles, n_rows):
    """Rows of A and columns of B of 1, T - 1, T, T + 1 and 2 T + 3 entries against the restatement, bit for bit, equal on shift."""
    T = gorio.scan_context.TILE_ROWS
    assert (T, gorio.scan_context.TILE_COLS) == (8, 8) and [1, T - 1, T, T + 1, 2 * T + 3] == [1, 7, 8, 9, 19]
    a, b = handles
    dist, shift = world["axb"]
    rng = np.random.default_rng(100 + n_rows)
    for n_cols in [1, 7, 8, 9, 19]:
        rows = rng.permutation(cs.N_A)[:n_rows]
        cols = rng.permutation(cs.N_B)[:n_cols]
        if n_rows > 8 and n_cols > 8:  # every special scan on both sides at least once
            rows[:3], cols[:3] = [cs.A_EMPTY, cs.A_NARROW, 27], [cs.B_NARROW, cs.B_EMPTY, cs.B_TIED[0]]
        d, s = a.cross_distance_matrix(b, rows, cols)
        assert d.shape == (n_rows, n_cols) and s.dtype == np.int32
        assert _same_bits(d, dist[np.ix_(rows, cols)]), (n_rows, n_cols)
        assert (s == shift[np.ix_(rows, cols)]).all(), (n_rows, n_cols)


def test_matrix_null_indices_outputs_repeats_and_the_other_direction(world, handles):
    a, b = handles
    dist, shift = world["axb"]
    d, s = a.cross_distance_matrix(b)  # both NULL: all of A against all of B
    assert d.shape == (29, 19) and _same_bits(d, dist) and (s == shift).all()
    d, s = a.cross_distance_matrix(b, None, [4, 4, cs.B_EMPTY, 4])
    assert _same_bits(d, dist[:, [4, 4, cs.B_EMPTY, 4]]) and (s == shift[:, [4, 4, cs.B_EMPTY, 4]]).all()
    rep = [7, 7, 7, 2, 7, 7, 7, 7, 7, 2]
    d, s = a.cross_distance_matrix(b, rep, None, want_shift=False)  # repeated rows across a tile edge, shift not wanted
    assert s is None and _same_bits(d, dist[rep])
    d, s = a.cross_distance_matrix(b, [11, 12], rep, want_dist=False)  # repeated columns across a tile edge, dist not wanted
    assert d is None and (s == shift[np.ix_([11, 12], rep)]).all()
    assert a.cross_distance_matrix(b, [], [1, 2])[0].shape == (0, 2)  # an empty extent touches nothing
    d, s = b.cross_distance_matrix(a)  # B as the query side: the transpose's own values, d is not symmetric
    assert d.shape == (19, 29) and _same_bits(d, world["bxa"][0]) and (s == world["bxa"][1]).all()


def test_cross_equals_a_merged_handle(gorio, world, handles):
    a, b = handles
    m = gorio.ScanContext()
    m.add_scans(world["scans_a"]), m.add_scans(world["scans_b"])
    rng = np.random.default_rng(9)
    for rows, cols in [(None, None), (rng.permutation(29)[:9], rng.permutation(19)[:17])]:
        r = np.arange(29) if rows is None else rows
        c = np.arange(19) if cols is None else cols
        d, s = a.cross_distance_matrix(b, rows, cols)
        md, ms = m.distance_matrix(r, 29 + c)
        assert _same_bits(d, md) and (s == ms).all()
    for count in (0, 1, 4, 7):
        q, c = rng.integers(0, 29, count), rng.integers(0, 19, count)
        if count == 7:
            q[:3], c[:3] = [cs.A_EMPTY, 3, cs.A_NARROW], [3, cs.B_EMPTY, cs.B_TIED[1]]
        d, s = a.cross_distance_pairs(b, q, c)
        md, ms = m.distance_pairs(q, 29 + c)
        assert d.shape == (count,) and _same_bits(d, md) and (s == ms).all()
        assert _same_bits(d, world["axb"][0][q, c]) and (s == world["axb"][1][q, c]).all()
    for q, c in [(3, 5), (cs.A_EMPTY, 2), (27, cs.B_TIED[0])]:  # and each is gorio_sc_distance on the merged handle
        d, s = a.cross_distance_pairs(b, [q], [c])
        assert (d[0], s[0]) == m.distance(q, 29 + c)
    m.close()


def test_same_handle_on_both_sides(world, handles):
    a, _ = handles
    rows, cols = [cs.A_EMPTY, cs.A_NARROW, 0, 13, 27, 5, 22, 9, 16], [3, cs.A_NARROW, 27, cs.A_EMPTY, 1, 13, 20, 8, 11, 4]
    d, s = a.cross_distance_matrix(a, rows, cols)
    wd, ws = a.distance_matrix(rows, cols)
    assert _same_bits(d, wd) and (s == ws).all() and _same_bits(d, world["axa"][0][np.ix_(rows, cols)])
    d, s = a.cross_distance_pairs(a, rows, cols[:9])
    wd, ws = a.distance_pairs(rows, cols[:9])
    assert _same_bits(d, wd) and (s == ws).all()
    assert (d[2], s[2]) == a.distance(rows[2], cols[2])
    for rows, g in [(None, 1), (None, 10), (None, 1000), ([27, 3, 28, 0, 26, 27, 12, 9, 10, 11, 5], 1)]:
        r = np.arange(29) if rows is None else np.asarray(rows)
        want = a.best_matches(rows, g)
        for other in (None, a):
            got = a.top_matches(other, rows, np.maximum(0, r - g + 1), k=1)
            assert got[0].shape == (len(r), 1)
            _top_equal([x[:, 0] for x in got], want, (rows, g))


MIXED = np.array([0, 1, 2, 8, 9, 19, 3, 19, 7, 16, 0, 17, 18, 15, 14, 1, 19, 8, 9, 2, 10, 11, 12, 13, 19, 19, 5, 6, 19], np.int32)


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_top_matches_of_a_in_b(world, handles, k):
    a, b = handles
    dist, shift = world["axb"]
    assert len(MIXED) == 29 and {0, 1, 2, 8, 9, 19} <= set(MIXED.tolist())
    for col_end in (None, np.zeros(29, np.int32), MIXED, np.full(29, 3, np.int32)):
        _top_equal(a.top_matches(b, None, col_end, k), cx.top_from_matrix(dist, shift, col_end, k), (k, col_end))
    rows = [27, cs.A_EMPTY, 3, 1, 1, cs.A_NARROW, 28, 0, 14, 20, 9]  # listed rows, repeated, across a tile edge
    ends = MIXED[:11][::-1].copy()
    _top_equal(a.top_matches(b, rows, ends, k), cx.top_from_matrix(dist[rows], shift[rows], ends, k), (k, "listed"))
    idx, best, arg = a.top_matches(b, None, None, k)
    t0, t1 = cs.B_TIED
    if k >= 2:  # the two tied copies in index order at adjacent ranks: A's keyframe 1 and its copies score their self-distance
        for r in (1, 26, 27):
            assert idx[r, :2].tolist() == [t0, t1] and best[r, 0] == best[r, 1] and arg[r, 0] == arg[r, 1]
    else:
        assert idx[1, 0] == t0 and idx[26, 0] == t0
    assert (idx[cs.A_EMPTY] == -1).all() and (best[cs.A_EMPTY] == sr.BIG).all() and (arg[cs.A_EMPTY] == 0).all()
    assert not (idx == cs.B_EMPTY).any()
    if k == 8:  # 3 admissible columns leave 5 unused slots
        idx, best, arg = a.top_matches(b, None, np.full(29, 3, np.int32), 8)
        live = np.delete(np.arange(29), cs.A_EMPTY)
        assert (idx[live, :3] >= 0).all() and (idx[:, 3:] == -1).all() and (best[:, 3:] == sr.BIG).all() and (arg[:, 3:] == 0).all()


def test_top_matches_over_several_column_tiles_and_runs(gorio, world):
    """400 rows (A's descriptors in rotation) against a 400-entry database (B's in rotation): 50 row tiles, so a workgroup walks 2
    column tiles per run and 25 runs are merged per row.  Nearly every rank is an exact tie among the copies of one descriptor, so only
    the (d, c) rule gives the expected order."""
    n = 400
    qa, qb = np.arange(n) % cs.N_A, np.arange(n) % cs.N_B
    a, b = gorio.ScanContext(), gorio.ScanContext()
    a.add_scans([world["scans_a"][i] for i in qa]), b.add_scans([world["scans_b"][i] for i in qb])
    big_d, big_s = world["axb"][0][np.ix_(qa, qb)], world["axb"][1][np.ix_(qa, qb)]
    descending = (n - np.arange(n)).astype(np.int32)
    for k in (3, 8):
        for col_end in (None, descending):
            want = cx.top_from_matrix(big_d, big_s, col_end, k)
            _top_equal(a.top_matches(b, None, col_end, k), want, (k, col_end is None))
            assert (want[1][0, 1:] == want[1][0, :-1]).any()  # exact ties at adjacent ranks
    rows = np.arange(399, 0, -7)
    _top_equal(a.top_matches(b, rows, descending[: len(rows)], 3), cx.top_from_matrix(big_d[rows], big_s[rows], descending[: len(rows)], 3), "listed")
    a.close(), b.close()


def _lists():
    """One list of B indices per keyframe of A, with the cases the call is there for."""
    rng = np.random.default_rng(17)
    lists = [rng.permutation(cs.N_B)[: int(rng.integers(1, cs.N_B + 1))].astype(np.int32) for _ in range(cs.N_A)]
    lists[1] = np.array([3, cs.B_TIED[1], cs.B_TIED[0], 0], np.int32)   # the two tied copies in reverse index order: list order wins
    lists[5] = np.array([cs.B_EMPTY], np.int32)                           # only the empty scan
    lists[7] = np.array([cs.B_EMPTY, cs.B_NARROW, cs.B_EMPTY], np.int32)
    lists[28] = np.arange(cs.N_B - 1, -1, -1, dtype=np.int32)            # all of B, backwards
    return lists


def test_cross_detect_equals_the_restatement(world, handles):
    a, b = handles
    lists = _lists()
    da, db = world["descs_a"], world["descs_b"]
    want = [cx.cross_detect(da, db, 0.5, 56.5, q, lists[q]) for q in range(cs.N_A)]
    before = a.cross_counters()
    got = a.cross_detect(b, list(range(cs.N_A)), lists)
    after = a.cross_counters()
    assert after["calls"] - before["calls"] == 1 and after["synchronisations"] - before["synchronisations"] == 1
    for q in range(cs.N_A):
        assert got[q][0] == want[q][0] and got[q][1] == want[q][1] and _same_bits(got[q][2], want[q][2]), (q, got[q], want[q])
    assert got[1][0] == cs.B_TIED[1] and got[1][2] < 0.5                      # strict minimum in LIST order
    assert got[5] == (-1, sr.yaw_rad(0, 56.5), sr.BIG) and got[5][1] == F(0.0)   # nothing scored below 1e7: the yaw of shift 0
    assert got[28][0] == cs.B_A14 and any(g[0] >= 0 for g in got[:10])          # queries below 10 are scored like any other
    assert sum(g[0] >= 0 for g in got) >= 3 and sum(g[0] < 0 for g in got) >= 3
    for q in (0, 1, 5, 7, 28):  # one query at a time gives the same
        assert a.cross_detect(b, [q], [lists[q]])[0] == got[q]
    # the threshold is the query handle's
    assert all(g[0] == -1 for g in _with_thresh(world, b, 0.0, lists)) and all(g[0] >= 0 or g[2] == sr.BIG for g in _with_thresh(world, b, 2.0, lists))


def _with_thresh(world, b, thresh, lists):
    import importlib

    q = importlib.import_module("go-rio_amd").ScanContext(sc_dist_thresh=thresh)
    q.add_scans(world["scans_a"])
    out = q.cross_detect(b, list(range(cs.N_A)), lists)
    q.close()
    return out


def _diag_equal(a, b):
    assert a[:3] == b[:3]
    for k in a[3]:
        assert np.asarray(a[3][k]).tobytes() == np.asarray(b[3][k]).tobytes(), k


def test_both_handles_stay_stateless(gorio, world):
    """Q and D beside twins that make no cross call: the same detect_batch sequence gives the same diagnostics, state and counters."""
    q, q2, d, d2 = (gorio.ScanContext() for _ in range(4))
    for h in (q, q2):
        h.add_scans(world["scans_a"])
    for h in (d, d2):
        h.add_scans(world["scans_b"])
    ca = [np.asarray(c, np.int32) for c in ss.candidate_lists(cs.N_A)]
    cb = [np.asarray(c, np.int32) for c in ss.candidate_lists(cs.N_B)]
    lists = _lists()
    for lo, hi in [(0, 13), (13, 17), (17, 29)]:
        part_a, part_b = list(range(lo, hi)), list(range(min(lo, 19), min(hi, 19)))
        ra = q.detect_batch(part_a, [ca[i] for i in part_a])
        rd = d.detect_batch(part_b, [cb[i] for i in part_b]) if part_b else []
        q.cross_distance_matrix(d, [1, 2, 3], None)
        q.top_matches(d, None, None, 3)
        q.cross_distance_pairs(d, [5, 6], [7, 8])
        q.cross_detect(d, list(range(cs.N_A)), lists)
        q.top_matches(None, None, None, 2)
        ra2 = q2.detect_batch(part_a, [ca[i] for i in part_a])
        rd2 = d2.detect_batch(part_b, [cb[i] for i in part_b]) if part_b else []
        for x, y in list(zip(ra, ra2)) + list(zip(rd, rd2)):
            _diag_equal(x, y)
        for x, y in ((q, q2), (d, d2)):
            sx_, sy = x.state(), y.state()
            assert sx_["counter"] == sy["counter"] and list(sx_["snapshot"]) == list(sy["snapshot"]) and sx_["n_scans"] == sy["n_scans"]
    assert q.state()["counter"] > 10 and d.state()["counter"] > 5
    assert q.pairs_counters() == q2.pairs_counters() == ZERO and d.pairs_counters() == d2.pairs_counters() == ZERO
    assert d.cross_counters() == d2.cross_counters() == ZERO and q2.cross_counters() == ZERO and q.cross_counters()["calls"] == 15
    assert q.distance(3, 17) == q2.distance(3, 17) and d.distance(3, 17) == d2.distance(3, 17)
    for h in (q, q2, d, d2):
        h.close()


def test_database_grows_between_calls(world, fresh):
    """19 + 60 scans pass the database's first capacity of 64, so its buffers move: the next call reads the new ones."""
    a, b = fresh
    dist, shift = world["axb"]
    _top_equal(a.top_matches(b, None, None, 3), cx.top_from_matrix(dist, shift, None, 3), "before")
    more = np.arange(60) % cs.N_A
    assert b.add_scans([world["scans_a"][i] for i in more]) == 19 and b.state()["n_scans"] == 79
    big_d = np.concatenate([dist, world["axa"][0][:, more]], axis=1)
    big_s = np.concatenate([shift, world["axa"][1][:, more]], axis=1)
    d, s = a.cross_distance_matrix(b)
    assert d.shape == (29, 79) and _same_bits(d, big_d) and (s == big_s).all()
    _top_equal(a.top_matches(b, None, None, 3), cx.top_from_matrix(big_d, big_s, None, 3), "after")
    _top_equal(a.top_matches(b, None, np.full(29, 19, np.int32), 3), cx.top_from_matrix(dist, shift, None, 3), "old columns")
    got = a.cross_detect(b, [2], [[78, 20, 3]])[0]
    assert got == cx.cross_detect(world["descs_a"], world["descs_b"] + [world["descs_a"][i] for i in more], 0.5, 56.5, 2, [78, 20, 3])


def test_counters_pin_the_launch_structure(fresh):
    a, b = fresh
    lists = _lists()

    def step(fn):
        c0 = a.cross_counters()
        fn()
        c1 = a.cross_counters()
        return {k: c1[k] - c0[k] for k in c0}

    assert a.cross_counters() == ZERO
    assert step(lambda: a.cross_distance_pairs(b, [1], [2])) == dict(calls=1, pairs=1, launches=1, synchronisations=1)
    assert step(lambda: a.cross_distance_pairs(b, list(range(19)), list(range(19)))) == dict(calls=1, pairs=19, launches=1, synchronisations=1)
    assert step(lambda: a.cross_distance_matrix(b, [1, 2, 3], [4, 5])) == dict(calls=1, pairs=6, launches=1, synchronisations=1)
    assert step(lambda: a.cross_distance_matrix(b)) == dict(calls=1, pairs=29 * 19, launches=1, synchronisations=1)
    assert step(lambda: a.top_matches(b, [12], None, 1)) == dict(calls=1, pairs=19, launches=2, synchronisations=1)
    assert step(lambda: a.top_matches(b, None, None, 8)) == dict(calls=1, pairs=29 * 19, launches=2, synchronisations=1)
    assert step(lambda: a.top_matches(b, None, MIXED, 3)) == dict(calls=1, pairs=int(MIXED.sum()), launches=2, synchronisations=1)
    assert step(lambda: a.top_matches(None, None, np.arange(29), 3)) == dict(calls=1, pairs=29 * 28 // 2, launches=2, synchronisations=1)
    assert step(lambda: a.cross_detect(b, [18], [lists[18]])) == dict(calls=1, pairs=len(lists[18]), launches=2, synchronisations=1)
    assert step(lambda: a.cross_detect(b, list(range(29)), lists)) == dict(calls=1, pairs=sum(len(x) for x in lists), launches=2, synchronisations=1)
    # nothing to compute: nothing reaches the device
    assert step(lambda: a.cross_distance_pairs(b, [], [])) == ZERO and step(lambda: a.cross_distance_matrix(b, [], None)) == ZERO
    assert step(lambda: a.cross_distance_matrix(b, None, [])) == ZERO and step(lambda: a.top_matches(b, [], [], 3)) == ZERO
    idx, best, arg = None, None, None

    def all_zero():
        nonlocal idx, best, arg
        idx, best, arg = a.top_matches(b, None, np.zeros(29, np.int32), 3)

    assert step(all_zero) == ZERO and (idx == -1).all() and (best == sr.BIG).all() and (arg == 0).all()
    assert step(lambda: a.cross_detect(b, [], [])) == ZERO
    assert a.pairs_counters() == ZERO and b.pairs_counters() == ZERO and b.cross_counters() == ZERO


def _int_columns(result):
    """A call's result as integer arrays: a detect's list of (loop_id, yaw_rad, min_dist) by column, float64 viewed as int64 and float32
    as int32."""
    if isinstance(result, list):
        result = (np.array([r[0] for r in result]), np.array([r[1] for r in result], F), np.array([r[2] for r in result], np.float64))
    return [a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == F else a for a in map(np.asarray, result)]


def test_call_order_does_not_matter(gorio, world):
    """The eight calls of the two headers share two runners and one pair of scratch buffers on the query handle.  Each call's result on
    a fresh pair of handles is the reference; all eight then run on one pair of handles in two interleavings, one ending each family with
    its largest request (the whole matrix) and one with its smallest (a few listed pairs), top_matches before a matrix and a detect after
    best_matches, so partial tables and segment offsets lie in the buffers the next call uses.  Every result has the reference's bits,
    and each counter group advances by its own family's four calls."""
    lists = _lists()
    cq = [1, 5, 7, 28, 14]
    eq = [28, 3, 20, 12]  # 3 returns early; 25 lies after its query 20 and is kept (SC:300); 3 is too recent for 12
    el = [np.arange(28), [0, 1], [5, 15, 25, 10], [0, 1, 2, 3]]
    kept = sum(1 for q, cand in zip(eq, el) if q >= 10 for c in cand if c > q or q - c >= 10)
    assert kept == 19 + 3 + 3
    calls = {  # name: (family, pairs, launches, the call)
        "distance_pairs": ("pairs", 5, 1, lambda a, b: a.distance_pairs([3, cs.A_EMPTY, 27, 0, 13], [27, 4, cs.A_NARROW, 0, 2])),
        "distance_matrix": ("pairs", 29 * 29, 1, lambda a, b: a.distance_matrix()),
        "best_matches": ("pairs", 29 * 28 // 2, 2, lambda a, b: a.best_matches(None, 1)),
        "detect_exhaustive": ("pairs", kept, 2, lambda a, b: a.detect_exhaustive(eq, el)),
        "cross_distance_pairs": ("cross", 7, 1, lambda a, b: a.cross_distance_pairs(b, [cs.A_EMPTY, 3, cs.A_NARROW, 28, 0, 9, 9], [3, cs.B_EMPTY, cs.B_TIED[1], 18, 0, 7, 7])),
        "cross_distance_matrix": ("cross", 29 * 19, 1, lambda a, b: a.cross_distance_matrix(b)),
        "top_matches": ("cross", int(MIXED.sum()), 2, lambda a, b: a.top_matches(b, None, MIXED, 3)),
        "cross_detect": ("cross", sum(len(lists[q]) for q in cq), 2, lambda a, b: a.cross_detect(b, cq, [lists[q] for q in cq])),
    }

    def pair_of_handles():
        a, b = gorio.ScanContext(), gorio.ScanContext()
        a.add_scans(world["scans_a"]), b.add_scans(world["scans_b"])
        return a, b

    want = {}
    for name, (_, _, _, fn) in calls.items():
        a, b = pair_of_handles()
        want[name] = _int_columns(fn(a, b))
        a.close(), b.close()
    assert (want["detect_exhaustive"][0] >= 0).any() and (want["cross_detect"][0] >= 0).any() and (want["best_matches"][0] >= 0).any()
    largest_last = ["cross_distance_pairs", "top_matches", "distance_pairs", "best_matches", "cross_detect", "detect_exhaustive", "cross_distance_matrix", "distance_matrix"]
    smallest_last = ["top_matches", "cross_distance_matrix", "best_matches", "detect_exhaustive", "distance_matrix", "cross_detect", "distance_pairs", "cross_distance_pairs"]
    for order in (largest_last, smallest_last):
        assert sorted(order) == sorted(calls)
        a, b = pair_of_handles()
        for name in order:
            got = _int_columns(calls[name][3](a, b))
            assert len(got) == len(want[name]) and all(np.array_equal(g, w) for g, w in zip(got, want[name])), (order[-1], name)
        for family, counters in (("pairs", a.pairs_counters()), ("cross", a.cross_counters())):
            mine = [c for c in calls.values() if c[0] == family]
            assert counters == dict(calls=4, pairs=sum(c[1] for c in mine), launches=sum(c[2] for c in mine), synchronisations=4), family
        assert b.pairs_counters() == ZERO and b.cross_counters() == ZERO
        a.close(), b.close()


def test_errors_change_nothing(gorio, world, fresh):
    a, b = fresh
    lib = a.lib
    lists = _lists()
    other = gorio.ScanContext(azimuth_range=50.0)
    other.add_scans(world["scans_b"][:3])
    a.detect_batch(list(range(20)), [np.asarray(c, np.int32) for c in ss.candidate_lists(20)])
    a.top_matches(b, None, None, 3)
    before = (a.state(), b.state(), a.cross_counters(), b.cross_counters(), a.pairs_counters(), b.pairs_counters())
    out_d, out_i, out_j = np.full(1024, 7.0), np.full(1024, 7, np.int32), np.full(1024, 7, np.int32)
    yaw = np.full(64, 7.0, F)

    def p(x):
        return None if x is None else C.c_void_p(np.ascontiguousarray(x).__array_interface__["data"][0])

    def ints(x):
        return np.ascontiguousarray(x, np.int32)

    def refused(rc, code, *words):
        text = lib.gorio_sc_last_error().decode()
        assert rc == code, (rc, text)
        for w in words:
            assert w in text, text
        assert (out_d == 7.0).all() and (out_i == 7).all() and (out_j == 7).all() and (yaw == 7.0).all()

    def matrix(Q, D, rows, cols, d=out_d, s=out_i):
        r, c = (None if rows is None else ints(rows)), (None if cols is None else ints(cols))
        return lib.gorio_sc_cross_distance_matrix(Q.h, p(r), 29 if r is None else len(r), D.h, p(c), D.state()["n_scans"] if c is None else len(c), p(d), p(s))

    def top(Q, D, rows, col_end, k):
        r, e = (None if rows is None else ints(rows)), (None if col_end is None else ints(col_end))
        return lib.gorio_sc_cross_top_matches(Q.h, p(r), 29 if r is None else len(r), D.h, p(e), k, p(out_i), p(out_d), p(out_j))

    def pairs(Q, D, q, c):
        q, c = ints(q), ints(c)
        return lib.gorio_sc_cross_distance_pairs(Q.h, D.h, p(q), p(c), len(q), p(out_d), p(out_i))

    def detect(Q, D, queries, cand):
        k = len(queries)
        arrs = [ints(c) for c in cand]
        P = (C.c_void_p * k)(*[x.__array_interface__["data"][0] if x.size else None for x in arrs])
        qs, ns = ints(queries), ints([x.size for x in arrs])  # named, so they outlive the call
        return lib.gorio_sc_cross_detect(Q.h, D.h, k, p(qs), P, p(ns), p(out_i), p(yaw), p(out_d))

    # descriptors of different azimuth ranges are not comparable: every call refuses, naming both values
    for rc in (matrix(a, other, [1], [1]), top(a, other, [1], None, 3), pairs(a, other, [1], [1]), detect(a, other, [1], [[1]]), matrix(other, a, [1], [1])):
        refused(rc, INVALID, "azimuth_range", "56.5", "50.0")
    # index 25 is valid in A (29 scans) but not in B (19): the text names the database handle and its count
    refused(matrix(a, b, [1, 2], [3, 25]), INVALID, "cols[1]", "25", "database handle", "19")
    refused(pairs(a, b, [1, 25], [3, 25]), INVALID, "c[1]", "25", "database handle", "19")
    refused(detect(a, b, [15, 16], [[1], [2, 25]]), INVALID, "candidate 1 = 25", "database handle", "19", "query 1")
    assert matrix(a, b, [25], [3], out_d[:1].copy(), None) == 0  # ... and it is fine as a row
    # row index 29
    refused(matrix(a, b, [1, 29], [3]), INVALID, "rows[1]", "29", "query handle", "(29 scans)")
    refused(top(a, b, [3, 29], None, 3), INVALID, "rows[1]", "29", "query handle")
    refused(pairs(a, b, [29], [3]), INVALID, "q[0]", "query handle", "(29 scans)")
    refused(pairs(a, b, [1, -1], [3, 3]), INVALID, "q[1]")
    refused(detect(a, b, [15, 29], [[1], [2]]), INVALID, "query index 29", "query handle")
    # k
    refused(top(a, b, None, None, 0), INVALID, "k = 0")
    refused(top(a, b, None, None, -2), INVALID, "k = -2")
    refused(top(a, b, None, None, 9), UNSUPPORTED, "k = 9", "GORIO_SC_TOP_MAX")
    with pytest.raises(gorio.GorioError) as e:
        a.top_matches(b, None, None, 9)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(gorio.GorioError) as e:
        a.top_matches(b, None, None, 0)
    assert e.value.code == INVALID
    # col_end
    ends = np.full(29, 19, np.int32)
    ends[4] = 20
    refused(top(a, b, None, ends, 3), INVALID, "col_end[4]", "20", "19")
    ends[4], ends[28] = 19, -1
    refused(top(a, b, None, ends, 3), INVALID, "col_end[28]", "-1")
    refused(top(a, a, None, np.full(29, 30), 1), INVALID, "col_end[0]", "30")
    # outputs and lists
    refused(matrix(a, b, [1], [2], None, None), INVALID, "both outputs are null")
    refused(lib.gorio_sc_cross_top_matches(a.h, None, 29, b.h, None, 3, None, p(out_d), None), INVALID, "null output")
    refused(detect(a, b, [15, 16], [[1], []]), INVALID, "empty candidate list", "query 1")
    # raw: a NULL extent list needs the whole database of its side, negative counts, and the 2^31 - 1 bound
    refused(lib.gorio_sc_cross_distance_matrix(a.h, None, 19, b.h, None, 19, p(out_d), None), INVALID, "rows", "29")
    refused(lib.gorio_sc_cross_distance_matrix(a.h, None, 29, b.h, None, 29, p(out_d), None), INVALID, "cols", "19")
    refused(lib.gorio_sc_cross_top_matches(a.h, None, 19, b.h, None, 3, p(out_i), p(out_d), None), INVALID, "rows", "29")
    refused(lib.gorio_sc_cross_distance_matrix(a.h, None, -1, b.h, None, 19, p(out_d), None), INVALID, "negative")
    refused(lib.gorio_sc_cross_distance_pairs(a.h, b.h, None, None, -1, p(out_d), None), INVALID, "count < 0")
    refused(lib.gorio_sc_cross_top_matches(a.h, None, -1, b.h, None, 3, p(out_i), p(out_d), None), INVALID, "negative")
    refused(lib.gorio_sc_cross_detect(a.h, b.h, -1, None, None, None, None, None, None), INVALID, "count < 0")
    refused(lib.gorio_sc_cross_distance_pairs(a.h, None, None, None, 0, None, None), INVALID, "null database handle")
    rows, cols = np.zeros(65536, np.int32), np.zeros(32768, np.int32)
    refused(lib.gorio_sc_cross_distance_matrix(a.h, p(rows), 65536, b.h, p(cols), 32768, p(out_d), None), UNSUPPORTED, "2^31")
    assert lib.gorio_sc_cross_distance_matrix(a.h, p(rows), 0, b.h, p(cols), 32768, None, None) == 0
    assert lib.gorio_sc_cross_distance_pairs(a.h, b.h, None, None, 0, None, None) == 0
    assert lib.gorio_sc_cross_top_matches(a.h, None, 0, b.h, None, 0, None, None, None) == 0
    assert lib.gorio_sc_cross_detect(a.h, b.h, 0, None, None, None, None, None, None) == 0
    assert (out_d == 7.0).all() and (out_i == 7).all() and (out_j == 7).all()
    after = (a.state(), b.state(), a.cross_counters(), b.cross_counters(), a.pairs_counters(), b.pairs_counters())
    for x, y in zip(before[:2], after[:2]):
        assert x["counter"] == y["counter"] and list(x["snapshot"]) == list(y["snapshot"]) and x["n_scans"] == y["n_scans"]
    before[2]["calls"] += 1  # the one accepted call above (row 25 of A)
    before[2]["pairs"] += 1
    before[2]["launches"] += 1
    before[2]["synchronisations"] += 1
    assert before[2:] == after[2:]
    other.close()
