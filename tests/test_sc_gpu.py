"""Intensity Scan Context on the MI355X (include/gorio_sc.h) against the NumPy restatement (tests/sc_restatement.py)."""
import numpy as np
import pytest

import sc_restatement as sr
import sc_scenes as ss

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def S(gorio, gpu):
    return gorio.scan_context


@pytest.fixture(scope="module")
def loop_seq():
    scans, info = ss.loop_sequence()
    return scans, info, ss.candidate_lists(len(scans))


def _odd_scans():
    """0 to 60 k points with NaN / Inf coordinates, NaN, negative and <= -1000 intensities, and an empty scan."""
    rng = np.random.default_rng(42)
    out = [(np.zeros((0, 3), F), np.zeros(0, F))]
    for n in [1, 7, 300, 5000, 60000]:
        xyz = np.stack([rng.uniform(-90, 90, n), rng.uniform(-90, 90, n), rng.normal(0, 2, n)], 1).astype(F)
        inten = rng.uniform(-20, 60, n).astype(F)
        m = max(n // 50, 1)
        idx = rng.choice(n, size=min(n, 6 * m), replace=False)
        g = np.array_split(idx, 6)
        xyz[g[0], 0] = np.nan
        xyz[g[1], 1] = np.nan
        xyz[g[2], rng.integers(0, 2)] = np.inf
        inten[g[3]] = np.nan
        inten[g[4]] = -1000.0
        inten[g[5]] = -rng.uniform(1, 999, g[5].size)
        xyz, inten = ss.drop_abs_band(xyz, inten)
        out.append((xyz, inten))
    return out


def test_descriptors_and_keys_match(S):
    sc = S.ScanContext()
    scans = _odd_scans() + [ss.keyframe(0.3 * k, 900 + k) for k in range(4)]
    first = sc.add_scans(scans)
    assert first == 0
    for k, (xyz, inten) in enumerate(scans):
        d, rk, sk = sc.descriptor(k)
        want = sr.make_scancontext(xyz, inten)
        assert (d == want).all(), k  # == : -0.0 and +0.0 are equal in the reference
        assert rk.tobytes() == sr.ring_key(want).tobytes()
        assert sk.tobytes() == sr.sector_key(want).tobytes()
    assert (sc.descriptor(0)[0] == 0).all()  # the empty scan


def test_batched_add_equals_single_adds(S):
    rng = np.random.default_rng(9)
    scans = []
    for k in range(256):
        n = int(rng.integers(0, 3000))
        xyz = rng.uniform(-85, 85, (n, 3)).astype(F)
        xyz[:, 0] = np.abs(xyz[:, 0])
        scans.append(ss.drop_abs_band(xyz, rng.uniform(-5, 40, n).astype(F)))
    a, b = S.ScanContext(), S.ScanContext()
    assert a.add_scans(scans) == 0
    for k, (x, i) in enumerate(scans):
        assert b.add_scan(x, i) == k
    assert a.state()["n_scans"] == b.state()["n_scans"] == 256
    for k in range(256):
        for u, v in zip(a.descriptor(k), b.descriptor(k)):
            assert u.tobytes() == v.tobytes(), k


def test_pair_distances(S, loop_seq):
    scans, _, _ = loop_seq
    pick = list(range(0, 160, 5))[:32] + list(range(82, 160, 5))[:32]
    sc = S.ScanContext()
    sc.add_scans([scans[k] for k in pick])
    descs = [sr.make_scancontext(*scans[k]) for k in pick]
    n_shift = 0
    for i in range(len(pick)):
        for j in range(len(pick)):
            d, s = sc.distance(i, j)
            wd, ws = sr.distance(descs[i], descs[j])
            assert s == ws, (i, j)
            assert abs(d - wd) <= 1e-12, (i, j, d, wd)
            n_shift += s != 0
    assert n_shift > 100


def _ref_run(scans, cands, queries):
    ref = sr.SCManagerRef()
    for x, i in scans:
        ref.add_scan(x, i)
    return ref, [ref.detect(q, cands[q]) for q in queries]


def _assert_same(got, want):
    lid, yaw, md, dg = got
    wl, wy, wm, wd = want
    assert lid == wl
    assert yaw == wy
    assert abs(md - wm) <= 1e-12 or md == wm
    for k in ["early_return", "rebuilt", "counter", "snapshot_size", "n_found"]:
        assert dg[k] == wd[k], k
    if dg["early_return"]:
        return
    assert list(dg["position"]) == list(wd["position"])
    assert dg["key_dist"].tobytes() == np.asarray(wd["key_dist"], F).tobytes()
    assert list(dg["keyframe"]) == list(wd["keyframe"])
    assert list(dg["sc_shift"]) == list(wd["sc_shift"])
    np.testing.assert_allclose(dg["sc_dist"], wd["sc_dist"], rtol=0, atol=1e-12)


def test_loop_sequence_matches(S, loop_seq):
    scans, _, cands = loop_seq
    sc = S.ScanContext()
    sc.add_scans(scans)
    queries = list(range(len(scans)))
    ref, want = _ref_run(scans, cands, queries)
    got = [sc.detect(q, cands[q]) for q in queries]
    # margins that make the comparison meaningful rather than lucky
    live = [w for w in want if not w[3]["early_return"]]
    md = np.array([w[2] for w in live if w[2] < 1e6])
    assert np.min(np.abs(md - 0.5)) > 1e-6
    gaps = [np.min(np.diff(w[3]["key_dist"][:w[3]["n_found"]].astype(np.float64))) for w in live if w[3]["n_found"] > 1]
    assert min(gaps) > 1e-3
    for q in queries:
        _assert_same(got[q], want[q])
    found = sum(1 for w in live if w[0] >= 0)
    rejected = sum(1 for w in live if w[0] < 0)
    assert found >= 5 and rejected >= 5
    assert any(w[3]["rebuilt"] for w in live) and any(not w[3]["rebuilt"] for w in live)
    assert any(-1 in list(w[3]["keyframe"]) for w in live)  # a stale position beyond the current list
    st = sc.state()
    assert st["counter"] == ref.counter and list(st["snapshot"]) == ref.snapshot


def test_shift_margins_on_the_sequence(loop_seq):
    """The three shift distances of every pair the sequence evaluates are far enough apart that 1e-12 cannot reorder them."""
    scans, _, cands = loop_seq
    ref, want = _ref_run(scans, cands, range(len(scans)))
    gaps = []
    for q, w in enumerate(want):
        for kf in w[3]["keyframe"]:
            if kf < 0:
                continue
            a, b = ref.descs[q], ref.descs[kf]
            al = sr.fast_align(sr.sector_key(a), sr.sector_key(b))
            d = [x for x in (sr.dist_direct(a, sr.circshift(b, s)) for s in sr.search_shifts(al)) if not np.isnan(x)]
            gaps += [abs(d[i] - d[j]) for i in range(len(d)) for j in range(i + 1, len(d))]
    assert len(gaps) > 100 and min(gaps) > 1e-7


def test_batch_equals_sequential(S, loop_seq):
    scans, _, cands = loop_seq
    a, b = S.ScanContext(), S.ScanContext()
    a.add_scans(scans)
    b.add_scans(scans)
    queries = list(range(len(scans)))
    seq = [a.detect(q, cands[q]) for q in queries]
    bat = b.detect_batch(queries, [cands[q] for q in queries])
    for x, y in zip(seq, bat):
        _assert_same(y, x)
    assert a.state()["counter"] == b.state()["counter"]
    assert list(a.state()["snapshot"]) == list(b.state()["snapshot"])
    # one more single call agrees after the batch
    _assert_same(b.detect(150, cands[90]), a.detect(150, cands[90]))


def test_large_database_knn(S):
    rng = np.random.default_rng(77)
    n_db = 20000
    sc = S.ScanContext()
    for start in range(0, n_db, 2500):
        scans = []
        for _ in range(2500):
            m = int(rng.integers(20, 60))
            xyz = np.stack([rng.uniform(1, 79, m), rng.uniform(-40, 40, m), np.zeros(m)], 1).astype(F)
            scans.append(ss.drop_abs_band(xyz, rng.uniform(0, 100, m).astype(F)))
        sc.add_scans(scans)
    keys = np.stack([sc.descriptor(k)[1] for k in range(n_db)]).astype(F)
    queries = [int(q) for q in rng.choice(np.arange(10000, n_db), 64, replace=False)]
    cand = [np.sort(rng.choice(n_db, 5000, replace=False)).astype(np.int32) for _ in queries]
    res = sc.detect_batch(queries, cand)
    snap = None
    for i, (q, c) in enumerate(zip(queries, cand)):
        if i % 10 == 0:
            snap = [int(k) for k in c if (q - int(k)) % (1 << 64) >= 10]
        pos, kd, n = sr.knn(keys[q], keys[snap])
        dg = res[i][3]
        assert dg["snapshot_size"] == len(snap) and len(snap) > 4000
        assert list(dg["position"]) == list(pos), i
        assert dg["key_dist"].tobytes() == kd.tobytes(), i


def test_errors_leave_state_unchanged(S, gorio):
    scans, _ = ss.loop_sequence(n_lap=12, n_points=500)
    sc = S.ScanContext()
    sc.add_scans(scans)
    sc.detect(15, list(range(5)))
    before = sc.state()
    for q, c in [(15, []), (16, [3, 999]), (24, [1, 2]), (-1, [1])]:
        with pytest.raises(gorio.GorioError) as e:
            sc.detect(q, c)
        assert e.value.code == -1  # GORIO_ERR_INVALID
    with pytest.raises(gorio.GorioError):
        sc.detect_batch([15, 16, 30], [[1], [2], [3]])  # query 30 not yet added: nothing runs
    with pytest.raises(gorio.GorioError):
        sc.distance(0, 24)
    with pytest.raises(gorio.GorioError):
        sc.descriptor(24)
    after = sc.state()
    assert after["counter"] == before["counter"] and list(after["snapshot"]) == list(before["snapshot"]) and after["n_scans"] == 24
