"""Pose-graph edges between resident keyframes (include/gorio_kf_edges.h) on the MI355X.  The score of an edge is DEFINED as what
gorio_apd_fitness_score returns on a fresh pruned-search handle that was handed the two keyframes; every comparison with it is `==` on
doubles.  Keyframe sizes sit on both sides of the wave (64), the reduction block (256) and the search's padding (512), plus two scan-sized
ones; one batch mixes them all on both sides."""
import importlib
import math

import numpy as np
import pytest

synth = importlib.import_module("go-rio_amd.synth")

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -3
DBL_MAX = float(np.finfo(np.float64).max)
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2000, 5000]  # keyframe id = position
RANGES = [DBL_MAX, 4.0, 0.01]  # the reference's max_range: SQUARED distances
KW = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)  # search = 1: GORIO_SEARCH_PRUNED


def _pose(k):
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0.1 * k, -0.2 * k, 0.5 * k])
    T[:3, 3] = [0.1 * k, -0.05 * k, 0.02 * k]
    return T


FAR = np.eye(4)
FAR[0, 3] = 1000.0
# (target id, source id, relpose)
EDGES = [
    (11, 10, _pose(1)), (8, 10, _pose(2)), (0, 10, _pose(3)), (5, 10, _pose(4)),  # keyframe 10 is the source of four edges, four poses
    (11, 0, _pose(5)), (11, 1, _pose(6)), (11, 2, _pose(7)), (11, 3, _pose(8)), (11, 4, _pose(9)),  # keyframe 11 is the target of these five (and more)
    (11, 11, np.eye(4)),  # a keyframe against itself
    (10, 9, FAR),         # the source moved 1 km away
    (1, 5, _pose(1)), (2, 6, _pose(2)), (3, 7, _pose(3)), (4, 8, _pose(4)), (6, 9, _pose(5)), (7, 11, _pose(6)), (9, 8, _pose(7)),
    (10, 11, _pose(8)), (0, 0, np.eye(4)), (10, 8, _pose(9)), (8, 7, _pose(3)), (10, 6, _pose(4)), (6, 5, _pose(5)),
]
SELF, FAR_EDGE = 9, 10
ORACLE_EDGES = [1, 20, 22]  # both sides <= 2000 points


def _clouds():
    out = []
    for i, n in enumerate(SIZES):
        pose = np.eye(4)
        pose[:3, 3] = [0.05 * i, 0.02 * i, 0.0]
        out.append(synth.radar_scan(n, seed=500 + i, sensor_pose=pose))
    return out


def _store(gorio, clouds):
    store = gorio.KeyframeStore()
    for i, (xyz, lab) in enumerate(clouds):
        assert store.add(xyz, None, lab) == i
    return store


def _single(gorio, store, edge, max_range):
    """The definition: a fresh pruned-search handle, the two keyframe hand-offs, gorio_apd_fitness_score at the float cast of the pose."""
    tgt, src, T = edge
    g = gorio.ApdGicp(**KW)
    g.setInputTargetKeyframe(store, tgt)
    g.setInputSourceKeyframe(store, src)
    return g.getFitnessScore(np.asarray(T, np.float64).astype(np.float32), max_range=max_range, inlier_dist=0.0)[0]


@pytest.fixture(scope="module")
def scene(gpu, gorio):
    """The store, the batch scored once per max_range (first thing done with the store: its first call builds every index), the counters
    around those calls, and the definition's score of every edge from a second store that no edge call has touched."""
    clouds = _clouds()
    store = _store(gorio, clouds)
    before = dict(info=[store.info(i) for i in range(len(SIZES))], counters=store.counters(), edge=store.edge_counters())
    batch, after_call = {}, []
    for r in RANGES:
        batch[r] = store.edge_fitness(EDGES, r)
        after_call.append(store.edge_counters())
    after = dict(info=[store.info(i) for i in range(len(SIZES))], counters=store.counters())
    plain = _store(gorio, clouds)
    want = {r: np.array([_single(gorio, plain, e, r) for e in EDGES]) for r in RANGES}
    yield dict(store=store, clouds=clouds, batch=batch, want=want, before=before, after=after, after_call=after_call)
    store.close()
    plain.close()


@pytest.mark.parametrize("max_range", RANGES)
def test_batch_equals_the_single_call_on_a_fresh_handle(scene, max_range):
    score, nr = scene["batch"][max_range]
    want = scene["want"][max_range]
    print(score, want, nr)
    assert score.dtype == np.float64 and len(score) == len(EDGES) == 24
    for e in range(len(EDGES)):
        assert score[e] == want[e], (e, EDGES[e][:2], score[e], want[e])
    # the self edge: every point finds itself
    assert score[SELF] == 0.0 and nr[SELF] == SIZES[11]
    assert score[19] == 0.0 and nr[19] == 1
    if max_range != DBL_MAX:
        assert score[FAR_EDGE] == DBL_MAX and nr[FAR_EDGE] == 0
    else:
        assert nr[FAR_EDGE] == SIZES[9] and 0.64e6 < score[FAR_EDGE] < 1.44e6  # (1 km -+ the 200 m a scene spans at most)^2
        assert all(nr[e] == SIZES[EDGES[e][1]] for e in range(len(EDGES)))  # no limit: every source point counts
    # the ranges do cut: the tight one drops points of ordinary edges
    if max_range == 0.01:
        assert nr[0] < SIZES[10]


@pytest.mark.parametrize("max_range", RANGES)
def test_edge_by_edge_and_reversed_give_the_same_bits(scene, max_range):
    store = scene["store"]
    score, nr = scene["batch"][max_range]
    for e, edge in enumerate(EDGES):
        s1, n1 = store.edge_fitness([edge], max_range)
        assert s1[0] == score[e] and n1[0] == nr[e], (e, s1[0], score[e])
    sr, nrr = store.edge_fitness(EDGES[::-1], max_range)
    assert np.array_equal(sr[::-1], score) and np.array_equal(nrr[::-1], nr)


@pytest.mark.parametrize("max_range", RANGES)
def test_score_equals_the_cpu_oracle(scene, oracle_apd, max_range):
    """The statistic tests/test_apd_gpu.py::test_transform_source_and_fitness checks, with its tolerance; the count is exact."""
    score, nr = scene["batch"][max_range]
    p = oracle_apd.default_params()
    for e in ORACLE_EDGES:
        tgt, src, T = EDGES[e]
        sx, tx = scene["clouds"][src][0], scene["clouds"][tgt][0]
        assert len(sx) <= 2000 and len(tx) <= 2000
        Td = np.asarray(T, np.float64).astype(np.float32).astype(np.float64)
        _, sqd, _ = oracle_apd.update_correspondences(Td, sx, tx, np.zeros((len(sx), 4, 4)), np.zeros((len(tx), 4, 4)), p)
        d = sqd.astype(np.float64)
        keep = d <= max_range
        print(e, score[e], nr[e], int(keep.sum()))
        assert nr[e] == int(keep.sum())
        if keep.any():
            assert score[e] == pytest.approx(float(np.mean(d[keep])), rel=1e-12)
        else:
            assert score[e] == DBL_MAX


def test_state_and_counters(scene):
    before, after, calls = scene["before"], scene["after"], scene["after_call"]
    assert before["edge"] == dict(calls=0, edges_scored=0, index_builds=0, synchronisations=0)
    for i, n in enumerate(SIZES):
        assert before["info"][i]["index_built"] == 0 and after["info"][i]["index_built"] == 1  # every keyframe is named by the batch
        assert after["info"][i]["cov_count"] == before["info"][i]["cov_count"] == 0 and after["info"][i]["sharers"] == 0
    assert after["counters"] == before["counters"] == dict(point_uploads=len(SIZES), point_downloads=0, device_copies=0)
    # one synchronisation per call whatever the count; the indexes are built by the first call and found by the others
    assert calls[0] == dict(calls=1, edges_scored=24, index_builds=len(SIZES), synchronisations=1)
    assert calls[1] == dict(calls=2, edges_scored=48, index_builds=len(SIZES), synchronisations=2)
    assert calls[2] == dict(calls=3, edges_scored=72, index_builds=len(SIZES), synchronisations=3)
    store = scene["store"]
    c0 = store.edge_counters()
    store.edge_fitness(EDGES[:1])
    store.edge_information(EDGES[:7])
    c1 = store.edge_counters()
    assert (c1["calls"] - c0["calls"], c1["edges_scored"] - c0["edges_scored"], c1["index_builds"] - c0["index_builds"], c1["synchronisations"] - c0["synchronisations"]) == (2, 8, 0, 2)


def test_empty_keyframes_score_dbl_max_and_leave_the_others_alone(gpu, gorio, scene):
    clouds = scene["clouds"]
    store = gorio.KeyframeStore()
    a = store.add(*[clouds[7][0], None, clouds[7][1]])
    empty = store.add(np.zeros((0, 3), np.float32))
    b = store.add(*[clouds[10][0], None, clouds[10][1]])
    edges = [(b, a, _pose(3)), (empty, a, _pose(1)), (b, empty, _pose(2)), (empty, empty, np.eye(4)), (a, b, _pose(4))]
    for r in RANGES:
        score, nr = store.edge_fitness(edges, r)
        assert list(score[1:4]) == [DBL_MAX] * 3 and list(nr[1:4]) == [0, 0, 0]
        alone, nra = store.edge_fitness([edges[0], edges[4]], r)
        assert score[0] == alone[0] and score[4] == alone[1] and nr[0] == nra[0] and nr[4] == nra[1]
        assert score[0] == _single(gorio, store, edges[0], r) and score[4] == _single(gorio, store, edges[4], r)
    c = store.edge_counters()
    s, n = store.edge_fitness([(empty, empty, np.eye(4))])  # nothing to launch: no synchronisation either
    assert s[0] == DBL_MAX and n[0] == 0
    c2 = store.edge_counters()
    assert c2["synchronisations"] == c["synchronisations"] and c2["calls"] == c["calls"] + 1
    assert store.info(empty)["index_built"] == 0
    store.close()


def test_refusals_change_nothing(gpu, gorio, scene):
    clouds = scene["clouds"]
    store = gorio.KeyframeStore()
    a = store.add(clouds[8][0])
    b = store.add(clouds[9][0])
    gone = store.add(clouds[3][0])
    store.release(gone)
    good = [(a, b, _pose(2)), (b, a, _pose(5))]
    s0, n0 = store.edge_fitness(good, 4.0)
    c0 = store.edge_counters()
    with pytest.raises(gorio.GorioError) as e:  # a released id
        store.edge_fitness(good + [(a, gone, np.eye(4))], 4.0)
    assert e.value.code == STATE and "edges[2]" in str(e.value) and "released" in str(e.value)
    with pytest.raises(gorio.GorioError) as e:
        store.edge_information([(gone, a, np.eye(4))])
    assert e.value.code == STATE and "edges[0]" in str(e.value)
    with pytest.raises(gorio.GorioError) as e:  # an id never added
        store.edge_fitness([(a, 17, np.eye(4))])
    assert e.value.code == INVALID and "edges[0]" in str(e.value)
    for bad in (float("nan"), float("inf")):  # a non-finite pose entry: the text names the edge and the entry
        T = np.eye(4)
        T[1, 3] = bad
        with pytest.raises(gorio.GorioError) as e:
            store.edge_fitness(good + [(a, b, T)])
        assert e.value.code == INVALID and "edges[2]" in str(e.value) and "relpose[7]" in str(e.value)
    with pytest.raises(gorio.GorioError) as e:
        store.edge_fitness(good, float("nan"))
    assert e.value.code == INVALID
    assert store.edge_counters() == c0
    s1, n1 = store.edge_fitness(good, 4.0)
    assert np.array_equal(s1, s0) and np.array_equal(n1, n0)
    store.close()


def test_a_sharing_handle_aligns_to_the_same_bits_around_an_edge_call(gpu, gorio):
    sx, sl, tx, tl, _ = synth.scan_pair(2048, 2048, seed=1)
    store = gorio.KeyframeStore()
    s, t = store.add(sx, None, sl), store.add(tx, None, tl)
    g = gorio.ApdGicp(**KW)
    g.setInputTargetKeyframe(store, t)
    g.setInputSourceKeyframe(store, s)
    r1 = g.align()
    info = [store.info(s), store.info(t)]
    assert info[0]["cov_count"] == 2048 and info[0]["sharers"] == 1
    score, nr = store.edge_fitness([(t, s, r1["T"]), (s, t, np.linalg.inv(r1["T"].astype(np.float64))), (s, s, np.eye(4))])
    assert score[0] == g.getFitnessScore(r1["T"])[0] and score[2] == 0.0 and nr[2] == 2048
    assert [store.info(s), store.info(t)] == info  # covariances, index and sharers as they were
    assert store.edge_counters()["index_builds"] == 0  # the align had built both indexes: the edge call found them
    r2 = g.align()
    assert r2["T"].tobytes() == r1["T"].tobytes() and r2["H"].tobytes() == r1["H"].tobytes()
    assert (r2["converged"], r2["nr_iterations"], r2["n_linearize"]) == (r1["converged"], r1["nr_iterations"], r1["n_linearize"]) and r1["nr_iterations"] >= 1
    store.close()


def _restated(score, a=20.0, thresh=0.5, min_sx=0.1, max_sx=5.0, min_sq=0.05, max_sq=0.2):
    def weight(max_x, min_y, max_y, x):
        y = (1.0 - math.exp(-a * x)) / (1.0 - math.exp(-a * max_x))
        return min_y + (max_y - min_y) * y

    return 1.0 / float(np.float32(weight(thresh, min_sx ** 2, max_sx ** 2, score))), 1.0 / float(np.float32(weight(thresh, min_sq ** 2, max_sq ** 2, score)))


def test_information_is_the_restatement_of_the_scores(scene):
    store = scene["store"]
    inf, score = store.edge_information(EDGES)
    assert np.array_equal(score, scene["batch"][DBL_MAX][0])  # calc_fitness_score with max_range at its default
    for e in range(len(EDGES)):
        rx, rq = _restated(float(score[e]))
        assert inf[e, 0] == pytest.approx(rx, rel=2.3e-16, abs=0.0) and inf[e, 1] == pytest.approx(rq, rel=2.3e-16, abs=0.0)
    assert inf[SELF, 0] == pytest.approx(100.0, rel=1e-6) and inf[SELF, 1] == pytest.approx(400.0, rel=1e-6)  # a perfect fit: 1 / min_stddev^2
    inf2, score2 = store.edge_information(EDGES, fitness_score_thresh=2.5, var_gain_a=5.0)
    assert np.array_equal(score2, score)
    for e in (0, 5, FAR_EDGE):
        rx, rq = _restated(float(score[e]), a=5.0, thresh=2.5)
        assert inf2[e, 0] == pytest.approx(rx, rel=2.3e-16, abs=0.0) and inf2[e, 1] == pytest.approx(rq, rel=2.3e-16, abs=0.0)
