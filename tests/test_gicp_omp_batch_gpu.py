"""Batched GICP_OMP aligns on the GPU (gorio_apd_gicp_omp_align_batch, go-rio_amd/csrc/apd_gicp_omp.hip) on the scenes of
tests/gicp_omp_batch_scenes.py.  Gates: every handle of a batch ends bit for bit where its own align() on a fresh handle ends (pose, counts,
diag values, correspondences, Mahalanobis matrices), in both search modes; against the NumPy restatement the pose holds to 1e-4 m /
1e-4 rad with equal outer, inner and evaluation counts (the gate of test_gicp_omp_gpu.check_align), on all ten scenes, which all pass the
restatement's stability condition; the lock-step round count is the longest member's."""
import importlib

import numpy as np
import pytest

import gicp_omp_batch_scenes as B
import gicp_omp_scenes as S

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SEARCHES = [apd.SEARCH_BRUTE_FORCE, apd.SEARCH_PRUNED]


def handle(gorio, gpu, scene, search, upload=True, **over):
    """test_gicp_omp_gpu.handle() with max_correspondence_distance = 0.5 for every handle."""
    p = dict(scene["params"])
    kw = dict(k_correspondences=20, max_iterations=p.get("max_iterations", 200), transformation_epsilon=5e-4, rotation_epsilon=2e-3,
              corr_dist_threshold=p.get("max_correspondence_distance", 5.0), search=search, keep_knn_indices=1)
    kw.update(over)
    g = gorio.ApdGicp(device=gpu, **kw)
    g.set_method(apd.METHOD_GICP_OMP)
    g.setGicpOmpParams(1e-3, p.get("max_optimizer_iterations", 20))
    if upload:
        g.setInputTarget(scene["target"])
        g.setInputSource(scene["source"])
    return g


def state_of(g, r):
    """Everything an align leaves behind that a caller can read."""
    corr, sqd = g.getCorrespondences()
    return dict(T=r["T"].copy(), converged=r["converged"], nr_iterations=r["nr_iterations"], n_linearize=r["n_linearize"], diag=g.gicpOmpDiag(), corr=corr, sqd=sqd,
                maha=g.getMahalanobis())


def assert_same_bits(got, want, what):
    assert got["T"].tobytes() == want["T"].tobytes(), what
    assert (got["converged"], got["nr_iterations"], got["n_linearize"]) == (want["converged"], want["nr_iterations"], want["n_linearize"]), what
    assert got["diag"] == want["diag"], what
    assert np.array_equal(got["corr"], want["corr"]) and got["sqd"].tobytes() == want["sqd"].tobytes(), what
    assert got["maha"].tobytes() == want["maha"].tobytes(), what


_single = {}


def single(gorio, gpu, name, search):
    """The state after align() on a fresh handle with the scene's inputs, computed once per (scene, search)."""
    if (name, search) not in _single:
        sc = B.all_scenes()[name]
        g = handle(gorio, gpu, sc, search)
        _single[(name, search)] = state_of(g, g.align(sc["guess"]))
    return _single[(name, search)]


def check_restatement(name, got):
    """The gate of test_gicp_omp_gpu.check_align; no scene is left out: every one passes the stability condition."""
    assert B.is_stable(name), name
    want = B.reference(name)
    dt, dr = S.pose_error(want["T"], got["T"])
    print("%s: %d / %d outer, %d / %d inner, %d / %d evaluations, pose error %.3e m %.3e rad" % (name, got["nr_iterations"], want["nr_iterations"], got["diag"]["inner_total"],
                                                                                               want["inner_total"], got["n_linearize"], want["evaluations"], dt, dr))
    assert got["converged"] == want["converged"]
    assert (got["nr_iterations"], got["diag"]["inner_total"]) == (want["nr_iterations"], want["inner_total"]) and got["diag"]["outer"] == got["nr_iterations"]
    assert got["n_linearize"] == got["diag"]["evaluations"] == want["evaluations"]
    assert dt <= 1e-4 and dr <= 1e-4


def expected_rounds(states):
    """Every unfinished handle advances in every round: evaluations + updates of the longest member; an align that ended by a break made
    one update more than its outer count."""
    return max(s["n_linearize"] + s["nr_iterations"] + (0 if s["converged"] else 1) for s in states)


def run_batch(gorio, objs, scenes):
    res = gorio.gicp_omp_align_batch(objs, np.stack([sc["guess"] for _, sc in scenes]))
    return res, [state_of(g, r) for g, r in zip(objs, res)]


@pytest.mark.parametrize("search", SEARCHES)
def test_mixed_batch(gorio, gpu, search):
    scenes = B.mixed()
    objs = [handle(gorio, gpu, sc, search) for _, sc in scenes]
    res, states = run_batch(gorio, objs, scenes)
    for (name, sc), st in zip(scenes, states):
        assert_same_bits(st, single(gorio, gpu, name, search), name)
        check_restatement(name, st)
    three = states[1]  # ends at its first update while the others go on
    assert not three["converged"] and three["nr_iterations"] == 0 and np.array_equal(three["T"], scenes[1][1]["guess"])
    assert states[0]["converged"] and int((states[0]["corr"] >= 0).sum()) == 4
    assert (states[3]["nr_iterations"], states[3]["n_linearize"]) == (1, 1)
    diag = res[0]["batch_diag"]
    print("mixed batch: %d rounds, %d launches; one by one %d round trips" % (diag["rounds"], diag["launches"], sum(s["n_linearize"] + s["nr_iterations"] + (0 if s["converged"] else 1)
                                                                                                               for s in states)))
    assert diag["rounds"] == expected_rounds(states) == 123
    assert diag["launches"] <= 4 * diag["rounds"] + len(objs)


@pytest.mark.parametrize("search", SEARCHES)
def test_loop_closure_shape(gorio, gpu, search):
    scenes = B.loop_closure()
    owner = handle(gorio, gpu, scenes[0][1], search, upload=False)
    owner.setInputTarget(scenes[0][1]["target"])
    objs = []
    for _, sc in scenes:
        g = handle(gorio, gpu, sc, search, upload=False)
        g.setInputTargetShared(owner)
        g.setInputSource(sc["source"])
        objs.append(g)
    for g in objs:
        g.setProfiling(True)
    res, states = run_batch(gorio, objs, scenes)
    for (name, sc), st in zip(scenes, states):
        assert_same_bits(st, single(gorio, gpu, name, search), name)
        check_restatement(name, st)
    diag = res[0]["batch_diag"]
    assert diag["rounds"] == expected_rounds(states)
    assert diag["launches"] <= 4 * diag["rounds"] + len(objs)
    # the shared target's covariances and index were made once: one covariance stage (0) and one index stage (4, pruned search only) over
    # the whole batch, all clouds in it; a second batch finds everything valid and adds none
    def stages():
        counts = np.sum([g.getStageTimes()[1] for g in objs], axis=0)
        return int(counts[0]), int(counts[4])
    assert stages() == (1, 1 if search == apd.SEARCH_PRUNED else 0)
    assert owner.getTargetCovariances().tobytes() == objs[-1].getTargetCovariances().tobytes()
    res2, states2 = run_batch(gorio, objs, scenes)
    assert stages() == (1, 1 if search == apd.SEARCH_PRUNED else 0)
    for st, st2 in zip(states, states2):
        assert_same_bits(st2, st, "second batch")


@pytest.mark.parametrize("search", SEARCHES)
def test_batch_of_one_and_reversed_order(gorio, gpu, search):
    scenes = B.mixed()
    name, sc = scenes[2]
    g = handle(gorio, gpu, sc, search)
    r = gorio.gicp_omp_align_batch([g], sc["guess"][None])
    assert_same_bits(state_of(g, r[0]), single(gorio, gpu, name, search), "batch of one")
    assert r[0]["batch_diag"]["rounds"] == r[0]["n_linearize"] + r[0]["nr_iterations"]
    rev = scenes[::-1]
    objs = [handle(gorio, gpu, s, search) for _, s in rev]
    _, states = run_batch(gorio, objs, rev)
    for (n, _), st in zip(rev, states):
        assert_same_bits(st, single(gorio, gpu, n, search), "reversed " + n)


def test_per_handle_settings_may_differ(gorio, gpu):
    scenes = B.mixed()
    sc = scenes[2][1]
    a = handle(gorio, gpu, sc, apd.SEARCH_BRUTE_FORCE)
    a.setGicpOmpParams(1e-3, 1)
    b = handle(gorio, gpu, sc, apd.SEARCH_BRUTE_FORCE)
    b.setGicpOmpParams(1e-2, 20)
    res = gorio.gicp_omp_align_batch([a, b], np.stack([sc["guess"], sc["guess"]]))
    sa, sb = state_of(a, res[0]), state_of(b, res[1])
    a1 = handle(gorio, gpu, sc, apd.SEARCH_BRUTE_FORCE)
    a1.setGicpOmpParams(1e-3, 1)
    b1 = handle(gorio, gpu, sc, apd.SEARCH_BRUTE_FORCE)
    b1.setGicpOmpParams(1e-2, 20)
    assert_same_bits(sa, state_of(a1, a1.align(sc["guess"])), "max_optimizer_iterations = 1")
    assert_same_bits(sb, state_of(b1, b1.align(sc["guess"])), "gicp_epsilon = 1e-2")
    assert sa["diag"]["inner_total"] == sa["nr_iterations"]  # the cap of 1 held
    assert sa["T"].tobytes() != sb["T"].tobytes()
    assert a.getSourceCovariances().tobytes() == a1.getSourceCovariances().tobytes() and b.getSourceCovariances().tobytes() == b1.getSourceCovariances().tobytes()


def test_refusals(gorio, gpu):
    scenes = B.mixed()
    sc, sc2 = scenes[2][1], scenes[4][1]
    search = apd.SEARCH_BRUTE_FORCE
    g, g2 = handle(gorio, gpu, sc, search), handle(gorio, gpu, sc2, search)
    before = [state_of(g, g.align(sc["guess"])), state_of(g2, g2.align(sc2["guess"]))]
    plain = gorio.ApdGicp(device=gpu, corr_dist_threshold=0.5, k_correspondences=20, max_iterations=200, transformation_epsilon=5e-4, rotation_epsilon=2e-3, search=search,
                          keep_knn_indices=1)
    plain.setInputTarget(sc["target"])
    plain.setInputSource(sc["source"])
    other_thr = handle(gorio, gpu, sc, search, corr_dist_threshold=0.6)
    no_source = handle(gorio, gpu, sc, search, upload=False)
    no_source.setInputTarget(sc["target"])
    tiny = handle(gorio, gpu, dict(sc, source=S.room(19, 5)), search)
    cases = [([g, g2, g], INVALID, "handle 2"), ([g, plain, g2], STATE, "handle 1"), ([g, g2, other_thr], INVALID, "handle 2"), ([g, no_source, g2], STATE, "handle 1"),
             ([g, g2, tiny], INVALID, "handle 2")]
    for objs, code, where in cases:
        with pytest.raises(gorio.GorioError) as e:
            gorio.gicp_omp_align_batch(objs)
        assert e.value.code == code and where in str(e.value), (code, where, str(e.value))
        assert_same_bits(state_of(g, g.align(sc["guess"])), before[0], "after refusal " + where)
        assert_same_bits(state_of(g2, g2.align(sc2["guess"])), before[1], "after refusal " + where)
    assert "k_correspondences" in str(e.value)
    assert plain.get_method()["method"] == apd.METHOD_APDGICP and plain.align()["converged"] in (True, False)
    with pytest.raises(gorio.GorioError) as e:
        gorio.align_batch([g])
    assert e.value.code == UNSUPPORTED


def test_keyframe_hand_off(gorio, gpu):
    scenes = B.loop_closure()[:3]
    search = apd.SEARCH_PRUNED
    store = gorio.KeyframeStore(device=gpu)
    kt = store.add(scenes[0][1]["target"])
    objs = []
    for _, sc in scenes:
        g = handle(gorio, gpu, sc, search, upload=False)
        g.setInputTargetKeyframe(store, kt)
        g.setInputSourceKeyframe(store, store.add(sc["source"]))
        objs.append(g)
    _, states = run_batch(gorio, objs, scenes)
    for (name, _), st in zip(scenes, states):
        assert_same_bits(st, single(gorio, gpu, name, search), "keyframes " + name)
