"""GICP_OMP on the GPU (GORIO_METHOD_GICP_OMP, go-rio_amd/csrc/apd_gicp_omp.hip) against the NumPy restatement
(tests/gicp_omp_restatement.py) on the scenes of tests/gicp_omp_scenes.py.  Gates: k-NN lists, pairs and float distances bit for
bit; covariances, Mahalanobis matrices, f and g to 1e-9 relative; final pose to 1e-4 m / 1e-4 rad with equal outer and inner counts on
the scenes that pass the restatement's own stability condition."""
import ctypes as C
import importlib

import numpy as np
import pytest

import gicp_omp_restatement as R
import gicp_omp_scenes as S

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
INVALID, UNSUPPORTED = -1, -5
F32_HALF_ULP = 2.0 ** -24


def handle(gorio, gpu, scene, search=apd.SEARCH_BRUTE_FORCE, upload=True):
    p = dict(scene["params"])
    g = gorio.ApdGicp(device=gpu, k_correspondences=20, max_iterations=p.get("max_iterations", 200), transformation_epsilon=5e-4, rotation_epsilon=2e-3,
                      corr_dist_threshold=p.get("max_correspondence_distance", 5.0), search=search, keep_knn_indices=1)
    g.set_method(apd.METHOD_GICP_OMP)
    g.setGicpOmpParams(1e-3, p.get("max_optimizer_iterations", 20))
    if upload:
        g.setInputTarget(scene["target"])
        g.setInputSource(scene["source"])
    return g


def check_parts(g, ref, scene, degenerate_ok=False):
    """k-NN lists, covariances, one update at the identity, the three evaluations."""
    g.calculateCovariances()
    ref.compute_covariances()
    assert np.array_equal(g.getKnnIndices(0), ref.knn_src) and np.array_equal(g.getKnnIndices(1), ref.knn_tgt)
    for got, want, cloud, lists in ((g.getSourceCovariances(), ref.C1, ref.src, ref.knn_src), (g.getTargetCovariances(), ref.C2, ref.tgt, ref.knn_tgt)):
        err = np.abs(got[:, :3, :3] - want).max(axis=(1, 2))
        if degenerate_ok:  # equal smallest singular values leave U's last columns free: compare where the gap is resolved in double
            s = R.covariances(cloud, lists)[1]
            err = err[(s[:, 1] - s[:, 2]) > 1e-6 * s[:, 0]]
        print("covariances: max abs error %.3e over %d points" % (err.max() if err.size else 0.0, err.size))
        assert (err <= 1e-9).all()  # entries are O(1): singular values 1, 1, 1e-3
        assert (got[:, 3, :] == 0).all() and (got[:, :, 3] == 0).all()
    eye = np.eye(4, dtype=np.float32)
    out = R.transform_f(scene["guess"], ref.src)
    C1, C2 = ref.C1, ref.C2
    if degenerate_ok:  # where a covariance is undetermined, so is the Mahalanobis matrix built from it: that step is compared on the device's own covariances
        C1, C2 = g.getSourceCovariances()[:, :3, :3].copy(), g.getTargetCovariances()[:, :3, :3].copy()
    corr, d, M, Mf = R.update(eye, scene["guess"], out, ref.tgt, C1, C2, ref.corr_dist)
    m = g.gicpOmpUpdate(eye, scene["guess"])
    gc, gd = g.getCorrespondences()
    assert m == int((corr >= 0).sum()) and np.array_equal(gc, corr)
    assert np.array_equal(gd[corr >= 0], d[corr >= 0])
    gm = g.getMahalanobis()[:, :3, :3]
    scale = np.abs(M).max(axis=(1, 2), keepdims=True)
    # the hook returns the stored floats: the double matrix to 1e-9 of its largest entry, then one rounding to float of each entry
    assert (np.abs(gm - M) <= 1e-9 * scale + F32_HALF_ULP * np.abs(M) * (1 + 1e-6)).all()
    assert (gm[corr < 0] == 0).all()
    if m == 0:
        return
    fun = R.Functor(out, ref.tgt, gc, gm.astype(np.float32))  # the device's own float matrices: the functor is compared on equal inputs
    for x in (np.zeros(6), np.array([0.03, -0.02, 0.01, 0.004, -0.006, 0.01])):
        f0, _ = g.gicpOmpEvaluate(x, apd.GICP_OMP_F)
        _, g1 = g.gicpOmpEvaluate(x, apd.GICP_OMP_DF)
        f2, g2 = g.gicpOmpEvaluate(x, apd.GICP_OMP_FDF)
        rf, (rf2, rg) = fun.f(x), fun.fdf(x)
        print("evaluate: f %.12e / %.12e, fdf f %.12e / %.12e, max |g - ref| %.3e of %.3e" % (f0, rf, f2, rf2, np.abs(g2 - rg).max(), np.abs(rg).max()))
        assert abs(f0 - rf) <= 1e-9 * abs(rf) and abs(f2 - rf2) <= 1e-9 * abs(rf2)
        assert np.array_equal(g1, g2) and (np.abs(g2 - rg) <= 1e-9 * np.abs(rg).max()).all()


def check_align(g, name):
    sc = S.scenes()[name]
    _, want = S.reference(name)
    r = g.align(sc["guess"])
    diag = g.gicpOmpDiag()
    dt, dr = S.pose_error(want["T"], r["T"])
    print("%s: %d / %d outer, %d / %d inner, %d / %d evaluations, pose error %.3e m %.3e rad" % (name, r["nr_iterations"], want["nr_iterations"], diag["inner_total"],
                                                                                               want["inner_total"], r["n_linearize"], want["evaluations"], dt, dr))
    assert r["converged"] == want["converged"] and (r["H"] == 0).all()
    if S.is_stable(name):
        assert (r["nr_iterations"], diag["inner_total"]) == (want["nr_iterations"], want["inner_total"]) and diag["outer"] == r["nr_iterations"]
        assert r["n_linearize"] == diag["evaluations"] == want["evaluations"]
        assert dt <= 1e-4 and dr <= 1e-4
    return r


@pytest.mark.parametrize("name,search", [(n, apd.SEARCH_BRUTE_FORCE) for n in sorted(S.scenes())] + [("general", apd.SEARCH_PRUNED), ("four_pairs", apd.SEARCH_PRUNED)])
def test_scene(gorio, gpu, name, search):
    sc = S.scenes()[name]
    g = handle(gorio, gpu, sc, search)
    ref, want = S.reference(name)
    check_parts(g, ref, sc)
    r = check_align(g, name)
    if name in ("three_pairs", "no_pairs"):
        assert not r["converged"] and r["nr_iterations"] == 0 and np.array_equal(r["T"], sc["guess"])
    if name == "four_pairs":
        assert g.gicpOmpUpdate(np.eye(4, dtype=np.float32), sc["guess"]) == 4 and r["converged"]
    if name == "outer_cap":
        assert r["nr_iterations"] == 1 and r["converged"]
    if name == "inner_cap":
        assert g.gicpOmpDiag()["inner_total"] == r["nr_iterations"]
    if name == "identical":
        assert r["nr_iterations"] == 1 and r["converged"] and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
    # the rest of the handle keeps working in this mode: fitness score and transformed source
    score, _ = g.getFitnessScore(r["T"])
    _, d = R.nn1(R.transform_f(r["T"], sc["source"]), sc["target"])
    assert abs(score - d.astype(np.float64).mean()) <= 1e-12 * max(1.0, score)
    assert np.array_equal(g.transformSource(r["T"]), R.transform_f(r["T"], sc["source"]))


@pytest.mark.parametrize("search", [apd.SEARCH_BRUTE_FORCE, apd.SEARCH_PRUNED])
def test_lattice_tie_order(gorio, gpu, search):
    pts = S.lattice()
    sc = dict(source=pts, target=pts + np.float32(0.01), guess=np.eye(4, dtype=np.float32), params={})
    g = handle(gorio, gpu, sc, search)
    ref = S.make(sc)
    check_parts(g, ref, sc, degenerate_ok=True)


def test_cloud_smaller_than_k_is_refused(gorio, gpu):
    pts = S.room(19, 5)
    sc = dict(source=pts, target=S.room(64, 6), guess=np.eye(4, dtype=np.float32), params={})
    g = handle(gorio, gpu, sc)
    with pytest.raises(gorio.GorioError) as e:
        g.align()
    assert e.value.code == INVALID and "k_correspondences" in str(e.value)
    with pytest.raises(ValueError):
        S.make(sc).align()


def test_swap_then_align_equals_a_fresh_handle(gorio, gpu):
    sc = S.scenes()["general"]
    g = handle(gorio, gpu, sc)
    g.align(sc["guess"])
    g.swapSourceAndTarget()
    a = g.align()
    fresh = handle(gorio, gpu, dict(sc, source=sc["target"], target=sc["source"]))
    b = fresh.align()
    assert np.array_equal(a["T"], b["T"]) and (a["nr_iterations"], a["n_linearize"]) == (b["nr_iterations"], b["n_linearize"])
    g.clearSource()
    with pytest.raises(gorio.GorioError):
        g.align()


def test_keyframe_hand_off_equals_an_upload(gorio, gpu):
    sc = S.scenes()["general"]
    store = gorio.KeyframeStore(device=gpu)
    ks, kt = store.add(sc["source"]), store.add(sc["target"])
    g = handle(gorio, gpu, sc, upload=False)
    g.setInputTargetKeyframe(store, kt)
    g.setInputSourceKeyframe(store, ks)
    a = g.align(sc["guess"])
    b = handle(gorio, gpu, sc).align(sc["guess"])
    assert np.array_equal(a["T"], b["T"]) and (a["nr_iterations"], a["n_linearize"], a["converged"]) == (b["nr_iterations"], b["n_linearize"], b["converged"])
    # the keyframe's covariances now follow the GICP_OMP rule: a handle that estimates by another rule may not share them
    other = gorio.ApdGicp(device=gpu)
    with pytest.raises(gorio.GorioError) as e:
        other.setInputTargetKeyframe(store, kt)
    assert e.value.code == INVALID


def test_batch_and_linearisation_calls_are_refused(gorio, gpu):
    sc = S.scenes()["general"]
    g = handle(gorio, gpu, sc)
    before = g.align(sc["guess"])
    plain = gorio.ApdGicp(device=gpu)
    plain.setInputTarget(sc["target"])
    plain.setInputSource(sc["source"])
    for objs in ([g], [plain, g], [g, plain]):
        with pytest.raises(gorio.GorioError) as e:
            gorio.align_batch(objs)
        assert e.value.code == UNSUPPORTED
    assert g.get_method()["method"] == apd.METHOD_GICP_OMP and plain.get_method()["method"] == apd.METHOD_APDGICP
    for call in (lambda: g.linearize(np.eye(4)), lambda: g.compute_error(np.eye(4))):
        with pytest.raises(gorio.GorioError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    after = g.align(sc["guess"])
    assert np.array_equal(before["T"], after["T"]) and before["n_linearize"] == after["n_linearize"]
    assert plain.align()["converged"] in (True, False)  # the other handle still aligns by its own method


def test_shared_target_needs_the_same_rule(gorio, gpu):
    sc = S.scenes()["general"]
    g = handle(gorio, gpu, sc)
    g.calculateCovariances()
    other = gorio.ApdGicp(device=gpu)
    with pytest.raises(gorio.GorioError) as e:
        other.setInputTargetShared(g)
    assert e.value.code == INVALID
    twin = handle(gorio, gpu, sc, upload=False)
    twin.setInputTargetShared(g)
    twin.setInputSource(sc["source"])
    assert np.array_equal(twin.align(sc["guess"])["T"], g.align(sc["guess"])["T"])
    eps = handle(gorio, gpu, sc, upload=False)
    eps.setGicpOmpParams(1e-2, 20)
    with pytest.raises(gorio.GorioError) as e:
        eps.setInputTargetShared(g)
    assert e.value.code == INVALID
