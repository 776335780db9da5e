"""ICP (GORIO_METHOD_ICP, go-rio_amd/csrc/apd_icp.hip) on the GPU against the NumPy restatement (tests/icp_restatement.py) on the scenes of
tests/icp_scenes.py.  One pass (gorio_apd_icp_step): corr and sqd bit for bit, the 17 sums to 1e-9 relative (the H / b gate of the
project: the GPU adds block partials, NumPy adds in index order).  Full aligns: nr_iterations, state and pairs equal, the pose within
1e-4 m / 1e-4 rad (every scene's criteria are decided with a relative margin above 1e-6, tests/test_icp_restatement.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_restatement as R
import icp_scenes as S

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SEARCHES = [apd.SEARCH_BRUTE_FORCE, apd.SEARCH_PRUNED]
DBL_MAX = np.finfo(np.float64).max


def handle(gorio, gpu, params, search, source=None, target=None):
    """An ICP handle with the restatement's keyword arguments (defaults = pcl::IterativeClosestPoint's constructor values)."""
    g = gorio.ApdGicp(device=gpu, max_iterations=params.get("max_iterations", 10), transformation_epsilon=params.get("transformation_epsilon", 0.0),
                      corr_dist_threshold=params.get("max_correspondence_distance", np.sqrt(DBL_MAX)), search=search)
    g.set_method(apd.METHOD_ICP)
    g.set_icp_params(params.get("use_reciprocal", False), params.get("euclidean_fitness_epsilon", -DBL_MAX), params.get("transformation_rotation_epsilon", 0.0))
    if target is not None:
        g.setInputTarget(target)
    if source is not None:
        g.setInputSource(source)
    return g


def scene_handle(gorio, gpu, name, search):
    sc = S.scenes()[name]
    return handle(gorio, gpu, sc["params"], search, sc["source"], sc["target"])


def state_of(g, r):
    """Everything an align leaves behind that a caller can read."""
    corr, sqd = g.getCorrespondences()
    return dict(T=r["T"].copy(), converged=r["converged"], nr_iterations=r["nr_iterations"], n_linearize=r["n_linearize"], diag=g.icp_diag(), corr=corr, sqd=sqd)


def assert_same_bits(got, want, what):
    assert got["T"].tobytes() == want["T"].tobytes(), what
    assert (got["converged"], got["nr_iterations"], got["n_linearize"]) == (want["converged"], want["nr_iterations"], want["n_linearize"]), what
    assert got["diag"] == want["diag"], what
    assert np.array_equal(got["corr"], want["corr"]) and got["sqd"].tobytes() == want["sqd"].tobytes(), what


def check_align(name, got):
    want = S.reference(name)
    dt, dr = S.pose_error(want["T"], got["T"])
    print("%s: %d / %d iterations, state %d / %d, pairs %d / %d, mse %.6e / %.6e, pose error %.3e m %.3e rad" % (
        name, got["nr_iterations"], want["nr_iterations"], got["diag"]["state"], want["state"], got["diag"]["pairs"], want["pairs"], got["diag"]["mse"], want["mse"], dt, dr))
    assert got["converged"] == want["converged"]
    assert got["nr_iterations"] == got["diag"]["iterations"] == want["nr_iterations"]
    assert got["diag"]["state"] == want["state"] and got["diag"]["pairs"] == want["pairs"]
    assert got["n_linearize"] == want["passes"]
    assert dt <= 1e-4 and dr <= 1e-4
    if want["pairs"] >= 3:
        assert abs(got["diag"]["mse"] - want["mse"]) <= 1e-6 * want["mse"]


@pytest.mark.parametrize("search", SEARCHES)
def test_step_matches_the_restatement(gorio, gpu, search):
    for name, src, tgt, T, dist, recip in S.step_cases():
        g = handle(gorio, gpu, dict(max_correspondence_distance=dist, use_reciprocal=recip), search, src, tgt)
        got = g.icp_step(T)
        want = R.step(src, tgt, T, dist, recip)
        corr, sqd = g.getCorrespondences()
        assert np.array_equal(corr, want["corr"]), name
        assert sqd.tobytes() == want["sqd"].tobytes(), name
        assert got["pairs"] == want["pairs"] == int((corr >= 0).sum()), name
        assert got["sums"][0] == want["sums"][0] and got["sums"][1] >= 0.0
        scale = np.abs(want["sums"]).copy()
        scale[2:5], scale[5:8], scale[8:17] = scale[2:5].max(), scale[5:8].max(), scale[8:17].max()  # a vector / matrix is judged as a whole, like H and b
        err = np.abs(got["sums"] - want["sums"]) / np.maximum(scale, 1e-300)
        print("%s: %d pairs, sums off by %.2e relative" % (name, got["pairs"], err.max()))
        assert err.max() <= 1e-9, name
        if want["pairs"] >= 3:
            assert np.abs(got["T_est"].astype(np.float64) - want["T_est"].astype(np.float64)).max() <= 1e-6, name
        else:
            assert np.array_equal(got["T_est"], np.eye(4, dtype=np.float32))


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("name", [n for n in sorted(S.scenes()) if not n.startswith("batch_")])
def test_align_matches_the_restatement(gorio, gpu, name, search):
    sc = S.scenes()[name]
    g = scene_handle(gorio, gpu, name, search)
    r = g.align(sc["guess"])
    got = state_of(g, r)
    check_align(name, got)
    assert np.array_equal(r["H"], np.zeros((6, 6)))
    want = S.reference(name)
    assert int((got["corr"] >= 0).sum()) == want["pairs"]  # the pairs of the LAST pass
    # two runs give the same bits, on the same handle and on a fresh one
    assert_same_bits(state_of(g, g.align(sc["guess"])), got, name + " again")
    g2 = scene_handle(gorio, gpu, name, search)
    assert_same_bits(state_of(g2, g2.align(sc["guess"])), got, name + " fresh handle")


def test_search_modes_agree_bit_for_bit(gorio, gpu):
    for name in ("transform_255_recip", "relmse_513", "cap3_513_guess"):
        sc = S.scenes()[name]
        a, b = scene_handle(gorio, gpu, name, SEARCHES[0]), scene_handle(gorio, gpu, name, SEARCHES[1])
        assert_same_bits(state_of(a, a.align(sc["guess"])), state_of(b, b.align(sc["guess"])), name)


def test_two_pairs_end_unconverged_in_state_5(gorio, gpu):
    sc = S.scenes()["two_pairs"]
    g = scene_handle(gorio, gpu, "two_pairs", apd.SEARCH_BRUTE_FORCE)
    r = g.align(sc["guess"])
    assert not r["converged"] and r["nr_iterations"] == 0 and np.array_equal(r["T"], sc["guess"])
    assert g.icp_diag()["state"] == 5 and g.icp_diag()["pairs"] == 2 and int((g.getCorrespondences()[0] >= 0).sum()) == 2
    assert "fewer than 3 correspondences" in g._lib.gorio_apd_last_error(g._h).decode()


def test_three_points_align_where_the_other_methods_refuse(gorio, gpu):
    sc = S.scenes()["three_points"]
    g = scene_handle(gorio, gpu, "three_points", apd.SEARCH_PRUNED)
    assert g.align(sc["guess"])["converged"]
    for method in (apd.METHOD_APDGICP, apd.METHOD_GICP, apd.METHOD_GICP_OMP):
        o = gorio.ApdGicp(device=gpu)
        o.set_method(method)
        o.setInputTarget(sc["target"])
        o.setInputSource(sc["source"])
        with pytest.raises(gorio.GorioError) as e:
            o.align(sc["guess"])
        assert e.value.code == INVALID and "fewer points than k_correspondences" in str(e.value)


def test_the_other_calls_of_the_handle(gorio, gpu):
    name = "transform_256"
    sc = S.scenes()[name]
    g = scene_handle(gorio, gpu, name, apd.SEARCH_PRUNED)
    r = g.align(sc["guess"])
    before = state_of(g, r)
    lib, h = g._lib, g._h
    T = np.eye(4, dtype=np.float64)
    e = C.c_double(0)
    H, b = np.zeros(36), np.zeros(6)
    assert lib.gorio_apd_linearize(h, apd._p(T, C.c_double), apd._p(H, C.c_double), apd._p(b, C.c_double), C.byref(e)) == UNSUPPORTED
    assert lib.gorio_apd_compute_error(h, apd._p(T, C.c_double), C.byref(e)) == UNSUPPORTED
    with pytest.raises(gorio.GorioError) as ex:
        gorio.align_batch([g])
    assert ex.value.code == UNSUPPORTED
    m = np.zeros((sc["source"].shape[0], 16))
    assert lib.gorio_apd_get_mahalanobis(h, apd._p(m, C.c_double), sc["source"].shape[0]) == STATE
    assert lib.gorio_apd_debug_set_shard(h, 2, 0) == STATE
    assert lib.gorio_apd_comm_init(h, 2, 0, C.create_string_buffer(128)) == STATE
    x, f, cnt = (C.c_double * 6)(), C.c_double(0), C.c_int(0)
    Tf = np.eye(4, dtype=np.float32)
    assert lib.gorio_apd_gicp_omp_evaluate(h, x, 0, C.byref(f), None) == STATE
    assert lib.gorio_apd_gicp_omp_update(h, apd._p(Tf, C.c_float), apd._p(Tf, C.c_float), C.byref(cnt)) == STATE
    with pytest.raises(gorio.GorioError) as ex:
        gorio.gicp_omp_align_batch([g])
    assert ex.value.code == STATE
    # nothing changed
    after = state_of(g, dict(r))
    assert_same_bits(after, before, "after the refusals")
    # what keeps working: transform_source and the fitness score, equal to another method's handle on the same clouds
    o = gorio.ApdGicp(device=gpu, search=apd.SEARCH_PRUNED)
    o.setInputTarget(sc["target"])
    o.setInputSource(sc["source"])
    assert g.transformSource(r["T"]).tobytes() == o.transformSource(r["T"]).tobytes()
    assert g.getFitnessScore(r["T"], 1.0) == o.getFitnessScore(r["T"], 1.0)
    assert gorio.fitness_score_batch([g], r["T"][None], 1.0)[0][0] == g.getFitnessScore(r["T"], 1.0)[0]
    # a shared target and the device hand-off give the bits of an upload
    g2 = handle(gorio, gpu, sc["params"], apd.SEARCH_PRUNED, sc["source"])
    g2.setInputTargetShared(g)
    assert_same_bits(state_of(g2, g2.align(sc["guess"])), before, "shared target")
    # leaving the mode drops the pairs
    g.set_method(apd.METHOD_GICP)
    with pytest.raises(gorio.GorioError) as ex:
        g.getCorrespondences()
    assert ex.value.code == STATE
