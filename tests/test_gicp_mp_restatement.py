"""The restatement of fast_gicp::FastGICPMultiPoints (tests/gicp_mp_restatement.py) on the CPU: it recovers the scenes' true pose, every scene is
admitted (no floating-point criterion decided by a hair), empty neighbourhoods are skipped, and the rounding spreads the GPU tests take their
tolerances from are the ones recorded there."""
import numpy as np
import pytest

import gicp_mp_restatement as R
import gicp_mp_scenes as M
import icp_scenes as S
import search_restatement as sr


@pytest.mark.parametrize("name", M.ALIGN_SCENES)
def test_recovers_the_true_pose(name):
    r = M.reference(name)
    dt, dr = S.pose_error(r["T"], S.T_TRUE)
    assert r["converged"] and 2 <= r["passes"] <= 6 and r["iterations"] == r["passes"] - 1
    assert dt < 0.05 and dr < np.deg2rad(1.0)  # the acceptance of the reference's gicp_test.cpp:148-149


@pytest.mark.parametrize("name", list(M.scenes()))
def test_scene_is_admitted(name):
    r = M.reference(name)
    for q in r["ratios"]:
        assert q < 0.5 or q > 2.0, r["ratios"]  # float noise cannot flip the pass count
    assert r["clamp_margin"] > 1e-6  # no weight sits on the clamp switch


def test_far_points_are_skipped_and_the_rest_align():
    sc = M.scenes()["far_points_257"]
    cs, ct = R.covariances(sc["source"]), R.covariances(sc["target"])
    P = R.one_pass(sc["source"], cs, sc["target"], ct, sc["guess"])
    lens = np.diff(P.offsets)
    assert (lens[100:120] == 0).all() and (lens[:100] > 0).all() and (lens[120:] > 0).all() and P.n_used == 257
    assert (P.mean_B[100:120] == 0).all()
    a, b = M.reference("far_points_257"), M.reference("id_257_2000")
    assert a["converged"] and a["iterations"] == b["iterations"]
    assert S.pose_error(a["T"], b["T"])[0] < 1e-6  # the far points add nothing but a different summation tree


def test_all_empty_ends_unconverged_at_the_guess():
    r = M.reference("all_empty")
    assert not r["converged"] and r["iterations"] == 0 and r["passes"] == 1 and r["used"] == [0]
    dt, dr = S.pose_error(r["T"], M.scenes()["all_empty"]["guess"])
    assert np.array_equal(r["T"][:3, 3], M.scenes()["all_empty"]["guess"][:3, 3]) and dt < 1e-6 and dr < 1e-6


def test_exp_log_round_trip_and_small_angle_branch():
    for w in ([0.3, -0.2, 0.1], [1e-7, 2e-7, -1e-7], [0.0, 0.0, 0.0], [1e-4, 0.0, 2e-4]):
        Rm = R.so3_exp(w)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-14) and np.allclose(R.so3_log(Rm), w, rtol=1e-9, atol=1e-16)


def test_ldlt_solves_and_block_sums_add_up():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(9, 6))
    H, g = A.T @ A, rng.normal(size=6)
    assert np.allclose(R.ldlt6_solve(H, g), np.linalg.solve(H, g), rtol=1e-10)
    v = rng.normal(size=(600, 28))
    assert np.allclose(R.block_sums(v), v.sum(axis=0), rtol=1e-12, atol=1e-12)


def test_covariance_rules():
    cloud = M.cov_clouds()["room_257"]
    raw = R.raw_covariances(cloud, 20)
    lists = sr.knn(cloud, None, 20)[0]
    p = cloud[lists[5]].astype(np.float64)
    d = p - p.mean(axis=0)
    assert np.allclose(R.full3(raw[5:6])[0], d.T @ d, rtol=1e-4, atol=1e-6)  # not divided by k
    w = np.linalg.eigvalsh(R.full3(R.regularize(raw, R.PLANE).astype(np.float64)))
    assert np.allclose(w, [1e-3, 1.0, 1.0], rtol=0, atol=5e-7)  # the entries are float32: an eigenvalue moves by a few 6e-8
    c = R.full3(raw.astype(np.float64)) + 1e-3 * np.eye(3)
    fro = R.full3(R.regularize(raw, R.FROBENIUS).astype(np.float64))
    assert np.allclose(fro, c * np.linalg.norm(np.linalg.inv(c), axis=(1, 2))[:, None, None], rtol=1e-5)
    with pytest.raises(ValueError):
        R.regularize(raw, R.NONE)


def test_recorded_spreads_are_the_measured_ones():
    import test_gicp_mp_gpu as G

    m = M.measured_spreads()
    for q, recorded in G.SPREAD.items():
        assert m[q] <= recorded <= 2.0 * m[q], (q, m[q], recorded)
