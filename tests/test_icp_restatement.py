"""The NumPy restatement of GORIO_METHOD_ICP (tests/icp_restatement.py) against what can be known without a GPU: recovery of a known
transform inside gicp_test.cpp's acceptance shape (0.05 m, 1 degree), Umeyama's reflection and rank-2 branches against closed forms, the
convergence states, and the admission rule of the scenes (every criterion decided with a relative margin above icp_scenes.MARGIN)."""
import numpy as np
import pytest

import icp_restatement as R
import icp_scenes as S

f32 = np.float32


def sums_of(q, t):
    q, t = np.asarray(q, f32), np.asarray(t, f32)
    return R.sums17(q, t, np.arange(q.shape[0], dtype=np.int32), np.zeros(q.shape[0], f32))


@pytest.mark.parametrize("name", ["defaults_257", "transform_256", "transform_255_recip", "relmse_513", "roteps_257"])
def test_known_transform_is_recovered(name):
    r = S.reference(name)
    dt, dr = S.pose_error(S.T_TRUE, r["T"])
    print("%s: %.3e m, %.3e rad after %d iterations" % (name, dt, dr, r["nr_iterations"]))
    assert r["converged"] and dt < 0.05 and dr < np.deg2rad(1.0)


def test_umeyama_general_reflection_and_rank2():
    rng = np.random.default_rng(0)
    q = rng.normal(size=(60, 3)) * [3.0, 2.0, 1.0]
    Tt = S.pose([0.3, -0.2, 0.1], [10, -20, 30]).astype(np.float64)
    # full rank: the transform itself
    T, branch = R.umeyama(sums_of(q, q @ Tt[:3, :3].T + Tt[:3, 3]))
    assert branch == "full" and np.abs(T - Tt).max() < 2e-6
    # a mirrored copy: det Sigma < 0.  With Sigma = M C (M = diag(1, 1, -1), C the covariance of q) the closed form is R = U diag(1, 1, -1) V^T
    # from the SVD of Sigma, a proper rotation; for the diagonal-dominant C here it stays near the identity, never the mirror
    s = sums_of(q, q * [1.0, 1.0, -1.0])
    T, branch = R.umeyama(s)
    n = s[0]
    sig = s[8:17].reshape(3, 3) / n - np.outer(s[5:8] / n, s[2:5] / n)
    U, _, Vt = np.linalg.svd(sig)
    assert branch == "reflection" and np.linalg.det(sig) < 0
    assert np.abs(T[:3, :3] - U @ np.diag([1.0, 1.0, -1.0]) @ Vt).max() < 1e-6 and abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) < 1e-5
    # an exactly diagonal case by construction: 8 corners of a box, mirrored in z -> Sigma = diag(a, b, -c), R = I exactly, t = 0
    box = np.array([[x, y, z] for x in (-3, 3) for y in (-2, 2) for z in (-1, 1)], np.float64)
    T, branch = R.umeyama(sums_of(box, box * [1.0, 1.0, -1.0]))
    assert branch == "reflection" and np.array_equal(T, np.eye(4, dtype=f32))
    # a planar cloud (rank 2) moved by a rigid transform: the transform itself, in the det(U) det(V) > 0 branch or the other, always proper
    qp = q.copy()
    qp[:, 2] = 0.0
    T, branch = R.umeyama(sums_of(qp, qp @ Tt[:3, :3].T + Tt[:3, 3]))
    assert branch.startswith("rank2") and np.abs(T - Tt).max() < 2e-6
    # the planar cloud mirrored inside its plane, then moved: the best PROPER rotation turns the plane over (R = Rt diag(1, -1, -1))
    T, branch = R.umeyama(sums_of(qp, (qp * [1.0, -1.0, 1.0]) @ Tt[:3, :3].T + Tt[:3, 3]))
    assert branch.startswith("rank2") and np.abs(T[:3, :3] - Tt[:3, :3] @ np.diag([1.0, -1.0, -1.0])).max() < 2e-6
    # three points are always rank 2
    q3 = rng.normal(size=(3, 3))
    T, branch = R.umeyama(sums_of(q3, q3 @ Tt[:3, :3].T + Tt[:3, 3]))
    assert branch.startswith("rank2") and np.abs(T - Tt).max() < 5e-6


def test_every_state_is_reached():
    got = {name: S.reference(name)["state"] for name in S.scenes()}
    print(got)
    assert got["defaults_257"] == R.STATE_ITERATIONS and S.reference("defaults_257")["nr_iterations"] == 10
    assert got["cap3_513_guess"] == R.STATE_ITERATIONS and S.reference("cap3_513_guess")["nr_iterations"] == 3
    assert got["transform_256"] == got["transform_255_recip"] == got["roteps_257"] == R.STATE_TRANSFORM
    assert got["relmse_513"] == got["relmse_4_recip"] == R.STATE_REL_MSE
    assert got["three_points"] == R.STATE_ABS_MSE
    r = S.reference("two_pairs")
    assert r["state"] == R.STATE_NO_CORRESPONDENCES and not r["converged"] and r["nr_iterations"] == 0 and r["pairs"] == 2
    assert np.array_equal(r["T"], np.eye(4, dtype=f32))
    for name in S.scenes():
        assert S.reference(name)["converged"] == (not name.endswith("two_pairs")), name
    # the members of the batch end at different iterations
    assert len({S.reference(n)["nr_iterations"] for n in S.batch()}) >= 4


@pytest.mark.parametrize("name", sorted(S.scenes()))
def test_scene_is_decided_with_margin(name):
    r = S.reference(name)
    print("%s: margin %.3e" % (name, r["margin"]))
    assert r["margin"] > S.MARGIN


def test_reciprocal_drops_pairs_and_gate_is_inclusive():
    for name, src, tgt, T, dist, recip in S.step_cases():
        if recip:
            a, b = R.step(src, tgt, T, dist, False), R.step(src, tgt, T, dist, True)
            assert b["pairs"] <= a["pairs"] and np.all((b["corr"] == a["corr"]) | (b["corr"] == -1))
            kept = b["corr"] >= 0
            assert len(set(b["corr"][kept])) == kept.sum()  # a target point keeps one source point at most
    # a pair exactly AT the threshold stays (PCL drops it only when the distance is greater)
    tgt = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], f32)
    src = tgt + np.array([0.5, 0, 0], f32)
    assert R.step(src, tgt, np.eye(4), 0.5)["pairs"] == 3 and R.step(src, tgt, np.eye(4), np.nextafter(0.5, 0))["pairs"] == 0
