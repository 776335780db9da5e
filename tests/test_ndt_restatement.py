"""Pins tests/ndt_restatement.py (the NumPy restatement of pclomp NDT_OMP that the GPU tests compare against) on the CPU: derivatives
against finite differences of its own score, the score against calculateScore's definition, the leaf rules of the voxel map, and
known-transform recovery on the real LiDAR pair in the acceptance shape of gicp_test.cpp:148-201 (0.05 m / 1 degree).  No GPU."""
import numpy as np
import pytest

import ndt_restatement as R
import ndt_scenes as S
from conftest import rot_err

T_TOL, R_TOL = 0.05, np.deg2rad(1.0)  # gicp_test.cpp:149-150


@pytest.fixture(scope="module")
def smooth():
    src, tgt = S.smooth_scene()
    vm = R.build_voxel_map(tgt, 1.0)
    d1, d2, d3 = R.gauss_constants(1.0, 0.55)
    return src, vm, d1, d2, d3


P0 = np.array([0.03, -0.02, 0.025, 0.02, -0.025, 0.03])  # every angle far above the 10e-5 switch, no source point changes its cell


def test_smooth_scene_keeps_every_point_in_its_cell(smooth):
    src, vm, *_ = smooth
    base = R.neighbourhood(vm, R.transform_cloud(R.pose_matrix(np.zeros(6)), src), R.DIRECT1)[0]
    assert (base >= 0).all() and (vm.count >= 6).sum() == 8
    for k in range(6):
        for s in (-1, 1):
            p = P0.copy()
            p[k] += s * 2e-3
            assert (R.neighbourhood(vm, R.transform_cloud(R.pose_matrix(p), src), R.DIRECT1)[0] == base).all()


def test_gradient_and_hessian_against_finite_differences(smooth):
    src, vm, d1, d2, _ = smooth
    h = 1e-3
    score, g, H, pairs = R.derivatives(vm, src, P0, R.DIRECT1, d1, d2)
    assert pairs == src.shape[0]
    g_fd, H_fd = np.zeros(6), np.zeros((6, 6))
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        sp, gp, _, _ = R.derivatives(vm, src, P0 + e, R.DIRECT1, d1, d2, compute_hessian=False)
        sm, gm, _, _ = R.derivatives(vm, src, P0 - e, R.DIRECT1, d1, d2, compute_hessian=False)
        g_fd[k] = (sp - sm) / (2 * h)
        H_fd[:, k] = (gp - gm) / (2 * h)
    assert np.abs(g - g_fd).max() < 1e-3 * np.abs(g).max()
    # computeHessian (double tables) is the derivative of the gradient in every entry
    Hd = R.hessian_only(vm, src, P0, R.DIRECT1, d1, d2)
    assert np.abs(Hd - H_fd).max() < 1e-3 * np.abs(Hd).max()
    # computeDerivatives' float Hessian too, but for (pitch, pitch): its float table row d1 holds +sy (NDT:383) against -sy (NDT:361)
    mask = np.ones((6, 6), bool)
    mask[4, 4] = False
    assert np.abs(H - H_fd)[mask].max() < 1e-3 * np.abs(H).max()
    assert np.abs(H - Hd)[mask].max() < 1e-4 * np.abs(H).max()
    assert np.array_equal(H, H.T)


def test_score_is_calculate_score_on_one_neighbour(smooth):
    """DIRECT1, every point with its one leaf: calculateScore = (sum(-d1 e) - N d3) / N, computeDerivatives' score = sum(-d1 e)."""
    src, vm, d1, d2, d3 = smooth
    n = src.shape[0]
    score, _, _, pairs = R.derivatives(vm, src, P0, R.DIRECT1, d1, d2, compute_hessian=False)
    cs = R.calculate_score(vm, src, R.pose_matrix(P0), R.DIRECT1, d1, d2, d3)
    assert pairs == n
    assert abs((cs * n + d3 * n) - score) < 1e-5 * abs(score)  # the derivative path rounds each term to float


def test_leaf_rules():
    pts, cells = S.rule_scene()
    vm = R.build_voxel_map(pts, 1.0)
    pos = {k: int(np.searchsorted(vm.idx, S.leaf_of(vm.min_b, vm.div_b, c))) for k, c in cells.items()}
    assert vm.n_leaves == 6 and all(vm.idx[p] == S.leaf_of(vm.min_b, vm.div_b, cells[k]) for k, p in pos.items())
    assert vm.count[pos["five"]] == 5 and vm.count[pos["six"]] == 6
    centre = lambda c: (np.array(c, np.float32) + np.float32(0.5))[None, :]
    nb = lambda k: R.neighbourhood(vm, centre(cells[k]), R.DIRECT1)[0][0]
    assert nb("five") == -1 and nb("six") == pos["six"]  # VGC:297, 395: 5 points never a neighbour, 6 are
    # collinear along x: the two zero eigenvalues are lifted to 0.01 x the largest (VGC:345-356)
    w = np.linalg.eigvalsh(vm.cov[pos["line"]])
    wr = np.linalg.eigvalsh(vm.cov_raw[pos["line"]])
    assert wr[0] == 0 and wr[1] == 0 and wr[2] > 0
    assert np.allclose(w[:2], 0.01 * wr[2], rtol=1e-12) and np.isclose(w[2], wr[2], rtol=1e-12)
    assert vm.count[pos["line"]] == 8 and nb("line") == pos["line"]
    # six coincident points: largest eigenvalue 0 -> disabled (VGC:337-341)
    assert vm.count[pos["same"]] == -1 and nb("same") == -1
    assert np.all(vm.cov_raw[pos["same"]] == 0)
    # a generic leaf: mean and the single-pass covariance against the two-pass definition
    for k in ("generic", "negative"):
        member = np.all(np.floor(pts) == np.array(cells[k]), axis=1)
        q = pts[member].astype(np.float64)
        assert np.allclose(vm.mean[pos[k]], q.mean(axis=0), rtol=0, atol=1e-12)
        assert np.allclose(vm.cov_raw[pos[k]], np.cov(q.T, bias=True) * (len(q) - 1.0) / len(q), rtol=0, atol=1e-12)
        assert np.allclose(vm.icov[pos[k]] @ vm.cov[pos[k]], np.eye(3), atol=1e-9)


def test_nonfinite_target_points_are_skipped():
    pts = S.clusters(500, 2)
    a = R.build_voxel_map(S.with_nonfinite(pts, 1), 1.0)
    keep = np.ones(500, bool)
    keep[np.arange(3, 500, 7)] = False
    b = R.build_voxel_map(pts[keep], 1.0)
    assert np.array_equal(a.idx, b.idx) and np.array_equal(a.count, b.count) and np.array_equal(a.mean, b.mean)


def test_neighbourhood_orders_and_bounds():
    assert R.offsets(R.DIRECT26).shape == (26, 3) and not (R.offsets(R.DIRECT26) == 0).all(axis=1).any()
    assert len({tuple(o) for o in R.offsets(R.DIRECT26)}) == 26
    vm = R.build_voxel_map(S.clusters(2000, 3), 1.0)
    far = np.array([[1e6, 0, 0], [3e38, 0, 0], [-1e6, -1e6, -1e6]], np.float32)
    for s in (R.DIRECT1, R.DIRECT7, R.DIRECT26):
        assert all((pos == -1).all() for pos in R.neighbourhood(vm, far, s))
    with pytest.raises(R.Unsupported):
        R.offsets(R.KDTREE)
    with pytest.raises(R.Unsupported):
        R.build_voxel_map(S.clusters(100, 1), 0.0)


def test_pose_matrix_and_euler_round_trip():
    for p in (np.zeros(6), np.array([1.0, -2.0, 0.5, 0.3, -0.2, 1.1]), np.array([0, 0, 0, -0.4, 0.1, -2.5])):
        T = R.pose_matrix(p)
        assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-6)
        a = R.euler_angles_012(T[:3, :3])
        T2 = R.pose_matrix(np.concatenate([p[:3], a.astype(np.float64)]))
        assert np.allclose(T, T2, atol=1e-6)  # the angles may differ by the (pi - a, pi - b, pi + c) branch, the rotation may not


def test_svd_solve():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(6, 6))
    H = A + A.T  # indefinite
    b = rng.normal(size=6)
    assert np.allclose(R.svd_solve(H, b), np.linalg.solve(H, b), rtol=1e-9)
    assert np.array_equal(R.svd_solve(np.zeros((6, 6)), b), np.zeros(6))
    v = rng.normal(size=6)
    x = R.svd_solve(np.outer(v, v), v)  # rank one: the minimum-norm solution
    assert np.allclose(x, v / (v @ v), rtol=1e-9)


@pytest.fixture(scope="module")
def real():
    return S.real_pair()


@pytest.mark.parametrize("search", [R.DIRECT7, R.DIRECT1])
def test_known_transform_recovery_on_the_real_pair(real, search):
    """a_0 -> a_1 moved by a known 0.3 m / 2 degree transform, resolution 1.0 (it converges on the thinned clouds)."""
    src, tgt, T = real
    ndt = R.Ndt(resolution=1.0, search=search, transformation_epsilon=0.01, max_iterations=64)
    ndt.set_target(tgt)
    ndt.set_source(src)
    r = ndt.align()
    dt, dr = rot_err(T, r["T"])
    assert r["converged"] and 0 < r["nr_iterations"] <= 64
    assert dt < T_TOL and dr < R_TOL, (dt, np.rad2deg(dr))
    assert r["n_derivatives"] == 1 + r["nr_iterations"] + r["n_mt"]  # NDT:119, 837, 881


def test_no_neighbour_returns_the_guess_at_once(real):
    src, tgt, _ = real
    ndt = R.Ndt(search=R.DIRECT7)
    ndt.set_target(tgt)
    ndt.set_source(src)
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = [5000.0, 0.0, 0.0]
    r = ndt.align(G)
    assert r["converged"] and r["nr_iterations"] == 0 and r["n_derivatives"] == 1 and np.array_equal(r["T"], G)
