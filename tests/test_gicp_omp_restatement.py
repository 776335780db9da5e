"""CPU tests of the GICP_OMP restatement (tests/gicp_omp_restatement.py): the objective's gradient, the BFGS of DESIGN.md against SciPy's,
known-transform recovery on the real pair, and the stability condition that admits a scene to the GPU pose gate."""
import numpy as np
import pytest

import gicp_omp_restatement as R
import gicp_omp_scenes as S

import scipy.optimize as scipy_optimize  # noqa: E402


@pytest.fixture(scope="module")
def frozen():
    """The pairs of the general scene's first outer iteration, frozen."""
    sc = S.scenes()["general"]
    g = S.make(sc)
    g.compute_covariances()
    out = R.transform_f(sc["guess"], g.src)
    corr, _, _, Mf = R.update(np.eye(4, dtype=np.float32), sc["guess"], out, g.tgt, g.C1, g.C2, g.corr_dist)
    return R.Functor(out, g.tgt, corr, Mf)


def test_gradient_against_central_differences(frozen):
    """df / fdf against central differences of the double-path f at h = 1e-3.  Bound: the residual is a float difference of coordinates up
    to 5 m, so it carries 2^-24 * 5 m = 3e-7 m of rounding per point; with Mahalanobis entries up to 1 / gicp_epsilon = 1e3 and residuals of
    0.05 m one term of f moves by 2 * 0.05 * 1e3 * 3e-7 = 3e-5, the mean over 600 pairs by 1e-6, and the difference quotient by
    1e-6 / 2h = 6e-4 per component; truncation adds h^2 |f'''| / 6, below that.  The gate is 1e-3 of the largest gradient component
    (36 here, so 3.6e-2): sixty such roundings, and still 30 times below a wrong sign or a missing factor 2 / m."""
    x = np.array([0.05, -0.02, 0.01, 0.01, -0.02, 0.03])
    f, g = frozen.fdf(x)
    assert np.array_equal(frozen.df(x), g)
    h = 1e-3
    fd = np.array([(frozen.fdf(x + h * e)[0] - frozen.fdf(x - h * e)[0]) / (2 * h) for e in np.eye(6)])
    err = np.abs(fd - g).max()
    print("gradient: max |fd - g| = %.3e, max |g| = %.3e" % (err, np.abs(g).max()))
    assert err <= 1e-3 * np.abs(g).max()
    assert abs(frozen.f(x) - f) <= 1e-5 * abs(f)  # float path against double path of the same sum


def test_frozen_pairs_bfgs_reaches_scipys_minimiser(frozen):
    """The restatement's BFGS (400 inner iterations, gradient tolerance 1e-8) and scipy.optimize.minimize(method="BFGS") on the same f
    (operator(), the float path) and g (df).  Both stop where the float rounding of f hides further descent -- SciPy reports "precision
    loss", the restatement NoProgress -- so they agree to that noise, not to 1e-8.  Measured state difference (max over the six
    components): 8.8e-5.  Gate: ten times that, 8.8e-4."""
    x, status, inner = R.minimize(frozen, np.zeros(6), 400, 1e-8)
    res = scipy_optimize.minimize(frozen.f, np.zeros(6), jac=frozen.df, method="BFGS", options=dict(gtol=1e-8, maxiter=400))
    diff = np.abs(res.x - x).max()
    print("frozen pairs: status %d after %d inner iterations, |x - x_scipy|_inf = %.3e, f = %.9e / %.9e" % (status, inner, diff, frozen.f(x), res.fun))
    assert status in (R.SUCCESS, R.NO_PROGRESS)
    assert diff <= 8.8e-4
    assert frozen.f(x) <= frozen.f(np.zeros(6)) * 0.5


def test_known_transform_recovery_on_the_real_pair():
    """a_0 -> a_1 moved by a known 0.3 m / 2 degree transform, within the reference's own acceptance of 0.05 m / 1 degree
    (fast_apdgicp/src/test/gicp_test.cpp:148-149)."""
    src, tgt, T = S.real_pair()
    g = R.GicpOmp()
    g.set_target(tgt)
    g.set_source(src)
    r = g.align()
    dt, dr = S.pose_error(T, r["T"])
    print("real pair: %.4f m, %.4f deg, %d outer / %d inner" % (dt, np.rad2deg(dr), r["nr_iterations"], r["inner_total"]))
    assert r["converged"] and 0 < r["nr_iterations"] < 200
    assert dt < 0.05 and dr < np.deg2rad(1.0)


@pytest.mark.parametrize("name", sorted(S.scenes()))
def test_scene_behaves_as_named(name):
    _, r = S.reference(name)
    sc = S.scenes()[name]
    if name in ("three_pairs", "no_pairs"):
        assert not r["converged"] and r["nr_iterations"] == 0 and r["evaluations"] == 0
        assert np.array_equal(r["T"], sc["guess"])  # previous_transformation_ (identity) * guess
    elif name == "outer_cap":
        assert r["converged"] and r["nr_iterations"] == 1
    elif name == "inner_cap":
        assert r["inner_total"] == r["nr_iterations"]  # one minimizeOneStep per outer iteration
    elif name == "identical":
        assert r["converged"] and r["nr_iterations"] == 1 and r["last_status"] == R.NO_PROGRESS and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
    else:
        assert r["converged"] and r["nr_iterations"] >= 1


def test_stability_condition_selects_the_pose_scenes():
    """Every reduction scaled by (1 +- 1e-9) must leave the outer and inner counts alone: only such scenes enter the GPU pose gate."""
    stable = [n for n in sorted(S.scenes()) if S.is_stable(n)]
    print("stable scenes:", stable)
    assert "general" in stable and len(stable) >= 5


def test_lattice_lists_prefer_the_lower_index():
    pts = S.lattice()
    lists = R.knn(pts, 20)
    d = R.sqdist(pts, pts)
    for i in (0, 62, 124):
        dl = d[i, lists[i]]
        assert (np.diff(dl) >= 0).all()
        same = np.diff(dl) == 0
        assert (np.diff(lists[i])[same] > 0).all()
