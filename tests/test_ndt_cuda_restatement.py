"""CPU checks of tests/ndt_cuda_restatement.py, the NumPy definition of GORIO_METHOD_NDT_CUDA: offset tables, the float coordinate rule,
the regularisation, the gradient structure of b, and the acceptance shape of the reference's gicp_test.cpp:148-149."""
import numpy as np
import pytest

import ndt_cuda_restatement as nr
from conftest import rot_err

F = np.float32


def test_offset_tables():
    assert [len(nr.offsets(s)) for s in (nr.DIRECT1, nr.DIRECT7, nr.DIRECT27)] == [1, 7, 27]
    assert [len(nr.offsets(nr.DIRECT_RADIUS, r)) for r in (1.0, 1.5, 2.0)] == [7, 19, 33]
    assert nr.offsets(nr.DIRECT7).tolist() == [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    o27 = nr.offsets(nr.DIRECT27)
    assert o27[0].tolist() == [-1, -1, -1] and o27[1].tolist() == [-1, -1, 0] and o27[13].tolist() == [0, 0, 0] and o27[26].tolist() == [1, 1, 1]
    o1 = nr.offsets(nr.DIRECT_RADIUS, 1.0)  # the triple loop's order, not DIRECT7's
    assert o1.tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0]]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            nr.offsets(nr.DIRECT_RADIUS, bad)
    with pytest.raises(NotImplementedError):
        nr.offsets(nr.DIRECT_RADIUS, 3.5)
    assert len(nr.offsets(nr.DIRECT_RADIUS, 3.0)) == 123


@pytest.mark.parametrize("res", [1.0, 0.5, 2.0])
def test_float_coordinate_rule(res):
    x = np.array([0.5 * res, 1.5 * res, -0.5 * res, -1.5 * res, 0.0, np.nextafter(F(0.5 * res), F(0)), -0.25 * res, 0.49 * res, 1.49 * res], F)
    assert nr.voxel_coord(x, res).tolist() == [0, 1, -1, -2, -1, -1, -1, -1, 0]


def test_float_and_double_rules_differ_somewhere():
    x = np.array([nr.FLOAT_RULE_POINT], F)
    assert float(x[0]) == nr.FLOAT_RULE_POINT  # exactly representable
    assert nr.voxel_coord(x, nr.FLOAT_RULE_RESOLUTION)[0] == 6 and nr.voxel_coord_double(x, nr.FLOAT_RULE_RESOLUTION)[0] == 7


def test_one_point_voxel_regularises_to_min_eig():
    m = nr.build_map(np.array([[3.2, -1.7, 0.4]], F), 1.0)
    assert m["num_points"].tolist() == [1] and np.array_equal(m["mean"][0], np.array([3.2, -1.7, 0.4], F))
    assert np.array_equal(m["cov_raw"][0], np.zeros((3, 3), F))
    assert np.array_equal(m["cov"][0], (1e-3 * np.eye(3)).astype(F))


def test_map_order_counts_and_moments():
    rng = np.random.default_rng(3)
    pts = rng.uniform(-3, 3, (500, 3)).astype(F)
    m = nr.build_map(pts, 1.0)
    assert m["num_points"].sum() == 500 and np.all(np.diff(m["key"]) > 0)
    c = nr.voxel_coord(pts, 1.0)
    for v in (0, len(m["key"]) // 2, len(m["key"]) - 1):
        sel = np.all(c == m["coord"][v], axis=1)
        assert sel.sum() == m["num_points"][v]
        p = pts[sel].astype(np.float64)
        assert np.allclose(m["mean"][v], p.mean(axis=0), atol=1e-5)
        assert np.allclose(m["cov_raw"][v], np.cov(p.T, bias=True).reshape(3, 3), atol=2e-5)
        w = np.linalg.eigvalsh(m["cov"][v].astype(np.float64))
        assert w.min() >= 1e-3 * (1 - 1e-5)


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_b_is_the_gradient_structure(mode):
    """With w and C frozen, b = w J^T C e and d(e^T C e)/dt_k = -2 (C e)_k along translation axis k (J's translation block is -I):
    so b[3 + k] = w/2 times the derivative.  A central difference with step h has truncation error 0 for a quadratic; what is left is float32
    rounding of the terms, about 4 eps |e^T C e| / h per axis, summed with the float32 rounding of b itself: 1e-3 relative for h = 1e-2."""
    src, tgt, _ = nr.scene_pair(1024)
    r = nr.NdtCuda(distance_mode=mode)
    r.setInputSource(src)
    r.setInputTarget(tgt)
    r.linearize(np.eye(4))
    items, icov = r._items()
    keep = np.flatnonzero(r.target_map["num_points"][r.pairs[:, 1]] > 6)
    assert keep.size >= 5
    h = 1e-2
    for pi in keep[:5]:
        pair = r.pairs[pi : pi + 1]
        a = items[pair[0, 0]].astype(np.float64)
        mb = r.target_map["mean"][pair[0, 1]].astype(np.float64)
        Q = r.target_map["cov"][pair[0, 1]].astype(np.float64)
        if mode == nr.D2D:
            Q = Q + icov[pair[0, 0]].astype(np.float64)
        C = np.linalg.inv(Q)
        e0 = mb - a
        w = 1.0 / (1.0 + e0 @ e0)  # k = res = 1
        _, b, _ = nr.pair_terms(pair, items, icov, r.target_map, np.eye(4), np.eye(4), mode == nr.D2D)
        for k in range(3):
            tp, tm = np.zeros(3), np.zeros(3)
            tp[k], tm[k] = h, -h
            fd = (((e0 - tp) @ C @ (e0 - tp)) - ((e0 - tm) @ C @ (e0 - tm))) / (2 * h)
            assert b[0, 3 + k] == pytest.approx(0.5 * w * fd, rel=1e-3, abs=1e-3 * np.abs(C @ e0).max() * w)


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
@pytest.mark.parametrize("case", ["forward", "backward", "swap"])
def test_known_transform_is_recovered(mode, case):
    """gicp_test.cpp:148-149: within 0.05 m and 1 degree, forward, backward and after swapSourceAndTarget.  Scene: SCENE_SEED, 4096 points,
    resolution 1.0, DIRECT7 (chosen by running this restatement: 8 m room, 2 cm noise)."""
    src, tgt, T = nr.scene_pair(4096)
    r = nr.NdtCuda(distance_mode=mode)
    if case == "backward":
        r.setInputSource(tgt)
        r.setInputTarget(src)
    else:
        r.setInputSource(src)
        r.setInputTarget(tgt)
    want = T if case == "forward" else np.linalg.inv(T)
    if case == "swap":
        builds = (r.align(), r.map_builds)[1]
        r.swapSourceAndTarget()
        out = r.align()
        assert r.map_builds == (builds + 1 if mode == nr.P2D else builds)  # the maps change sides with the clouds; P2D had no source map
    else:
        out = r.align()
    te, re_ = rot_err(want, out["T"])
    assert out["converged"] and te < 0.05 and np.degrees(re_) < 1.0, (te, np.degrees(re_))


def test_disjoint_clouds_leave_the_guess():
    src, tgt, _ = nr.scene_pair(512)
    r = nr.NdtCuda(distance_mode=nr.P2D)
    r.setInputSource(src + F(500.0))
    r.setInputTarget(tgt)
    out = r.align()
    assert len(r.pairs) == 0 and out["converged"] and out["n_linearize"] == 1 and np.array_equal(out["T"], np.eye(4, dtype=F))
