"""NDT_OMP on the GPU (include/gorio_ndt.h) against tests/ndt_restatement.py, which tests/test_ndt_restatement.py pins on the CPU.

Gates: leaf indices, counts, min_b / div_b, means and pre-inflation covariances bit-exact; enabled / disabled flags equal; inverse
covariances 1e-9 relative to the largest entry of the leaf's matrix; score / gradient / Hessian 1e-9 relative to the largest entry
(the project's H / b gate); align poses 1e-4 m / 1e-4 rad against the restatement with equal counts; recovery 0.05 m / 1 degree."""
import numpy as np
import pytest

import ndt_restatement as R
import ndt_scenes as S
from conftest import rot_err
from map_checks import check_ndt_map as _check_map

pytestmark = pytest.mark.gpu
SEARCHES = [R.DIRECT1, R.DIRECT7, R.DIRECT26]
REL = 1e-9


@pytest.fixture(scope="module")
def real():
    return S.real_pair()


def test_voxel_map_real_pair(gorio, gpu, real):
    ref, _ = _check_map(gorio, gpu, real[1])
    assert (ref.count >= 6).sum() > 200


@pytest.mark.parametrize("name", ["negative", "offset_1e5", "nonfinite", "rules"])
def test_voxel_map_scenes(gorio, gpu, name):
    if name == "negative":
        ref, _ = _check_map(gorio, gpu, S.clusters(6000, 1))
        assert (ref.min_b < 0).all()
    elif name == "offset_1e5":
        ref, _ = _check_map(gorio, gpu, S.clusters(6000, 2, offset=1e5))
        assert (ref.min_b > 90000).all() and (ref.count >= 6).sum() > 50
    elif name == "nonfinite":
        _check_map(gorio, gpu, S.with_nonfinite(S.clusters(6000, 3), 4))
    else:
        pts, cells = S.rule_scene()
        ref, v = _check_map(gorio, gpu, pts)
        pos = {k: int(np.searchsorted(ref.idx, S.leaf_of(ref.min_b, ref.div_b, c))) for k, c in cells.items()}
        assert v["nr_points"][pos["five"]] == 5 and v["nr_points"][pos["six"]] == 6
        assert v["nr_points"][pos["same"]] == -1 and v["nr_points"][pos["line"]] == 8
        w = np.linalg.eigvalsh(v["cov"][pos["line"]])
        assert np.allclose(w[:2], 0.01 * w[2], rtol=1e-9)


@pytest.mark.parametrize("n", [63, 64, 65, 4095, 4096, 4097])
def test_voxel_map_sizes(gorio, gpu, n):
    _check_map(gorio, gpu, S.clusters(n, 10 + n, span=4.0 if n < 100 else 12.0))


def test_voxel_map_resolution_half(gorio, gpu, real):
    _check_map(gorio, gpu, real[1], resolution=0.5)  # REG:108


@pytest.fixture(scope="module")
def deriv_case(gorio, gpu, real):
    """The real pair: one handle, the restatement's map, the pose set."""
    src, tgt, _ = real
    vm = R.build_voxel_map(tgt, 1.0)
    lo, hi = vm.min_b.astype(float), (vm.max_b + 1).astype(float)
    n = gorio.Ndt(device=gpu)
    n.set_target(tgt)
    n.set_source(src)
    d1, d2, d3 = R.gauss_constants(1.0, 0.55)
    yield n, src, vm, S.poses(src, (lo, hi)), (d1, d2, d3)
    n.close()


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.abs(b).max()
    return np.array_equal(a, b) if scale == 0 else np.abs(a - b).max() <= REL * scale


@pytest.mark.parametrize("search", SEARCHES)
@pytest.mark.parametrize("pose", ["identity", "below_switch", "above_switch", "third_outside", "all_outside", "typical"])
def test_derivatives(deriv_case, search, pose):
    n, src, vm, poses, (d1, d2, _) = deriv_case
    p = poses[pose]
    n.set_params(search=search)
    score, g, H = n.derivatives(p)
    rs, rg, rH, pairs = R.derivatives(vm, src, p, search, d1, d2)
    if pose == "all_outside":
        assert pairs == 0 and score == 0 and not g.any() and not H.any()
    elif pose == "third_outside":
        cell = np.floor(R.transform_cloud(R.pose_matrix(p), src) / vm.leaf)  # inside the grid's box, occupied leaf or not
        inside = ((cell >= vm.min_b) & (cell <= vm.max_b)).all(axis=1).mean()
        assert 0.55 < inside < 0.75 and pairs > 0
    else:
        assert pairs > src.shape[0] // 4
    assert abs(score - rs) <= REL * abs(rs)
    assert _close(g, rg) and _close(H, rH)
    assert np.array_equal(H, H.T)
    # without the Hessian: the same score and gradient bits; twice: the same bits
    s2, g2, none = n.derivatives(p, compute_hessian=False)
    assert none is None and s2 == score and np.array_equal(g2, g)
    s3, g3, H3 = n.derivatives(p)
    assert s3 == score and np.array_equal(g3, g) and np.array_equal(H3, H)
    assert _close(n.hessian(p), R.hessian_only(vm, src, p, search, d1, d2))


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 300])
def test_derivatives_source_sizes(deriv_case, gorio, gpu, real, n_src):
    _, src, vm, poses, (d1, d2, d3) = deriv_case
    sub = src[np.linspace(0, src.shape[0] - 1, n_src).astype(int)] if n_src > 1 else vm.mean[np.argmax(vm.count)][None, :].astype(np.float32)
    n = gorio.Ndt(device=gpu, search=R.DIRECT7)
    n.set_target(real[1])
    n.set_source(sub)
    p = poses["typical"]
    score, g, H = n.derivatives(p)
    rs, rg, rH, pairs = R.derivatives(vm, sub, p, R.DIRECT7, d1, d2)
    assert pairs > 0 and abs(score - rs) <= REL * abs(rs) and _close(g, rg) and _close(H, rH)
    T = R.pose_matrix(p)
    assert abs(n.calculate_score(T) - R.calculate_score(vm, sub, T, R.DIRECT7, d1, d2, d3)) <= REL * abs(R.calculate_score(vm, sub, T, R.DIRECT7, d1, d2, d3))
    n.close()


@pytest.mark.parametrize("search", SEARCHES)
def test_calculate_score(deriv_case, search):
    n, src, vm, poses, (d1, d2, d3) = deriv_case
    n.set_params(search=search)
    for name in ("identity", "typical", "third_outside", "all_outside"):
        T = R.pose_matrix(poses[name])
        ref = R.calculate_score(vm, src, T, search, d1, d2, d3)
        assert abs(n.calculate_score(T) - ref) <= REL * abs(ref), name


def _align_both(gorio, gpu, src, tgt, guess=None, **params):
    n = gorio.Ndt(device=gpu, **params)
    n.set_target(tgt)
    n.set_source(src)
    r = n.align(guess)
    n.close()
    ref = R.Ndt(**{("min_points" if k == "min_points_per_voxel" else k): v for k, v in params.items()})
    ref.set_target(tgt)
    ref.set_source(src)
    q = ref.align(guess)
    dt, dr = rot_err(q["T"], r["T"])
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    for k in ("converged", "nr_iterations", "n_derivatives", "n_hessians", "n_mt"):
        assert r[k] == q[k], (k, r[k], q[k])
    assert abs(r["trans_probability"] - q["trans_probability"]) <= 1e-6 * abs(q["trans_probability"]) + 1e-12
    return r, q


@pytest.mark.parametrize("search", [R.DIRECT1, R.DIRECT7])
def test_align_real_pair(gorio, gpu, real, search):
    src, tgt, T = real
    r, _ = _align_both(gorio, gpu, src, tgt, search=search, transformation_epsilon=0.01, max_iterations=64)
    dt, dr = rot_err(T, r["T"])
    assert r["converged"] and dt < 0.05 and dr < np.deg2rad(1.0)


@pytest.mark.parametrize("search", [R.DIRECT1, R.DIRECT7])
def test_align_synthetic_radar_pair(gorio, gpu, search):
    src, tgt, T = S.radar_pair()
    r, _ = _align_both(gorio, gpu, src, tgt, search=search, transformation_epsilon=0.01, max_iterations=64)
    dt, dr = rot_err(T, r["T"])
    assert r["converged"] and dt < 0.05 and dr < np.deg2rad(1.0), (dt, np.rad2deg(dr))


def test_align_guess_without_neighbours_returns_the_guess(gorio, gpu, real):
    src, tgt, _ = real
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = [5000.0, 0.0, 0.0]
    r, _ = _align_both(gorio, gpu, src, tgt, guess=G)
    assert r["converged"] and r["nr_iterations"] == 0 and r["n_derivatives"] == 1 and np.array_equal(r["T"], G)


def test_align_with_a_guess_and_one_iteration(gorio, gpu, real):
    src, tgt, T = real
    G = np.eye(4)
    G[:3, 3] = [0.1, -0.1, 0.0]
    r, _ = _align_both(gorio, gpu, src, tgt, guess=G.astype(np.float32), max_iterations=1, transformation_epsilon=1e-6)
    assert r["converged"] and r["nr_iterations"] == 3  # NDT:158: nr_iterations_ > max_iterations_ is tested before the increment


def test_handle_reuse_bigger_smaller_empty(gorio, gpu, real):
    src, tgt, _ = real
    n = gorio.Ndt(device=gpu)
    n.set_source(src)
    caps = None
    for cloud in (S.clusters(9000, 7), tgt, S.clusters(700, 8)):
        n.set_target(cloud)
        ref = R.build_voxel_map(cloud, 1.0)
        v = n.voxels()
        assert np.array_equal(v["leaf_index"], ref.idx) and np.array_equal(v["mean"], ref.mean)
        if caps is None:
            caps = n.capacities()  # after the biggest cloud
            assert caps["target"] >= 9000 and caps["leaves"] >= ref.n_leaves and caps["keys"] >= 9000
        assert n.capacities() == caps  # buffers are kept: a smaller cloud reallocates nothing
    n.set_target(np.zeros((0, 3), np.float32))
    assert n.voxels()["leaf_index"].size == 0 and n.capacities() == caps
    with pytest.raises(gorio.GorioError) as e:
        n.align()
    assert e.value.code == -3  # GORIO_ERR_STATE
    n.set_target(tgt)  # and the handle still works
    assert n.align()["converged"]
    n.close()


def test_state_and_argument_errors(gorio, gpu, real):
    src, tgt, _ = real
    n = gorio.Ndt(device=gpu)
    n.set_source(src)
    with pytest.raises(gorio.GorioError) as e:
        n.align()  # before set_target
    assert e.value.code == -3
    n.set_target(tgt)
    bad = src.copy()
    bad[5, 1] = np.nan
    with pytest.raises(gorio.GorioError) as e:
        n.set_source(bad)
    assert e.value.code == -1
    assert n.align()["converged"]  # the source held stayed
    for kw in ({"search": R.KDTREE}, {"resolution": 0.0}, {"resolution": -1.0}):
        with pytest.raises(gorio.GorioError) as e:
            n.set_params(**kw)
        assert e.value.code == -5
    n.close()


def test_device_inputs_equal_host_inputs(gorio, gpu, real):
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")  # the runtime the library itself is linked against (torch ships its own copy)
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a, np.float32)
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(ptr, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        bufs.append(ptr)
        return ptr.value

    src, tgt, _ = real
    a = gorio.Ndt(device=gpu)
    a.set_target(tgt)
    a.set_source(src)
    b = gorio.Ndt(device=gpu)
    b.set_target_device(*[dev(tgt[:, k]) for k in range(3)], tgt.shape[0])
    b.set_source_device(*[dev(src[:, k]) for k in range(3)], src.shape[0])
    ra, rb = a.align(), b.align()
    assert np.array_equal(ra["T"], rb["T"]) and ra["nr_iterations"] == rb["nr_iterations"]
    bad = src.copy()
    bad[3, 1] = np.inf
    with pytest.raises(gorio.GorioError) as e:
        b.set_source_device(*[dev(bad[:, k]) for k in range(3)], src.shape[0])
    assert e.value.code == -1
    assert np.array_equal(b.align()["T"], ra["T"])  # the source held stayed
    a.close()
    b.close()
    for ptr in bufs:
        hip.hipFree(ptr)
