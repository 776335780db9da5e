"""The radius neighbourhood of NDT on the GPU (gorio_ndt_set_radius_search, include/gorio_ndt.h) against tests/ndt_radius_restatement.py,
which tests/test_ndt_radius_restatement.py pins on the CPU.

Gates: centroid cloud, centroid -> leaf table and neighbour CSR bit-exact (array_equal); score / gradient / Hessian with the REL rule
of tests/test_ndt_gpu.py (1e-9 relative to the largest entry); align poses 1e-4 m / 1e-4 rad against the restatement with equal counts
and trans_probability to 1e-6 relative; everything the contract calls "the same" compared with == / array_equal."""
import numpy as np
import pytest

import ndt_radius_restatement as RR
import ndt_restatement as R
import ndt_scenes as S
from conftest import rot_err

pytestmark = pytest.mark.gpu
REL = 1e-9
POSES = ["identity", "typical", "third_outside", "all_outside"]
FIELDS = ("converged", "nr_iterations", "trans_probability", "n_derivatives", "n_hessians", "n_mt", "score")


@pytest.fixture(scope="module")
def real():
    return S.real_pair()


def _sparse_target():
    """40 points scattered over 60 m: leaves exist, none has min_points_per_voxel points, so the centroid cloud is empty."""
    return np.random.default_rng(21).uniform(-30.0, 30.0, (40, 3)).astype(np.float32)


def _close(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    scale = np.abs(b).max()
    return np.array_equal(a, b) if scale == 0 else np.abs(a - b).max() <= REL * scale


def _check_centroids(gorio, gpu, target, resolution=1.0):
    ref = RR.build_voxel_map(target, resolution)
    n = gorio.Ndt(device=gpu, resolution=resolution)
    n.set_target(target)
    xyz, pos = n.centroids()
    assert not n.get_radius_search()  # the hook builds the cloud with the switch off
    n.close()
    assert xyz.dtype == np.float32 and np.array_equal(xyz, ref.cent) and np.array_equal(pos, ref.cent_leaf)
    return ref


@pytest.mark.parametrize("name", ["real_1.0", "real_0.5", "rules", "no_eligible_leaf"])
def test_centroid_cloud(gorio, gpu, real, name):
    if name == "real_1.0":
        ref = _check_centroids(gorio, gpu, real[1])
        assert (ref.cent != ref.mean[ref.cent_leaf].astype(np.float32)).any()  # float sums, not rounded double means
    elif name == "real_0.5":
        _check_centroids(gorio, gpu, real[1], 0.5)
    elif name == "rules":
        pts, _ = S.rule_scene()
        ref = _check_centroids(gorio, gpu, pts)
        assert (ref.count[ref.cent_leaf] == -1).sum() == 1  # the disabled leaf is in the cloud
    else:
        ref = _check_centroids(gorio, gpu, _sparse_target())
        assert ref.n_leaves > 0 and ref.cent.shape[0] == 0


@pytest.fixture(scope="module")
def case(gorio, gpu, real):
    """The real pair at resolution 1.0: one radius handle, the restatement's map, the pose set, the Gaussian constants."""
    src, tgt, _ = real
    vm = RR.build_voxel_map(tgt, 1.0)
    lo, hi = vm.min_b.astype(float), (vm.max_b + 1).astype(float)
    n = gorio.Ndt(device=gpu, radius_search=True)
    n.set_target(tgt)
    n.set_source(src)
    yield n, src, vm, S.poses(src, (lo, hi)), R.gauss_constants(1.0, 0.55)
    n.close()


@pytest.mark.parametrize("pose", POSES)
def test_derivatives_and_neighbours(case, pose):
    n, src, vm, poses, (d1, d2, _) = case
    p = poses[pose]
    assert n.get_radius_search()
    score, g, H = n.derivatives(p)
    offs, leaf, sqd = n.neighbours()
    ro, rl, rd = RR.neighbour_csr(vm, R.transform_cloud(R.pose_matrix(p), src))
    assert np.array_equal(offs, ro) and np.array_equal(leaf, rl) and np.array_equal(sqd, rd)
    rs, rg, rH, pairs = RR.derivatives(vm, src, p, RR.RADIUS, d1, d2)
    assert pairs == ro[-1]
    if pose == "all_outside":
        assert pairs == 0 and score == 0 and not g.any() and not H.any()
    elif pose == "third_outside":
        assert 0 < pairs < src.shape[0] // 4  # most of the cloud has left the map, some of it has not
    else:
        assert pairs > src.shape[0]
    assert abs(score - rs) <= REL * abs(rs)
    assert _close(g, rg) and _close(H, rH)
    assert np.array_equal(H, H.T)
    s2, g2, none = n.derivatives(p, compute_hessian=False)  # without the Hessian: the same score and gradient bits
    assert none is None and s2 == score and np.array_equal(g2, g)
    s3, g3, H3 = n.derivatives(p)  # twice: the same bits
    assert s3 == score and np.array_equal(g3, g) and np.array_equal(H3, H)
    assert _close(n.hessian(p), RR.hessian_only(vm, src, p, RR.RADIUS, d1, d2))
    assert np.array_equal(n.neighbours()[0], ro)  # computeHessian searched the same queries


def test_radius_is_not_the_direct_neighbourhood(case):
    n, src, vm, poses, (d1, d2, _) = case
    p = poses["typical"]
    score = n.derivatives(p)[0]
    assert abs(score - R.derivatives(vm, src, p, R.DIRECT7, d1, d2)[0]) > 1e-3 * abs(score)


def test_calculate_score(case):
    n, src, vm, poses, (d1, d2, d3) = case
    for name in POSES:
        T = R.pose_matrix(poses[name])
        ref = RR.calculate_score(vm, src, T, RR.RADIUS, d1, d2, d3)
        assert abs(n.calculate_score(T) - ref) <= REL * abs(ref), name


@pytest.mark.parametrize("n_src", [1, 63, 64, 65, 255, 256, 257])
def test_source_sizes(case, gorio, gpu, real, n_src):
    _, src, vm, poses, (d1, d2, d3) = case
    sub = src[np.linspace(0, src.shape[0] - 1, n_src).astype(int)] if n_src > 1 else vm.cent[0][None, :].copy()
    n = gorio.Ndt(device=gpu, radius_search=True)
    n.set_target(real[1])
    n.set_source(sub)
    p = poses["typical"] if n_src > 1 else np.zeros(6)
    score, g, H = n.derivatives(p)
    rs, rg, rH, pairs = RR.derivatives(vm, sub, p, RR.RADIUS, d1, d2)
    assert pairs > 0 and abs(score - rs) <= REL * abs(rs) and _close(g, rg) and _close(H, rH)
    ro, rl, rd = RR.neighbour_csr(vm, R.transform_cloud(R.pose_matrix(p), sub))
    offs, leaf, sqd = n.neighbours()
    assert np.array_equal(offs, ro) and np.array_equal(leaf, rl) and np.array_equal(sqd, rd)
    T = R.pose_matrix(p)
    ref = RR.calculate_score(vm, sub, T, RR.RADIUS, d1, d2, d3)
    assert abs(n.calculate_score(T) - ref) <= REL * abs(ref)
    n.close()


def test_source_without_any_neighbour_gives_exact_zeros(gorio, gpu, real):
    src, tgt, _ = real
    n = gorio.Ndt(device=gpu, radius_search=True)
    n.set_target(tgt)
    n.set_source(src[:300] + np.float32(4000.0))
    score, g, H = n.derivatives(np.zeros(6))
    assert score == 0 and not g.any() and not H.any() and not n.hessian(np.zeros(6)).any() and n.calculate_score(np.eye(4)) == 0
    assert not n.neighbours()[0].any()
    r = n.align()
    assert r["converged"] and r["nr_iterations"] == 0 and np.array_equal(r["T"], np.eye(4, dtype=np.float32))
    n.close()


def test_map_without_eligible_leaf_gives_zero_sums(gorio, gpu, real):
    n = gorio.Ndt(device=gpu, radius_search=True)
    n.set_target(_sparse_target())
    n.set_source(real[0][:257])
    score, g, H = n.derivatives(np.zeros(6))
    assert score == 0 and not g.any() and not H.any() and n.calculate_score(np.eye(4)) == 0
    offs, leaf, _ = n.neighbours()
    assert offs.shape[0] == 258 and not offs.any() and leaf.size == 0
    n.close()


def test_disabled_leaf_is_a_neighbour(gorio, gpu):
    pts, _ = S.rule_scene()
    vm = RR.build_voxel_map(pts, 1.0)
    src = (vm.cent + np.float32(0.05)).astype(np.float32)
    d1, d2, d3 = R.gauss_constants(1.0, 0.55)
    n = gorio.Ndt(device=gpu, radius_search=True)
    n.set_target(pts)
    n.set_source(src)
    score, g, H = n.derivatives(np.zeros(6))
    rs, rg, rH, _ = RR.derivatives(vm, src, np.zeros(6), RR.RADIUS, d1, d2)
    offs, leaf, _ = n.neighbours()
    assert (vm.count[leaf] == -1).any()
    assert abs(score - rs) <= REL * abs(rs) and _close(g, rg) and _close(H, rH)
    ref = RR.calculate_score(vm, src, np.eye(4), RR.RADIUS, d1, d2, d3)
    assert abs(n.calculate_score(np.eye(4)) - ref) <= REL * abs(ref)
    n.close()


def _align_both(gorio, gpu, src, tgt, **params):
    n = gorio.Ndt(device=gpu, radius_search=True, **params)
    n.set_target(tgt)
    n.set_source(src)
    r = n.align()
    n.close()
    ref = RR.Ndt(**params)
    ref.set_target(tgt)
    ref.set_source(src)
    q = ref.align()
    dt, dr = rot_err(q["T"], r["T"])
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    for k in ("converged", "nr_iterations", "n_derivatives", "n_hessians", "n_mt"):
        assert r[k] == q[k], (k, r[k], q[k])
    assert abs(r["trans_probability"] - q["trans_probability"]) <= 1e-6 * abs(q["trans_probability"]) + 1e-12
    return r


def test_align_real_pair(gorio, gpu, real):
    src, tgt, T = real
    r = _align_both(gorio, gpu, src, tgt, transformation_epsilon=0.01, max_iterations=64)
    dt, dr = rot_err(T, r["T"])
    assert r["converged"] and dt < 0.05 and dr < np.deg2rad(1.0)


def test_align_synthetic_radar_pair(gorio, gpu):
    src, tgt, _ = S.radar_pair()
    assert _align_both(gorio, gpu, src, tgt, transformation_epsilon=0.01, max_iterations=64)["converged"]


def test_switch_off_again_is_the_direct_handle(gorio, gpu, real):
    src, tgt, _ = real
    p = np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03])
    plain = gorio.Ndt(device=gpu, search=R.DIRECT1)
    plain.set_target(tgt)
    plain.set_source(src)
    n = gorio.Ndt(device=gpu, search=R.DIRECT1)
    n.set_target(tgt)
    n.set_source(src)
    with pytest.raises(gorio.GorioError) as e:
        n.neighbours()  # no radius evaluation yet
    assert e.value.code == -3
    n.set_radius_search(True)
    on = n.derivatives(p)
    assert n.get_params().search == R.DIRECT1  # params.search is kept
    n.set_radius_search(False)
    with pytest.raises(gorio.GorioError) as e:
        n.neighbours()  # a changed switch invalidates the lists
    assert e.value.code == -3
    off, ref = n.derivatives(p), plain.derivatives(p)
    assert off[0] == ref[0] and np.array_equal(off[1], ref[1]) and np.array_equal(off[2], ref[2]) and on[0] != off[0]
    a, b = n.align(), plain.align()
    assert np.array_equal(a["T"], b["T"]) and all(a[k] == b[k] for k in FIELDS)
    assert n.calculate_score(np.eye(4)) == plain.calculate_score(np.eye(4))
    n.close()
    plain.close()


def test_shared_target_one_centroid_index(gorio, gpu, real):
    src, tgt, _ = real
    params = dict(transformation_epsilon=0.01, max_iterations=64)
    owner = gorio.Ndt(device=gpu, search=R.DIRECT7, **params)
    owner.set_target(tgt)
    owner.set_source(src[::2])
    rad = gorio.Ndt(device=gpu, radius_search=True, **params)
    rad.set_source(src[1::2])
    rad.set_target_shared(owner)
    r_own = owner.align()  # DIRECT7: builds the map, not the centroid cloud
    caps = owner.capacities()
    r_rad = rad.align()
    # the centroid cloud and its index were built through the sharer, into the ONE target state: the sharer owns no buffer of it,
    # the owner's buffers did not move, and both handles report the same cloud
    assert rad.capacities()["target"] == rad.capacities()["leaves"] == rad.capacities()["keys"] == 0 and owner.capacities() == caps
    assert all(np.array_equal(a, b) for a, b in zip(rad.centroids(), owner.centroids()))
    priv = gorio.Ndt(device=gpu, radius_search=True, **params)
    priv.set_target(tgt)
    priv.set_source(src[1::2])
    p_rad = priv.align()
    priv.set_radius_search(False)
    priv.set_source(src[::2])
    p_own = priv.align()
    assert np.array_equal(r_rad["T"], p_rad["T"]) and all(r_rad[k] == p_rad[k] for k in FIELDS)
    assert np.array_equal(r_own["T"], p_own["T"]) and all(r_own[k] == p_own[k] for k in FIELDS)
    assert not np.array_equal(r_rad["T"], r_own["T"])
    for h in (owner, rad, priv):
        h.close()
