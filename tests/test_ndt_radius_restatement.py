"""CPU pins of tests/ndt_radius_restatement.py, the parity reference of NDT's radius neighbourhood (gorio_ndt_set_radius_search):
the centroid cloud is what VGC:282-326 builds, the neighbour order is the search's, and the inputs of the GPU tests are such that the
radius neighbourhood is NOT the DIRECT7 one (a GPU test could otherwise pass by running the wrong neighbourhood)."""
import numpy as np
import pytest

import ndt_radius_restatement as RR
import ndt_restatement as R
import ndt_scenes as S
import search_restatement as SR

f32 = np.float32


@pytest.fixture(scope="module")
def real():
    src, tgt, _ = S.real_pair()
    return src, tgt, RR.build_voxel_map(tgt, 1.0)


def _leaf_points(target, vm, pos):
    """The finite points of leaf `pos` in input order."""
    P = np.asarray(target, f32)
    P = P[np.isfinite(P).all(axis=1)]
    lin = (np.floor(P * vm.inv) - vm.min_b.astype(f32)).astype(np.int64) @ vm.mul
    return P[lin == vm.idx[pos]]


def test_centroids_are_float_running_sums(real):
    _, tgt, vm = real
    assert vm.cent.dtype == f32 and vm.cent.shape[0] == vm.cent_leaf.shape[0] > 200
    assert np.array_equal(vm.cent_leaf, np.nonzero((vm.count >= vm.min_points) | (vm.count == -1))[0])  # ascending leaf index
    rounded = vm.mean[vm.cent_leaf].astype(f32)
    differs = np.nonzero((vm.cent != rounded).any(axis=1))[0]
    assert differs.size > 0  # the float sum is not the rounded double mean: these leaves tell the two apart
    assert np.abs(vm.cent - rounded).max() < 1e-4  # and still the same point up to float rounding
    for c in differs[:3]:
        pts = _leaf_points(tgt, vm, vm.cent_leaf[c])
        s = np.zeros(3, f32)
        for p in pts:
            s = s + p
        assert np.array_equal(vm.cent[c], s / f32(pts.shape[0]))


def test_disabled_leaf_is_in_the_cloud_with_zero_icov():
    pts, cells = S.rule_scene()
    vm = RR.build_voxel_map(pts, 1.0)
    pos = {k: int(np.searchsorted(vm.idx, S.leaf_of(vm.min_b, vm.div_b, c))) for k, c in cells.items()}
    assert vm.count[pos["same"]] == -1 and pos["same"] in vm.cent_leaf and not vm.icov[pos["same"]].any()
    assert pos["five"] not in vm.cent_leaf  # below min_points_per_voxel: never pushed
    assert {pos[k] for k in ("six", "line", "same", "generic", "negative")} == set(vm.cent_leaf.tolist())
    c = int(np.nonzero(vm.cent_leaf == pos["same"])[0][0])
    assert np.array_equal(vm.cent[c], np.array([6.5, 0.5, 0.25], f32))
    # a source point on that centroid has it as its first neighbour, and the pair enters the score's divisor
    offs, leaf, sqd = RR.neighbour_csr(vm, vm.cent[c][None, :])
    assert offs[1] >= 1 and leaf[0] == pos["same"] and sqd[0] == 0


def test_neighbour_order_and_rule(real):
    src, _, vm = real
    q = R.transform_cloud(R.pose_matrix(np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03])), src)[::5]
    offs, leaf, sqd = RR.neighbour_csr(vm, q)
    r2 = SR.radius_bound(float(vm.leaf))
    assert (sqd < r2).all() and np.diff(offs).max() > 1 and (np.diff(offs) == 0).any()
    cent_of = {int(l): i for i, l in enumerate(vm.cent_leaf)}
    for i in range(q.shape[0]):
        d, c = sqd[offs[i]:offs[i + 1]], np.array([cent_of[int(l)] for l in leaf[offs[i]:offs[i + 1]]])
        assert np.array_equal(np.lexsort((c, d)), np.arange(d.size))  # ascending (distance, centroid index)
        inside = np.nonzero(SR.sqdist(q[i:i + 1], vm.cent)[0] < r2)[0]
        assert set(inside.tolist()) == set(c.tolist())
    nb = RR.neighbourhood(vm, q, RR.RADIUS)
    assert len(nb) == np.diff(offs).max() and np.array_equal(np.sum([p >= 0 for p in nb], axis=0), np.diff(offs))
    assert np.array_equal(nb[0][np.diff(offs) > 0], leaf[offs[:-1][np.diff(offs) > 0]])


def test_radius_neighbourhood_is_not_direct7(real):
    src, _, vm = real
    q = R.transform_cloud(np.eye(4, dtype=f32), src)
    offs, leaf, _ = RR.neighbour_csr(vm, q)
    d7 = np.stack(R.neighbourhood(vm, q, R.DIRECT7), axis=1)
    differ = 0
    for i in range(q.shape[0]):
        differ += set(leaf[offs[i]:offs[i + 1]].tolist()) != set(d7[i][d7[i] >= 0].tolist())
    assert differ > q.shape[0] // 2, differ / q.shape[0]


def test_rebound_functions_are_the_restatements_code():
    assert RR.derivatives.__code__ is R.derivatives.__code__ and RR.Ndt.align.__code__ is R.Ndt.align.__code__
    assert RR.derivatives.__globals__["neighbourhood"] is RR.neighbourhood and R.derivatives.__globals__["neighbourhood"] is R.neighbourhood


def test_align_recovers_the_known_transform(real):
    from conftest import rot_err

    src, tgt, _ = real
    T = S.real_pair()[2]
    ref = RR.Ndt(transformation_epsilon=0.01, max_iterations=64)
    ref.set_target(tgt)
    ref.set_source(src)
    r = ref.align()
    dt, dr = rot_err(T, r["T"])
    assert r["converged"] and dt < 0.05 and dr < np.deg2rad(1.0), (dt, np.rad2deg(dr))
