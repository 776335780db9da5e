"""CPU checks of tests/vgicp_cuda_restatement.py, the NumPy definition of GORIO_METHOD_VGICP_CUDA: both covariance rules against a float64
evaluation of the same formulas, the origin-padding quirk of the RBF pass, the PLANE filter, the conditions the GPU tests rely on, and the
acceptance shape of the reference's gicp_test.cpp:148-149."""
import functools

import numpy as np
import pytest

import ndt_cuda_restatement as nr
import vgicp_cuda_restatement as vr
from conftest import rot_err

F = np.float32
NN = [vr.CPU_PARALLEL_KDTREE, vr.GPU_BRUTEFORCE, vr.GPU_RBF_KERNEL]


@functools.lru_cache(maxsize=None)
def fixture_raw(n, side, rbf):
    """raw covariances of one cloud of scene_pair(n), computed once for the tests below"""
    c = vr.scene_pair(n)[side]
    return vr.cov_rbf(c, 0.5, 3.0) if rbf else vr.cov_knn(c, vr.knn(c, 20))


@pytest.mark.parametrize("k", [5, 20])
def test_knn_covariance_float32_against_float64(k):
    """k float32 additions of products bounded by m = max |p|^2 in the list, a division and a subtraction of two numbers of that size: the
    error stays below (k + 3) eps m."""
    c = vr.rail_scene(700)
    lists = vr.knn(c, k)
    assert np.array_equal(lists[:, 0], np.arange(700))  # the point itself comes first (distance 0)
    a, b = vr.cov_knn(c, lists), vr.cov_knn(c, lists, np.float64)
    m = (c[lists].astype(np.float64) ** 2).sum(axis=2).max(axis=1)
    assert a.dtype == F and np.all(np.abs(a - b).max(axis=1) <= (k + 3) * np.finfo(F).eps * m)
    ref = np.cov(c[lists[0]].astype(np.float64).T, bias=True)
    assert np.allclose(vr.full(b[0]), ref, atol=1e-12)


def test_rbf_covariance_float32_against_float64():
    """the weighted sums run over at most n_ext terms with weights <= 1; the same bound with the number of terms in range"""
    c = vr.rail_scene(700)
    a, b = vr.cov_rbf(c, 0.5, 3.0), vr.cov_rbf(c, 0.5, 3.0, np.float64)
    ext = np.zeros((1024, 3))
    ext[:700] = c
    d2 = vr.sqdist(c, ext.astype(F), np.float64)
    inr = d2 <= 9.0
    m = np.where(inr, (ext ** 2).sum(axis=1)[None, :], 0.0).max(axis=1)
    terms = inr.sum(axis=1)
    assert a.dtype == F and np.all(np.abs(a - b).max(axis=1) <= (terms + 3) * np.finfo(F).eps * np.maximum(m, 1e-3))
    # against the textbook weighted covariance, in double, of one point
    i = 5
    w = np.where(inr[i], np.exp(-0.5 * d2[i]), 0.0)
    mu = (w[:, None] * ext).sum(axis=0) / w.sum()
    ref = (w[:, None, None] * ext[:, :, None] * ext[:, None, :]).sum(axis=0) / w.sum() - np.outer(mu, mu)
    assert np.allclose(vr.full(b[i]), ref, atol=1e-9)


def test_max_dist_default_is_five_widths():
    assert vr.max_dist(0.5, 3.0) == 3.0 and vr.max_dist(0.5, -1.0) == 2.5 and vr.max_dist(0.4, 0.0) == 2.0  # VI:46-50


def test_origin_padding_quirk():
    """700 points are padded to 1024 with 324 points at the origin: a point within max_dist of the origin gets phantom neighbours there, the
    others are untouched bit for bit; 512 points are not padded at all."""
    c = vr.rail_scene(700)
    quirk, plain = vr.cov_rbf(c, 0.5, 3.0), vr.cov_rbf(c, 0.5, 3.0, pad=False)
    near = (c.astype(np.float64) ** 2).sum(axis=1) <= 9.0
    assert 10 < near.sum() < 690
    changed = np.any(quirk.view(np.uint32) != plain.view(np.uint32), axis=1)
    assert np.all(changed[near]) and not np.any(changed[~near])
    cut = c[:512]
    assert np.array_equal(vr.cov_rbf(cut, 0.5, 3.0).view(np.uint32), vr.cov_rbf(cut, 0.5, 3.0, pad=False).view(np.uint32))
    # the same 512 points inside the 700-point cloud see 188 more real points and the padding: different covariances near the origin only
    diff = np.any(quirk[:512].view(np.uint32) != vr.cov_rbf(np.r_[cut, c[512:]], 0.5, 3.0, pad=False)[:512].view(np.uint32), axis=1)
    assert np.array_equal(diff, near[:512])


def test_plane_filter_drops_an_exact_line_and_keeps_a_plane():
    t = np.linspace(0.0, 4.0, 60)
    line = np.c_[1.0 + t, 2.0 + 0.5 * t, 0.25 * t].astype(F)
    keep, _ = vr.regularize(vr.cov_knn(line, vr.knn(line, 10)), vr.PLANE)
    assert not keep.any()
    g = np.stack(np.meshgrid(np.arange(8.0), np.arange(8.0)), -1).reshape(-1, 2)
    plane = np.c_[g, np.zeros(64)].astype(F)
    keep, cov = vr.regularize(vr.cov_knn(plane, vr.knn(plane, 9)), vr.PLANE)
    assert keep.all()
    assert np.allclose(vr.full(cov), np.diag([1.0, 1.0, 1e-3]), atol=1e-6)  # the normal takes 1e-3


def test_regularisations():
    raw = fixture_raw(700, 1, False)
    for method in (vr.NONE, vr.NORMALIZED_MIN_EIG):
        keep, cov = vr.regularize(raw, method)
        assert keep.all() and np.array_equal(cov.view(np.uint32), raw.view(np.uint32))
    keep, cov = vr.regularize(raw, vr.MIN_EIG)
    assert keep.all() and np.linalg.eigvalsh(vr.full(cov.astype(np.float64))).min() >= 1e-3 * (1 - 1e-4)
    keep, cov = vr.regularize(raw, vr.FROBENIUS)
    C = vr.full(raw[3].astype(np.float64)) + 1e-3 * np.eye(3)
    assert keep.all() and np.allclose(vr.full(cov[3]), np.linalg.inv(np.linalg.inv(C) / np.linalg.norm(np.linalg.inv(C))), rtol=1e-5)


@pytest.mark.parametrize("rbf", [False, True])
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n", [700, 3000])
def test_fixture_filter_conditions(n, side, rbf):
    """what tests/test_vgicp_cuda_gpu.py relies on: no point within 1 % of the threshold (a last-bit difference of a raw covariance cannot
    flip a keep flag), between 2 % and 50 % dropped"""
    r = vr.plane_ratio(fixture_raw(n, side, rbf))
    dropped = np.mean(~(r > vr.PLANE_RATIO))
    print("n %d side %d rbf %d: dropped %.3f, closest to the threshold %.4f" % (n, side, rbf, dropped, np.min(np.abs(r - 0.1)) / 0.1))
    assert np.min(np.abs(r - vr.PLANE_RATIO)) >= 0.01 * vr.PLANE_RATIO
    assert 0.02 <= dropped <= 0.5


def test_plain_scene_drops_nothing():
    c = nr.structured_scene(700)
    assert np.all(vr.plane_ratio(vr.cov_knn(c, vr.knn(c, 20))) > vr.PLANE_RATIO)


@functools.lru_cache(maxsize=None)
def aligned(nn, opt):
    src, tgt, T = vr.scene_pair(3000)
    r = vr.VgicpCuda(nn_method=nn)
    r.setInputSource(src)
    r.setInputTarget(tgt)
    return r, r.align(optimizer=opt), T


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("nn", NN)
def test_known_transform_is_recovered_with_decisions_off_their_boundaries(nn, opt):
    """gicp_test.cpp:148-149: within 0.05 m and 1 degree.  And the margins tests/test_ndt_cuda_gpu.py uses for the shell's decisions: every
    rho at least 1e-3 from 0, every convergence measure at least 0.01 from 1."""
    r, out, T = aligned(nn, opt)
    te, re_ = rot_err(T, out["T"])
    assert out["converged"] and te < 0.05 and np.degrees(re_) < 1.0, (te, np.degrees(re_))
    assert all(abs(x) >= 1e-3 for x in out["rhos"]) and all(abs(m - 1.0) >= 0.01 for m in out["measures"])
    assert r.builds == dict(raw=2, kept=2, map=1)  # both clouds filtered, one map, nothing made twice


def test_bruteforce_is_the_kdtree_path():
    a, b = aligned(vr.CPU_PARALLEL_KDTREE, "LM")[1], aligned(vr.GPU_BRUTEFORCE, "LM")[1]
    assert a["T"].tobytes() == b["T"].tobytes()


def test_lifecycle_rebuilds_what_depends_on_a_setting():
    src, tgt, _ = vr.scene_pair(700)
    r = vr.VgicpCuda()
    r.setInputSource(src)
    r.setInputTarget(tgt)
    r.linearize(np.eye(4))
    assert r.builds == dict(raw=2, kept=2, map=1)
    r.resolution = 2.0
    r.linearize(np.eye(4))
    assert r.builds == dict(raw=2, kept=2, map=2)
    r.regularization = vr.MIN_EIG
    r.linearize(np.eye(4))
    assert r.builds == dict(raw=2, kept=4, map=3) and len(r.kept(r.source)["index"]) == 700
    r.swapSourceAndTarget()
    r.linearize(np.eye(4))
    assert r.builds == dict(raw=2, kept=4, map=4)  # the covariances went with the clouds, the new target's map is built
    r.nn_method = vr.GPU_RBF_KERNEL
    r.linearize(np.eye(4))
    assert r.builds == dict(raw=4, kept=6, map=5)


def test_empty_pair_list_when_everything_is_filtered():
    t = np.linspace(0.0, 4.0, 60)
    line = np.c_[1.0 + t, 2.0 + 0.5 * t, 0.25 * t].astype(F)
    _, tgt, _ = vr.scene_pair(700)
    r = vr.VgicpCuda(k=10)
    r.setInputSource(line)
    r.setInputTarget(tgt)
    err, H, b = r.linearize(np.eye(4))
    assert len(r.kept(r.source)["index"]) == 0 and len(r.pairs) == 0 and err == 0.0 and not H.any() and not b.any()
    out = r.align()  # as the disjoint clouds of NDTCuda: the shell stops after one linearisation and leaves the guess
    assert out["converged"] and out["n_linearize"] == 1 and np.array_equal(out["T"], np.eye(4, dtype=F))
