"""The map comparisons the GPU tests share: a device voxel map against its CPU restatement, with the gates of the modules that first
stated them (tests/test_gicp_variants_gpu.py for the FastVGICP map, tests/test_ndt_gpu.py for the NDT grid)."""
import numpy as np

import ndt_restatement as R

MAP_RTOL = 1e-12  # voxel means / covariances: the same double sums in the same order, only the final division differs
NDT_REL = 1e-9    # inverse covariances of the NDT leaves, relative to the largest entry of the leaf's matrix


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _rel_rows(a, b):
    """rel() of every voxel's row at once: max |a - b| over the voxel / max |b| over the voxel"""
    n = len(b)
    if n == 0:
        return 0.0
    d = np.abs(np.asarray(a) - np.asarray(b)).reshape(n, -1).max(axis=1)
    s = np.maximum(np.abs(np.asarray(b)).reshape(n, -1).max(axis=1), 1e-300)
    return float((d / s).max())


def check_map(vm, ref):
    """FastVGICP: getVoxelMap() against gicp_restatement.VoxelMap -- coordinates and counts exact, means and covariances per voxel"""
    assert np.array_equal(vm["coord"], ref.coord)
    assert np.array_equal(vm["num_points"], ref.num_points)
    assert vm["mean"].shape == ref.mean.shape and vm["cov"].shape == ref.cov.shape
    m = _rel_rows(vm["mean"], ref.mean)
    c = _rel_rows(vm["cov"], ref.cov)
    print("voxel map: %d voxels, mean %.2e cov %.2e (per-voxel relative)" % (len(ref.mean), m, c))
    assert m < MAP_RTOL and c < MAP_RTOL


def check_ndt_map(gorio, gpu, target, resolution=1.0, ref=None):
    """NDT: Ndt.voxels() against ndt_restatement.build_voxel_map (`ref`: that map when the caller holds it already)"""
    if ref is None:
        ref = R.build_voxel_map(target, resolution)
    n = gorio.Ndt(device=gpu, resolution=resolution)
    n.set_target(target)
    v = n.voxels()
    n.close()
    assert np.array_equal(v["leaf_index"], ref.idx)
    assert np.array_equal(v["min_b"], ref.min_b) and np.array_equal(v["div_b"], ref.div_b)
    raw_cnt = np.where(ref.count < 0, -1, ref.count)
    assert np.array_equal(v["nr_points"], raw_cnt)  # the disabled flag (-1) of every leaf included
    assert np.array_equal(v["mean"], ref.mean)
    big = np.abs(ref.count) >= 6
    big |= ref.count == -1
    assert np.array_equal(v["cov_raw"][big], ref.cov_raw[big])
    on = ref.count >= 6
    if on.any():
        scale = np.abs(ref.icov[on]).max(axis=(1, 2), keepdims=True)
        assert (np.abs(v["icov"][on] - ref.icov[on]) / scale).max() < NDT_REL
        cscale = np.abs(ref.cov[on]).max(axis=(1, 2), keepdims=True)
        assert (np.abs(v["cov"][on] - ref.cov[on]) / cscale).max() < NDT_REL
    return ref, v
