"""GPU: pygicp (go-rio_amd/pygicp.py, the surface of fast_apdgicp/src/python/main.cpp) -- downsample() against the restatement of
pcl::ApproximateVoxelGrid, align_points() and the classes against ApdGicp configured by hand with the same settings."""
import importlib
import os
import sys

import numpy as np
import pytest

import approx_voxel_restatement as R
import ndt_scenes
from approx_voxel_scenes import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
prep = importlib.import_module("go-rio_amd.prep")
F = np.float32
METHODS = ["GICP", "VGICP", "VGICP_CUDA", "NDT_CUDA"]


@pytest.fixture(scope="module")
def pair():
    """(target, source) as float64 (n, 3), about 2.6 k points each: the type pygicp takes."""
    src, tgt, _ = ndt_scenes.real_pair()
    return tgt[::2].astype(np.float64), src[::2].astype(np.float64)


def by_hand(gorio, method, tgt, src, k=15, resolution=1.0, search="DIRECT1", radius=1.5):
    """ApdGicp set up as the reference's class would be by align_points (main.cpp:96-129); float clouds in."""
    s = dict(DIRECT1=apd.VOXEL_DIRECT1, DIRECT7=apd.VOXEL_DIRECT7, DIRECT27=apd.VOXEL_DIRECT27)[search]
    g = gorio.ApdGicp()
    if method == "GICP":
        g.set_method(apd.METHOD_GICP)
        g.set_params(k_correspondences=k, corr_dist_threshold=sys.float_info.max)
    elif method == "VGICP":
        g.set_method(apd.METHOD_VGICP, resolution, s, apd.VOXEL_ADDITIVE)
        g.set_params(k_correspondences=k)  # FastGICP's constructor leaves corr_dist_threshold at FLT_MAX: the library's default
    elif method == "VGICP_CUDA":
        g.set_method(apd.METHOD_VGICP_CUDA, resolution, s)
        g.set_ndt_cuda_params(g.get_ndt_cuda_params()["distance_mode"], radius)
    else:
        g.set_method(apd.METHOD_NDT_CUDA, resolution, s)
        g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, radius)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    return g


def test_downsample_equals_restatement(gpu, pair):
    import pygicp

    tgt, _ = pair
    got = pygicp.downsample(tgt, 0.25)
    want = R.sequential(tgt.astype(F), 0.25)
    assert got.dtype == np.float64 and got.shape == want.shape and 0 < len(want) < len(tgt)
    assert same(got.astype(F), want) and np.array_equal(got, want.astype(np.float64))
    assert pygicp.downsample(np.zeros((0, 3)), 0.25).shape == (0, 3)


@pytest.mark.parametrize("resolution", [-1.0, 0.25])
@pytest.mark.parametrize("method", METHODS)
def test_align_points_equals_apdgicp_by_hand(gpu, gorio, pair, method, resolution):
    import pygicp

    tgt, src = pair
    kw = dict(voxel_resolution=1.0, neighbor_search_method="DIRECT7") if method != "GICP" else {}
    T = pygicp.align_points(tgt, src, method=method, downsample_resolution=resolution, **kw)
    t32, s32 = tgt.astype(F), src.astype(F)
    if resolution > 0:
        t32, s32 = prep.approx_voxel_downsample(t32, resolution), prep.approx_voxel_downsample(s32, resolution)
        assert same(t32, R.sequential(tgt.astype(F), resolution)) and len(t32) < len(tgt)
    g = by_hand(gorio, method, t32, s32, search="DIRECT7" if method != "GICP" else "DIRECT1")
    want = g.align()["T"]
    assert T.dtype == np.float64 and np.array_equal(T, want.astype(np.float64))
    assert not np.array_equal(T, np.eye(4))


@pytest.mark.parametrize("method", METHODS)
def test_class_route_equals_align_points(gpu, pair, method):
    import pygicp

    tgt, src = pair
    if method == "GICP":
        reg = pygicp.FastGICP()
        reg.set_num_threads(4)
        reg.set_correspondence_randomness(15)
        reg.set_max_correspondence_distance(sys.float_info.max)
    elif method == "VGICP":
        reg = pygicp.FastVGICP()
        reg.set_correspondence_randomness(15)
        reg.set_resolution(1.0)
        reg.set_neighbor_search_method("DIRECT7")
    elif method == "VGICP_CUDA":
        reg = pygicp.FastVGICPCuda()
        reg.set_correspondence_randomness(15)
        reg.set_neighbor_search_method("DIRECT7", 1.5)
        reg.set_resolution(1.0)
    else:
        reg = pygicp.NDTCuda()
        reg.set_resolution(1.0)
        reg.set_neighbor_search_method("DIRECT7", 1.5)
    reg.set_input_target(tgt)
    reg.set_input_source(src)
    T = reg.align()
    kw = dict(neighbor_search_method="DIRECT7") if method != "GICP" else {}
    want = pygicp.align_points(tgt, src, method=method, **kw)
    assert T.dtype == F and np.array_equal(T.astype(np.float64), want)
    assert np.array_equal(reg.get_final_transformation(), T)
    H = reg.get_final_hessian()
    assert H.shape == (6, 6) and np.isfinite(H).all() and np.abs(H).max() > 0 and np.allclose(H, H.T, rtol=0.0, atol=1e-12 * np.abs(H).max())


def test_swap_source_and_target_gives_the_inverse(gpu, pair, pose_err):
    """swap_source_and_target followed by align returns the inverse pose within 1e-3 (m and rad).

    The target is the source moved rigidly by 0.3 m / 2 degrees, the SAME points: both directions then have an exact optimum (T and its
    inverse, cost zero) and mutual nearest neighbours, so what the bound sees is the clouds and covariances changing sides and the
    termination step of the class (5e-4 m, which pygicp cannot change).  Two different samples of a surface do not have that property:
    src -> nearest tgt and tgt -> nearest src are different pair sets, and the two optima differ by the sampling (observed on the
    two halves of the real scan: 1.1e-2 m)."""
    import pygicp

    _, src = pair
    T0 = importlib.import_module("go-rio_amd.synth").gt_transform([0.30, -0.20, 0.05], [0.5, -0.4, 2.0])
    tgt = (src @ T0[:3, :3].T + T0[:3, 3]).astype(F).astype(np.float64)
    reg = pygicp.FastGICP()
    reg.set_input_target(tgt)
    reg.set_input_source(src)
    T = reg.align()
    te0, re0 = pose_err(T0, T)
    reg.swap_source_and_target()
    Tinv = reg.align()
    te, re = pose_err(np.linalg.inv(T.astype(np.float64)), Tinv)
    print(f"forward: {te0:.3e} m, {re0:.3e} rad from the truth; swap: {te:.3e} m, {re:.3e} rad from the inverse")
    assert te < 1e-3 and re < 1e-3
