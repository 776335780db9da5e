"""pygicp on the MI355X: the surface of the reference's pybind11 module (fast_apdgicp/src/python/main.cpp:152-216, "PY"), every call
served by libgorio_amd.so.  Nothing here computes: downsample() is gorio_prep_approx_voxel_downsample (pcl::ApproximateVoxelGrid, as
PY:46-62 uses it), and each registration object owns ONE ApdGicp handle switched to its method with gorio_apd_set_method, the way the
C++ drop-in classes of go-rio_amd/host do.  No CPU fallback: without the library or a HIP device the calls raise.

    import pygicp                                   # the top-level pygicp.py re-exports this module
    T = pygicp.align_points(target, source, method="VGICP_CUDA", downsample_resolution=0.25)

The methods the reference compiles only with BUILD_VGICP_CUDA (VGICP_CUDA, NDT_CUDA) are always present here.  num_threads is accepted
and ignored.
"""
import sys

import numpy as np

from . import apd, prep
from .apd import ApdGicp

__version__ = "dev"  # PY:218-222 without VERSION_INFO
__all__ = ["downsample", "align_points", "LsqRegistration", "FastGICP", "FastVGICP", "FastVGICPCuda", "NDTCuda"]

_DBL_MAX = float(np.finfo(np.float64).max)
_SEARCH = {"DIRECT1": apd.VOXEL_DIRECT1, "DIRECT7": apd.VOXEL_DIRECT7, "DIRECT27": apd.VOXEL_DIRECT27, "DIRECT_RADIUS": apd.VOXEL_DIRECT_RADIUS}


def _search_method(name):  # PY:21-34
    if name in _SEARCH:
        return _SEARCH[name]
    print(f"error: unknown neighbor search method {name}", file=sys.stderr)
    return apd.VOXEL_DIRECT1


def _eigen2pcl(points):  # PY:36-44: Eigen::Matrix<double, -1, 3> rows cast to float
    p = np.asarray(points, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise TypeError("points must be an (n, 3) array")
    return np.ascontiguousarray(p.astype(np.float32))


def _filter(cloud, resolution, device=0):
    return prep.approx_voxel_downsample(cloud, float(resolution), device=device) if cloud.shape[0] else cloud


def downsample(points, downsample_resolution):
    """PY:46-62: pcl::ApproximateVoxelGrid<pcl::PointXYZ> with a cubic leaf on the float cast of `points`, back as float64 (m, 3)."""
    return _filter(_eigen2pcl(points), downsample_resolution).astype(np.float64)


class LsqRegistration:
    """fast_gicp::LsqRegistration as PY:169-182 binds it.  The base of the four classes; not constructible in the reference either."""

    def __init__(self, device=0):
        if type(self) is LsqRegistration:
            raise TypeError("pygicp.LsqRegistration: No constructor defined!")
        self._g = ApdGicp(device=device)
        self._H = np.zeros((6, 6), np.float64)
        self._T = np.eye(4, dtype=np.float32)

    def _select(self, method, resolution, search, mode=None):  # gorio_apd_set_method only when something differs: a repeated call drops the correspondences held
        cur = self._g.get_method()
        mode = cur["voxel_mode"] if mode is None else mode
        if (cur["method"], cur["voxel_resolution"], cur["voxel_search"], cur["voxel_mode"]) != (method, resolution, search, mode):
            self._g.set_method(method, resolution, search, mode)

    def _push(self):  # the object's settings -> the handle, before the align (as push_settings of the C++ drop-ins)
        raise NotImplementedError

    def set_input_target(self, points):
        self._g.setInputTarget(_eigen2pcl(points))

    def set_input_source(self, points):
        self._g.setInputSource(_eigen2pcl(points))

    def swap_source_and_target(self):
        self._g.swapSourceAndTarget()

    def get_final_hessian(self):
        return self._H.copy()

    def get_final_transformation(self):
        return self._T.copy()

    def align(self, initial_guess=np.eye(4, dtype=np.float32)):
        self._push()
        r = self._g.align(np.asarray(initial_guess, np.float32))
        self._T, self._H = r["T"].copy(), r["H"].copy()
        return self._T.copy()


class FastGICP(LsqRegistration):
    """PY:184-189."""

    def __init__(self, device=0):
        super().__init__(device)
        self._k = 20
        self._corr_dist = float(np.finfo(np.float32).max)  # fast_gicp_impl.hpp:14-30

    def set_num_threads(self, n):
        pass

    def set_correspondence_randomness(self, k):
        self._k = int(k)

    def set_max_correspondence_distance(self, d):
        self._corr_dist = float(d)

    def _push_params(self):
        p = self._g.params
        if (p.k_correspondences, p.corr_dist_threshold) != (self._k, self._corr_dist):
            self._g.set_params(k_correspondences=self._k, corr_dist_threshold=self._corr_dist)

    def _push(self):
        self._select(apd.METHOD_GICP, 1.0, apd.VOXEL_DIRECT1, apd.VOXEL_ADDITIVE)
        self._push_params()


class FastVGICP(FastGICP):
    """PY:191-195."""

    def __init__(self, device=0):
        super().__init__(device)
        self._res, self._search = 1.0, apd.VOXEL_DIRECT1

    def set_resolution(self, resolution):
        self._res = float(resolution)

    def set_neighbor_search_method(self, method):
        self._search = _search_method(method)

    def _push(self):
        self._select(apd.METHOD_VGICP, self._res, self._search, apd.VOXEL_ADDITIVE)
        self._push_params()


def _push_voxel_cuda(reg, method):
    """What FastVGICPCuda and NDTCuda share: resolution, search method and its radius -> the handle (as push_method of the C++ drop-ins)."""
    cur = reg._g.get_ndt_cuda_params()
    differ = cur["radius"] != reg._radius
    # the library checks a DIRECT_RADIUS radius in the call that puts it in use: the radius goes first when DIRECT_RADIUS is selected, last otherwise
    if differ and reg._search == apd.VOXEL_DIRECT_RADIUS:
        reg._g.set_ndt_cuda_params(cur["distance_mode"], reg._radius)
    reg._select(method, reg._res, reg._search)
    if differ and reg._search != apd.VOXEL_DIRECT_RADIUS:
        reg._g.set_ndt_cuda_params(cur["distance_mode"], reg._radius)


class FastVGICPCuda(LsqRegistration):
    """PY:198-206.  Constructor defaults of fast_vgicp_cuda_impl.hpp:22-32: k 20, DIRECT1, resolution 1.0."""

    def __init__(self, device=0):
        super().__init__(device)
        self._res, self._search, self._radius = 1.0, apd.VOXEL_DIRECT1, -1.0

    def set_resolution(self, resolution):
        self._res = float(resolution)

    def set_neighbor_search_method(self, method="DIRECT1", radius=1.5):
        self._search, self._radius = _search_method(method), float(radius)

    def set_correspondence_randomness(self, k):  # the no-op it is in the reference (fast_vgicp_cuda_impl.hpp:38): k stays 20
        pass

    def _push(self):
        _push_voxel_cuda(self, apd.METHOD_VGICP_CUDA)


class NDTCuda(LsqRegistration):
    """PY:208-215.  Constructor defaults of ndt_cuda_impl.hpp:11-14: D2D, DIRECT7, resolution 1.0."""

    def __init__(self, device=0):
        super().__init__(device)
        self._res, self._search, self._radius = 1.0, apd.VOXEL_DIRECT7, -1.0

    def set_neighbor_search_method(self, method="DIRECT1", radius=1.5):
        self._search, self._radius = _search_method(method), float(radius)

    def set_resolution(self, resolution):
        self._res = float(resolution)

    def _push(self):
        _push_voxel_cuda(self, apd.METHOD_NDT_CUDA)


def align_points(target, source, method="GICP", downsample_resolution=-1.0, k_correspondences=15, max_correspondence_distance=_DBL_MAX, voxel_resolution=1.0, num_threads=0,
                 neighbor_search_method="DIRECT1", neighbor_search_radius=1.5, initial_guess=np.eye(4, dtype=np.float32)):
    """PY:64-142: (optionally) both clouds through pcl::ApproximateVoxelGrid, then one align of the chosen class; the float pose as float64."""
    tgt, src = _eigen2pcl(target), _eigen2pcl(source)
    if downsample_resolution > 0.0:
        tgt, src = _filter(tgt, downsample_resolution), _filter(src, downsample_resolution)
    if method == "GICP":
        reg = FastGICP()
        reg.set_max_correspondence_distance(max_correspondence_distance)
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_num_threads(num_threads)
    elif method == "VGICP":
        reg = FastVGICP()
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_resolution(voxel_resolution)
        reg.set_neighbor_search_method(neighbor_search_method)
        reg.set_num_threads(num_threads)
    elif method == "VGICP_CUDA":
        reg = FastVGICPCuda()
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_neighbor_search_method(neighbor_search_method, neighbor_search_radius)
        reg.set_resolution(voxel_resolution)
    elif method == "NDT_CUDA":
        reg = NDTCuda()
        reg.set_resolution(voxel_resolution)
        reg.set_neighbor_search_method(neighbor_search_method, neighbor_search_radius)
    else:
        print(f"error: unknown registration method {method}", file=sys.stderr)
        return np.eye(4, dtype=np.float64)
    reg._g.setInputTarget(tgt)  # already float clouds: no second cast
    reg._g.setInputSource(src)
    return reg.align(initial_guess).astype(np.float64)
