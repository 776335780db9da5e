"""ctypes binding of include/gorio_apd.h (APD-GICP scan matching on MI355X).

`ApdGicp` mirrors the public surface of fast_gicp::FastAPDGICP (fast_apdgicp.hpp:48-79 + the pcl::Registration calls the
nodelets make), one method per reference member, so parity tests read like the reference's own gicp_test.cpp.  All numerics
happen in libgorio_amd.so on the GPU; nothing here computes.
"""
import ctypes as C
import os

import numpy as np

REG_NONE, REG_MIN_EIG, REG_NORMALIZED_MIN_EIG, REG_PLANE, REG_FROBENIUS = range(5)
OPT_GAUSS_NEWTON, OPT_LEVENBERG_MARQUARDT = 0, 1
SEARCH_BRUTE_FORCE, SEARCH_PRUNED = 0, 1


class GorioError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gorio error {code}: {msg}")
        self.code = code


class ApdParams(C.Structure):
    """gorio_apd_params (include/gorio_apd.h)."""

    _fields_ = [
        ("k_correspondences", C.c_int),
        ("regularization", C.c_int),
        ("dist_var", C.c_double),
        ("azimuth_var", C.c_double),
        ("elevation_var", C.c_double),
        ("corr_dist_threshold", C.c_double),
        ("max_iterations", C.c_int),
        ("rotation_epsilon", C.c_double),
        ("transformation_epsilon", C.c_double),
        ("optimizer", C.c_int),
        ("lm_max_iterations", C.c_int),
        ("lm_init_lambda_factor", C.c_double),
        ("search", C.c_int),
        ("cl_weight_points", C.c_int),
        ("keep_knn_indices", C.c_int),
    ]


# every symbol include/gorio_apd.h declares (tests check that the library exports all of them)
APD_SYMBOLS = [
    "gorio_apd_create", "gorio_apd_destroy", "gorio_apd_last_error", "gorio_apd_default_params", "gorio_apd_set_params",
    "gorio_apd_get_params", "gorio_apd_set_source", "gorio_apd_set_target", "gorio_apd_set_source_device",
    "gorio_apd_set_target_device", "gorio_apd_set_clouds_device_batch", "gorio_apd_clear_source", "gorio_apd_clear_target", "gorio_apd_swap_source_and_target",
    "gorio_apd_set_source_covariances", "gorio_apd_set_target_covariances", "gorio_apd_get_source_covariances",
    "gorio_apd_get_target_covariances", "gorio_apd_calculate_covariances", "gorio_apd_get_knn_indices", "gorio_apd_align",
    "gorio_apd_align_batch", "gorio_apd_linearize", "gorio_apd_compute_error", "gorio_apd_get_correspondences",
    "gorio_apd_get_mahalanobis", "gorio_apd_transform_source", "gorio_apd_fitness_score", "gorio_apd_fitness_score_batch", "gorio_apd_set_profiling",
    "gorio_apd_get_stage_times", "gorio_apd_set_target_shared", "gorio_comm_get_unique_id", "gorio_apd_comm_init", "gorio_apd_comm_destroy", "gorio_apd_comm_info", "gorio_apd_debug_set_shard", "gorio_apd_debug_set_schedule", "gorio_apd_debug_get_index", "gorio_apd_debug_knn_redo_groups", "gorio_apd_set_target_submap", "gorio_apd_get_target_points",
    "gorio_apd_set_method", "gorio_apd_get_method", "gorio_apd_get_voxelmap", "gorio_apd_get_voxel_correspondences",
    "gorio_apd_set_gicp_omp_params", "gorio_apd_get_gicp_omp_params", "gorio_apd_gicp_omp_update", "gorio_apd_gicp_omp_evaluate", "gorio_apd_gicp_omp_diag",
    "gorio_apd_gicp_omp_align_batch", "gorio_apd_gicp_omp_batch_diag",
    "gorio_apd_set_icp_params", "gorio_apd_get_icp_params", "gorio_apd_icp_diag", "gorio_apd_icp_step", "gorio_apd_icp_align_batch", "gorio_apd_icp_batch_diag",
    "gorio_apd_set_ndt_cuda_params", "gorio_apd_get_ndt_cuda_params", "gorio_apd_ndt_cuda_get_voxels", "gorio_apd_ndt_cuda_get_pairs",
    "gorio_apd_set_vgicp_cuda_params", "gorio_apd_get_vgicp_cuda_params", "gorio_apd_vgicp_cuda_get_points", "gorio_apd_vgicp_cuda_get_voxels", "gorio_apd_vgicp_cuda_get_pairs",
    "gorio_apd_set_gicp_mp_params", "gorio_apd_get_gicp_mp_params", "gorio_apd_gicp_mp_get_covariances", "gorio_apd_gicp_mp_pass", "gorio_apd_gicp_mp_get_neighbors", "gorio_apd_gicp_mp_get_merged",
    "gorio_apd_gicp_mp_diag", "gorio_apd_gicp_mp_align_batch", "gorio_apd_gicp_mp_batch_diag", "gorio_apd_gicp_mp_last_hessian",
    "gorio_apd_set_submap_downsample", "gorio_apd_get_submap_downsample",
]

# gorio_method / gorio_voxel_search / gorio_voxel_mode of gorio_apd.h (the latter two in the order of gicp_settings.hpp)
METHOD_APDGICP, METHOD_GICP, METHOD_VGICP, METHOD_GICP_OMP, METHOD_ICP = 0, 1, 2, 3, 4
METHOD_NDT_CUDA = 5  # gorio_method_fast_ndt: fast_gicp::NDTCuda
NDT_CUDA_P2D, NDT_CUDA_D2D = 0, 1  # gorio_ndt_cuda_distance (ndt_settings.hpp:6)
METHOD_VGICP_CUDA = 6  # gorio_method_fast_vgicp_cuda: fast_gicp::FastVGICPCuda
NN_CPU_PARALLEL_KDTREE, NN_GPU_BRUTEFORCE, NN_GPU_RBF_KERNEL = 0, 1, 2  # gorio_vgicp_cuda_nn (fast_vgicp_cuda.hpp:21)
METHOD_GICP_MP = 8  # gorio_method_fast_gicp_mp: fast_gicp::FastGICPMultiPoints (7 stays unused and refused)
GICP_OMP_F, GICP_OMP_DF, GICP_OMP_FDF = 0, 1, 2  # modes of gorio_apd_gicp_omp_evaluate
VOXEL_DIRECT27, VOXEL_DIRECT7, VOXEL_DIRECT1, VOXEL_DIRECT_RADIUS = 0, 1, 2, 3
VOXEL_ADDITIVE, VOXEL_ADDITIVE_WEIGHTED, VOXEL_MULTIPLICATIVE = 0, 1, 2
DOWNSAMPLE_VOXELGRID, DOWNSAMPLE_APPROX_VOXELGRID = 0, 1  # gorio_downsample_method: what a submap call's voxel_leaf > 0 runs
VOXEL_OFFSETS = {VOXEL_DIRECT27: 27, VOXEL_DIRECT7: 7, VOXEL_DIRECT1: 1}

_lib = None


def load_library():
    """dlopen go-rio_amd/lib/libgorio_amd.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        from . import LIB_PATH

        if not os.path.exists(LIB_PATH):
            raise GorioError(-2, f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        _lib = C.CDLL(LIB_PATH)
        _lib.gorio_apd_last_error.restype = C.c_char_p
    return _lib


def _p(a, t):
    """Typed pointer to a contiguous array without going through ndarray.ctypes (slow once torch is imported)."""
    return C.cast(a.__array_interface__["data"][0], C.POINTER(t))


def _check(h, rc):
    if rc < 0:
        msg = load_library().gorio_apd_last_error(h)
        raise GorioError(rc, msg.decode() if msg else "")
    return rc


class ApdGicp:
    """One fast_gicp::FastAPDGICP object living on one GPU."""

    def __init__(self, device=0, **params):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.gorio_apd_create(C.byref(self._h), int(device))
        if rc != 0:
            raise GorioError(rc, "gorio_apd_create failed (no usable HIP device?)")
        self.params = ApdParams()
        self._lib.gorio_apd_default_params(C.byref(self.params))
        self._n_src = self._n_tgt = 0
        if params:
            self.set_params(**params)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self._lib.gorio_apd_destroy(h)
            self._h = None

    # ---- setters of fast_apdgicp.hpp:48-58, lsq_registration.hpp:51-53 and the pcl::Registration setters (registrations.cpp:41-48)
    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)
        _check(self._h, self._lib.gorio_apd_set_params(self._h, C.byref(self.params)))

    # ---- which fast_gicp class the object stands for (gorio_apd_set_method): FastAPDGICP, FastGICP or FastVGICP with its
    # setResolution / setNeighborSearchMethod / setVoxelAccumulationMode (fast_vgicp.hpp:55-62)
    def set_method(self, method, voxel_resolution=1.0, voxel_search=VOXEL_DIRECT1, voxel_mode=VOXEL_ADDITIVE):
        _check(self._h, self._lib.gorio_apd_set_method(self._h, int(method), C.c_double(voxel_resolution), int(voxel_search), int(voxel_mode)))

    def get_method(self):
        m, s, a, r = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_get_method(self._h, C.byref(m), C.byref(r), C.byref(s), C.byref(a)))
        return dict(method=m.value, voxel_resolution=r.value, voxel_search=s.value, voxel_mode=a.value)

    # ---- GICP_OMP (METHOD_GICP_OMP): gicp_epsilon_ / setMaximumOptimizerIterations (gicp_omp.h:117-121, 255-260) and the three parity hooks
    def setGicpOmpParams(self, gicp_epsilon=0.001, max_optimizer_iterations=20):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_set_gicp_omp_params(self._h, C.c_double(gicp_epsilon), int(max_optimizer_iterations)))

    def getGicpOmpParams(self):  # noqa: N802
        e, m = C.c_double(0.0), C.c_int(0)
        _check(self._h, self._lib.gorio_apd_get_gicp_omp_params(self._h, C.byref(e), C.byref(m)))
        return e.value, m.value

    def setMaximumOptimizerIterations(self, n):  # noqa: N802
        self.setGicpOmpParams(self.getGicpOmpParams()[0], int(n))

    def gicpOmpUpdate(self, transformation, guess=None):  # noqa: N802 -- one pass of gicp_omp_impl.hpp:411-476; returns the number of pairs
        t = np.ascontiguousarray(transformation, np.float32)
        g = np.ascontiguousarray(np.eye(4) if guess is None else guess, np.float32)
        m = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_gicp_omp_update(self._h, _p(t, C.c_float), _p(g, C.c_float), C.byref(m)))
        return m.value

    def gicpOmpEvaluate(self, x, mode=GICP_OMP_FDF):  # noqa: N802 -- the functor at x over the pairs held: (f or None, g or None)
        x = np.ascontiguousarray(x, np.float64)
        f, g = C.c_double(0.0), np.zeros(6, np.float64)
        _check(self._h, self._lib.gorio_apd_gicp_omp_evaluate(self._h, _p(x, C.c_double), int(mode), C.byref(f), _p(g, C.c_double)))
        return (None if mode == GICP_OMP_DF else f.value), (None if mode == GICP_OMP_F else g)

    def gicpOmpDiag(self):  # noqa: N802
        o, i, e, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self._h, self._lib.gorio_apd_gicp_omp_diag(self._h, C.byref(o), C.byref(i), C.byref(e), C.byref(s)))
        return dict(outer=o.value, inner_total=i.value, evaluations=e.value, last_status=s.value)

    # ---- ICP (METHOD_ICP): the setters of pcl::IterativeClosestPoint that gorio_apd_params does not carry, and the parity hooks
    def set_icp_params(self, use_reciprocal=False, euclidean_fitness_epsilon=-np.finfo(np.float64).max, transformation_rotation_epsilon=0.0):
        _check(self._h, self._lib.gorio_apd_set_icp_params(self._h, int(bool(use_reciprocal)), C.c_double(euclidean_fitness_epsilon), C.c_double(transformation_rotation_epsilon)))

    def get_icp_params(self):
        r, f, t = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_get_icp_params(self._h, C.byref(r), C.byref(f), C.byref(t)))
        return dict(use_reciprocal=bool(r.value), euclidean_fitness_epsilon=f.value, transformation_rotation_epsilon=t.value)

    def icp_step(self, T=None):
        """gorio_apd_icp_step: one correspondence pass on T * source -> dict(pairs, sums [17], T_est [4, 4]); getCorrespondences() gives the pairs."""
        T = np.ascontiguousarray(np.eye(4) if T is None else T, np.float32)
        m, sums, est = C.c_int(0), np.zeros(17, np.float64), np.zeros((4, 4), np.float32)
        _check(self._h, self._lib.gorio_apd_icp_step(self._h, _p(T, C.c_float), C.byref(m), _p(sums, C.c_double), _p(est, C.c_float)))
        return dict(pairs=m.value, sums=sums, T_est=est)

    def icp_diag(self):
        """gorio_apd_icp_diag of the last align: iterations, ConvergenceState, mean squared pair distance, pairs of the last pass."""
        i, s, p, e = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_icp_diag(self._h, C.byref(i), C.byref(s), C.byref(e), C.byref(p)))
        return dict(iterations=i.value, state=s.value, mse=e.value, pairs=p.value)

    # ---- NDTCuda (METHOD_NDT_CUDA): setDistanceMode and the radius of setNeighborSearchMethod (ndt_cuda.hpp:53-55), and the parity hooks
    def set_ndt_cuda_params(self, distance_mode=NDT_CUDA_D2D, radius=-1.0):
        _check(self._h, self._lib.gorio_apd_set_ndt_cuda_params(self._h, int(distance_mode), C.c_double(radius)))

    def get_ndt_cuda_params(self):
        m, r = C.c_int(0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_get_ndt_cuda_params(self._h, C.byref(m), C.byref(r)))
        return dict(distance_mode=m.value, radius=r.value)

    def ndt_cuda_voxels(self, which):
        """gorio_apd_ndt_cuda_get_voxels: the float voxel map of the source (0) / target (1), voxels in ascending (x, y, z) coordinate order."""
        nv = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_ndt_cuda_get_voxels(self._h, int(which), 0, C.byref(nv), None, None, None, None, None))
        n = nv.value
        coord, num = np.empty((n, 3), np.int32), np.empty(n, np.int32)
        mean, raw, cov = np.empty((n, 3), np.float32), np.empty((n, 3, 3), np.float32), np.empty((n, 3, 3), np.float32)
        if n:
            _check(self._h, self._lib.gorio_apd_ndt_cuda_get_voxels(self._h, int(which), n, C.byref(nv), _p(coord, C.c_int), _p(num, C.c_int), _p(mean, C.c_float),
                                                                     _p(raw, C.c_float), _p(cov, C.c_float)))
        return dict(coord=coord, num_points=num, mean=mean, cov_raw=raw, cov=cov)

    def ndt_cuda_pairs(self):
        """gorio_apd_ndt_cuda_get_pairs: the (item, voxel) pairs of the last linearise, offset-major then item order, as an [n, 2] array."""
        m = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_ndt_cuda_get_pairs(self._h, 0, C.byref(m), None, None))
        item, vox = np.empty(m.value, np.int32), np.empty(m.value, np.int32)
        if m.value:
            _check(self._h, self._lib.gorio_apd_ndt_cuda_get_pairs(self._h, m.value, C.byref(m), _p(item, C.c_int), _p(vox, C.c_int)))
        return np.stack([item, vox], axis=1)

    # ---- FastVGICPCuda (METHOD_VGICP_CUDA): setNearestNeighborSearchMethod and setKernelWidth (fast_vgicp_cuda.hpp:55-59), and the parity hooks
    def set_vgicp_cuda_params(self, nn_method=NN_CPU_PARALLEL_KDTREE, kernel_width=0.5, kernel_max_dist=3.0):
        _check(self._h, self._lib.gorio_apd_set_vgicp_cuda_params(self._h, int(nn_method), C.c_double(kernel_width), C.c_double(kernel_max_dist)))

    def get_vgicp_cuda_params(self):
        m, w, d = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_get_vgicp_cuda_params(self._h, C.byref(m), C.byref(w), C.byref(d)))
        return dict(nn_method=m.value, kernel_width=w.value, kernel_max_dist=d.value)

    def vgicp_cuda_points(self, which):
        """gorio_apd_vgicp_cuda_get_points: of the source (0) / target (1) the raw covariance of every point, the input indices of the
        points the regularisation keeps, and their regularised covariances (six floats each: 00 01 02 11 12 22)."""
        n, nk = C.c_int(0), C.c_int(0)
        _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_points(self._h, int(which), 0, C.byref(n), None, C.byref(nk), None, None))
        raw, idx, cov = np.empty((n.value, 6), np.float32), np.empty(nk.value, np.int32), np.empty((nk.value, 6), np.float32)
        if n.value:
            _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_points(self._h, int(which), n.value, C.byref(n), _p(raw, C.c_float), C.byref(nk), _p(idx, C.c_int), _p(cov, C.c_float)))
        return dict(cov_raw=raw, kept_index=idx, cov=cov)

    def vgicp_cuda_voxels(self):
        """gorio_apd_vgicp_cuda_get_voxels: the voxel map of the kept target points, voxels in ascending (x, y, z) coordinate order."""
        nv = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_voxels(self._h, 0, C.byref(nv), None, None, None, None))
        n = nv.value
        coord, num, mean, cov = np.empty((n, 3), np.int32), np.empty(n, np.int32), np.empty((n, 3), np.float32), np.empty((n, 6), np.float32)
        if n:
            _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_voxels(self._h, n, C.byref(nv), _p(coord, C.c_int), _p(num, C.c_int), _p(mean, C.c_float), _p(cov, C.c_float)))
        return dict(coord=coord, num_points=num, mean=mean, cov=cov)

    def vgicp_cuda_pairs(self):
        """gorio_apd_vgicp_cuda_get_pairs: the (kept item, voxel) pairs of the last linearise, offset-major then item order, as an [n, 2] array."""
        m = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_pairs(self._h, 0, C.byref(m), None, None))
        item, vox = np.empty(m.value, np.int32), np.empty(m.value, np.int32)
        if m.value:
            _check(self._h, self._lib.gorio_apd_vgicp_cuda_get_pairs(self._h, m.value, C.byref(m), _p(item, C.c_int), _p(vox, C.c_int)))
        return np.stack([item, vox], axis=1)

    # ---- FastGICPMultiPoints (METHOD_GICP_MP): neighbor_search_radius_ (fast_gicp_mp_impl.hpp:35; the reference has no setter) and the parity hooks
    def set_gicp_mp_params(self, neighbor_search_radius=0.5):
        _check(self._h, self._lib.gorio_apd_set_gicp_mp_params(self._h, C.c_double(neighbor_search_radius)))

    def get_gicp_mp_params(self):
        r = C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_get_gicp_mp_params(self._h, C.byref(r)))
        return dict(neighbor_search_radius=r.value)

    def gicp_mp_covariances(self, which):
        """gorio_apd_gicp_mp_get_covariances: the float covariances of the source (0) / target (1), six floats per point (00 01 02 11 12 22)."""
        n = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_gicp_mp_get_covariances(self._h, int(which), 0, C.byref(n), None))
        cov = np.empty((n.value, 6), np.float32)
        if n.value:
            _check(self._h, self._lib.gorio_apd_gicp_mp_get_covariances(self._h, int(which), n.value, C.byref(n), _p(cov, C.c_float)))
        return cov

    def gicp_mp_pass(self, T=None):
        """gorio_apd_gicp_mp_pass: one pass (neighbourhoods, merge, linearisation) at the float pose T -> dict(used, total, H [6, 6], g [6])."""
        T = np.ascontiguousarray(np.eye(4) if T is None else T, np.float32)
        used, total = C.c_int(0), C.c_longlong(0)
        H, g = np.zeros((6, 6), np.float64), np.zeros(6, np.float64)
        _check(self._h, self._lib.gorio_apd_gicp_mp_pass(self._h, _p(T, C.c_float), C.byref(used), C.byref(total), _p(H, C.c_double), _p(g, C.c_double)))
        return dict(used=used.value, total=total.value, H=H, g=g)

    def gicp_mp_neighbors(self):
        """gorio_apd_gicp_mp_get_neighbors: the CSR of the last pass -> (offsets [n + 1] int64, idx [total] int32, sqd [total] float32)."""
        nq, total = C.c_int(0), C.c_longlong(0)
        _check(self._h, self._lib.gorio_apd_gicp_mp_get_neighbors(self._h, C.c_longlong(-1), C.byref(nq), C.byref(total), None, None, None))
        offs, idx, sqd = np.zeros(nq.value + 1, np.int64), np.empty(total.value, np.int32), np.empty(total.value, np.float32)
        _check(self._h, self._lib.gorio_apd_gicp_mp_get_neighbors(self._h, C.c_longlong(total.value), C.byref(nq), C.byref(total), _p(offs, C.c_longlong), _p(idx, C.c_int), _p(sqd, C.c_float)))
        return offs, idx, sqd

    def gicp_mp_merged(self):
        """gorio_apd_gicp_mp_get_merged: of the last gicp_mp_pass per source point mean_B [n, 3], cov_B [n, 6] and the used flag [n]."""
        n = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_gicp_mp_get_merged(self._h, 0, C.byref(n), None, None, None))
        mean, cov, used = np.empty((n.value, 3), np.float32), np.empty((n.value, 6), np.float32), np.empty(n.value, np.int32)
        if n.value:
            _check(self._h, self._lib.gorio_apd_gicp_mp_get_merged(self._h, n.value, C.byref(n), _p(mean, C.c_float), _p(cov, C.c_float), _p(used, C.c_int)))
        return dict(mean_B=mean, cov_B=cov, used=used.astype(bool))

    def gicp_mp_diag(self):
        p, u, t = C.c_int(0), C.c_int(0), C.c_longlong(0)
        s = (C.c_double * 4)()
        _check(self._h, self._lib.gorio_apd_gicp_mp_diag(self._h, C.byref(p), C.byref(u), C.byref(t), s))
        return dict(passes=p.value, used=u.value, total=t.value, stage_seconds=dict(zip(("query", "search", "linearize", "shell"), list(s))))

    def getVoxelMap(self):  # noqa: N802 -- parity hook: voxelmap_ (fast_vgicp.hpp:85), voxels in ascending (x, y, z) coordinate order
        nv = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_get_voxelmap(self._h, None, None, None, None, 0, C.byref(nv)))
        n = nv.value
        coord = np.empty((n, 3), np.int32)
        num = np.empty(n, np.int32)
        mean = np.empty((n, 4), np.float64)
        cov = np.empty((n, 4, 4), np.float64)
        _check(self._h, self._lib.gorio_apd_get_voxelmap(self._h, _p(coord, C.c_int), _p(num, C.c_int), _p(mean, C.c_double), _p(cov, C.c_double), n, C.byref(nv)))
        return dict(coord=coord, num_points=num, mean=mean, cov=cov)

    def getVoxelCorrespondences(self):  # noqa: N802 -- parity hook: voxel_correspondences_ as the table [n_source][n_offsets], -1 = no voxel
        n_off = VOXEL_OFFSETS[self.get_method()["voxel_search"]]
        idx = np.empty((self._n_src, n_off), np.int32)
        _check(self._h, self._lib.gorio_apd_get_voxel_correspondences(self._h, _p(idx, C.c_int), self._n_src * n_off))
        return idx

    def setNumThreads(self, n):  # noqa: N802 -- no-op on the GPU (APD:34-42)
        pass

    def setCorrespondenceRandomness(self, k):  # noqa: N802
        self.set_params(k_correspondences=int(k))

    def setRegularizationMethod(self, method):  # noqa: N802
        self.set_params(regularization=int(method))

    def setAzimuthVar(self, v):  # noqa: N802
        self.set_params(azimuth_var=float(v))

    def setElevationVar(self, v):  # noqa: N802
        self.set_params(elevation_var=float(v))

    def setDistVar(self, v):  # noqa: N802
        self.set_params(dist_var=float(v))

    def setTransformationEpsilon(self, v):  # noqa: N802
        self.set_params(transformation_epsilon=float(v))

    def setRotationEpsilon(self, v):  # noqa: N802
        self.set_params(rotation_epsilon=float(v))

    def setMaximumIterations(self, v):  # noqa: N802
        self.set_params(max_iterations=int(v))

    def setMaxCorrespondenceDistance(self, v):  # noqa: N802
        self.set_params(corr_dist_threshold=float(v))

    def setInitialLambdaFactor(self, v):  # noqa: N802
        self.set_params(lm_init_lambda_factor=float(v))

    # ---- clouds
    @staticmethod
    def _cloud_args(xyz, label):
        xyz = np.ascontiguousarray(xyz, np.float32)
        if xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("xyz must be [n, 3]")
        lab = None if label is None else np.ascontiguousarray(label, np.float32)
        return xyz, lab

    def setInputSource(self, xyz, label=None):  # noqa: N802
        xyz, lab = self._cloud_args(xyz, label)
        # labels are packed with their own 4-byte stride: pass a [n,4] interleaved buffer so one stride serves both
        buf = np.empty((xyz.shape[0], 4), np.float32)
        buf[:, :3] = xyz
        buf[:, 3] = 0.0 if lab is None else lab
        _check(self._h, self._lib.gorio_apd_set_source(self._h, _p(buf, C.c_float), _p(buf[:, 3:], C.c_float) if lab is not None else None, buf.shape[0], 16))
        self._n_src = buf.shape[0]

    def setInputTarget(self, xyz, label=None):  # noqa: N802
        xyz, lab = self._cloud_args(xyz, label)
        buf = np.empty((xyz.shape[0], 4), np.float32)
        buf[:, :3] = xyz
        buf[:, 3] = 0.0 if lab is None else lab
        _check(self._h, self._lib.gorio_apd_set_target(self._h, _p(buf, C.c_float), _p(buf[:, 3:], C.c_float) if lab is not None else None, buf.shape[0], 16))
        self._n_tgt = buf.shape[0]

    def setInputSourcePcl(self, points):  # noqa: N802
        """points: [n, 12] float32 laid out as pcl::PointXYZINormal (48 bytes: x y z 1 | normal_x normal_y normal_z 0 | intensity curvature - -):
        exactly the pointers and stride the C++ drop-in passes (&pts[0].x, &pts[0].normal_x, sizeof(PointT)); no repacking on the way."""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 12:
            raise ValueError("points must be [n, 12] float32 (PointXYZINormal)")
        _check(self._h, self._lib.gorio_apd_set_source(self._h, _p(pts, C.c_float), _p(pts[:, 4:], C.c_float), pts.shape[0], 48))
        self._n_src = pts.shape[0]

    def setInputTargetPcl(self, points):  # noqa: N802
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 12:
            raise ValueError("points must be [n, 12] float32 (PointXYZINormal)")
        _check(self._h, self._lib.gorio_apd_set_target(self._h, _p(pts, C.c_float), _p(pts[:, 4:], C.c_float), pts.shape[0], 48))
        self._n_tgt = pts.shape[0]

    def setInputSourceDevice(self, d_x, d_y, d_z, d_label, n):  # noqa: N802 -- raw device pointers (ints)
        _check(self._h, self._lib.gorio_apd_set_source_device(self._h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(d_z), C.c_void_p(d_label or 0), int(n)))
        self._n_src = int(n)

    def setInputTargetDevice(self, d_x, d_y, d_z, d_label, n):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_set_target_device(self._h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(d_z), C.c_void_p(d_label or 0), int(n)))
        self._n_tgt = int(n)

    def setInputSourceFromScan(self, scan):  # noqa: N802 -- gorio_apd_set_source_from_scan: the output of a prep.ScanPipeline, no host round trip
        _check(self._h, self._lib.gorio_apd_set_source_from_scan(self._h, scan.h))
        self._n_src = scan.last_result["n_out"]

    def setInputTargetFromScan(self, scan):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_set_target_from_scan(self._h, scan.h))
        self._n_tgt = scan.last_result["n_out"]

    def setInputTargetShared(self, owner):  # noqa: N802 -- gorio_apd_set_target_shared: one device copy of the map for many objects
        _check(self._h, self._lib.gorio_apd_set_target_shared(self._h, owner._h))
        self._n_tgt = owner._n_tgt

    def setInputTargetSubmap(self, frames, rel_poses, voxel_leaf=0.0):  # noqa: N802
        """gorio_apd_set_target_submap: frames = list of (xyz [n,3], label [n] or None), rel_poses = list of 4x4 (odom_i^-1 odom_newest)."""
        n = len(frames)
        arr = (Keyframe * n)()
        keep = []
        for i, ((xyz, lab), T) in enumerate(zip(frames, rel_poses)):
            xyz, lab = self._cloud_args(xyz, lab)
            buf = np.empty((xyz.shape[0], 4), np.float32)
            buf[:, :3] = xyz
            buf[:, 3] = 0.0 if lab is None else lab
            Td = np.ascontiguousarray(T, np.float64)
            keep += [buf, Td]
            arr[i].xyz = buf.__array_interface__["data"][0]
            arr[i].label = buf.__array_interface__["data"][0] + 12
            arr[i].n, arr[i].point_stride_bytes = buf.shape[0], 16
            arr[i].rel_pose = Td.__array_interface__["data"][0]
        cnt = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_set_target_submap(self._h, arr, n, C.c_double(voxel_leaf), C.byref(cnt)))
        self._n_tgt = cnt.value
        return cnt.value

    def setInputSourceKeyframe(self, store, kid):  # noqa: N802 -- gorio_apd_set_source_from_keyframe: a keyframes.KeyframeStore entry, shared
        _check(self._h, self._lib.gorio_apd_set_source_from_keyframe(self._h, store.h, int(kid)))
        self._n_src = store.info(kid)["n"]

    def setInputTargetKeyframe(self, store, kid):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_set_target_from_keyframe(self._h, store.h, int(kid)))
        self._n_tgt = store.info(kid)["n"]

    def setInputTargetSubmapKeyframes(self, store, ids, rel_poses, voxel_leaf=0.0):  # noqa: N802
        """gorio_apd_set_target_submap_keyframes: setInputTargetSubmap from keyframes resident in a keyframes.KeyframeStore."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        T = np.ascontiguousarray(rel_poses, np.float64).reshape(-1, 16)
        if T.shape[0] != ids.shape[0]:
            raise ValueError("one 4x4 pose per keyframe id")
        cnt = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_set_target_submap_keyframes(self._h, store.h, _p(ids, C.c_int) if ids.size else None, _p(T, C.c_double) if ids.size else None,
                                                                          int(ids.shape[0]), C.c_double(voxel_leaf), C.byref(cnt)))
        self._n_tgt = cnt.value
        return cnt.value

    def setSubmapDownsample(self, method):  # noqa: N802 -- gorio_apd_set_submap_downsample: DOWNSAMPLE_VOXELGRID (default) or DOWNSAMPLE_APPROX_VOXELGRID
        _check(self._h, self._lib.gorio_apd_set_submap_downsample(self._h, int(method)))

    def getSubmapDownsample(self):  # noqa: N802
        m = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_get_submap_downsample(self._h, C.byref(m)))
        return m.value

    def getTargetPoints(self):  # noqa: N802
        buf = np.empty((self._n_tgt, 4), np.float32)
        _check(self._h, self._lib.gorio_apd_get_target_points(self._h, _p(buf, C.c_float), _p(buf[:, 3:], C.c_float), self._n_tgt, 16))
        return buf[:, :3].copy(), buf[:, 3].copy()

    # ---- sharded-source mode (RCCL): see include/gorio_apd.h
    @staticmethod
    def commUniqueId():  # noqa: N802
        buf = C.create_string_buffer(128)
        rc = load_library().gorio_comm_get_unique_id(buf)
        if rc != 0:
            raise GorioError(rc, "gorio_comm_get_unique_id failed (librccl missing?)")
        return buf.raw

    def commInit(self, world_size, rank, unique_id):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_comm_init(self._h, int(world_size), int(rank), C.c_char_p(bytes(unique_id))))

    def commInfo(self):  # noqa: N802 -- (world size, rank) as RCCL reports them, ncclAllReduce calls enqueued so far
        w, r, c = C.c_int(0), C.c_int(0), C.c_longlong(0)
        _check(self._h, self._lib.gorio_apd_comm_info(self._h, C.byref(w), C.byref(r), C.byref(c)))
        return w.value, r.value, c.value

    def debugSetShard(self, world_size, rank):  # noqa: N802 -- test hook: the partition of a rank without the collectives
        _check(self._h, self._lib.gorio_apd_debug_set_shard(self._h, int(world_size), int(rank)))

    def debugSetSchedule(self, fuse_step=True, plan_search=True):  # noqa: N802 -- test hook: the two schedule optimisations of a GN align
        _check(self._h, self._lib.gorio_apd_debug_set_schedule(self._h, int(bool(fuse_step)), int(bool(plan_search))))

    def commDestroy(self):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_comm_destroy(self._h))

    def clearSource(self):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_clear_source(self._h))
        self._n_src = 0

    def clearTarget(self):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_clear_target(self._h))
        self._n_tgt = 0

    def swapSourceAndTarget(self):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_swap_source_and_target(self._h))
        self._n_src, self._n_tgt = self._n_tgt, self._n_src

    # ---- covariances
    def setSourceCovariances(self, cov):  # noqa: N802
        cov = np.ascontiguousarray(cov, np.float64).reshape(-1, 16)
        _check(self._h, self._lib.gorio_apd_set_source_covariances(self._h, _p(cov, C.c_double), cov.shape[0]))

    def setTargetCovariances(self, cov):  # noqa: N802
        cov = np.ascontiguousarray(cov, np.float64).reshape(-1, 16)
        _check(self._h, self._lib.gorio_apd_set_target_covariances(self._h, _p(cov, C.c_double), cov.shape[0]))

    def _get_covs(self, fn, n):
        cnt = _check(self._h, fn(self._h, None, 0))
        out = np.zeros((cnt, 4, 4), np.float64)
        if cnt:
            _check(self._h, fn(self._h, _p(out, C.c_double), cnt))
        return out

    def getSourceCovariances(self):  # noqa: N802
        return self._get_covs(self._lib.gorio_apd_get_source_covariances, self._n_src)

    def getTargetCovariances(self):  # noqa: N802
        return self._get_covs(self._lib.gorio_apd_get_target_covariances, self._n_tgt)

    def calculateCovariances(self):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_calculate_covariances(self._h))

    def debugKnnRedoGroups(self):  # noqa: N802 -- test hook: 64-point groups the redo pass of the last k-NN covariance estimation did
        groups = C.c_int(0)
        _check(self._h, self._lib.gorio_apd_debug_knn_redo_groups(self._h, C.byref(groups)))
        return groups.value

    def debugGetIndex(self, which):  # noqa: N802 -- test hook: the search index of the source (0) / target (1) as the pruned searches see it
        sizes = (C.c_int * 6)()
        _check(self._h, self._lib.gorio_apd_debug_get_index(self._h, int(which), sizes, None, None, None, None, None))
        n, n_spad, n_tiles, n_super, n_blk, chunk = list(sizes)
        sxyz = np.empty(7 * n_spad, np.float32)
        orig = np.empty(n_spad, np.int32)
        tbox, sbox, bbox = (np.empty((m, 8), np.float32) for m in (n_tiles, n_super, n_blk))
        _check(self._h, self._lib.gorio_apd_debug_get_index(self._h, int(which), sizes, _p(sxyz, C.c_float), _p(orig, C.c_int), _p(tbox, C.c_float), _p(sbox, C.c_float), _p(bbox, C.c_float)))
        return dict(n=n, n_spad=n_spad, kd_chunk=chunk, sx=sxyz[:n_spad], sy=sxyz[n_spad : 2 * n_spad], sz=sxyz[2 * n_spad : 3 * n_spad],
                    s4=sxyz[3 * n_spad :].reshape(n_spad, 4), orig=orig, tbox=tbox, sbox=sbox, bbox=bbox)

    def getKnnIndices(self, which):  # noqa: N802
        n = self._n_src if which == 0 else self._n_tgt
        k = self.params.k_correspondences
        idx = np.empty((n, k), np.int32)
        _check(self._h, self._lib.gorio_apd_get_knn_indices(self._h, int(which), _p(idx, C.c_int), n * k))
        return idx

    # ---- registration
    def align(self, guess=None):
        """pcl::Registration::align(output, guess) minus the output cloud; returns a dict like oracle.apd.align."""
        g = np.ascontiguousarray(np.eye(4) if guess is None else guess, np.float32)
        T = np.zeros((4, 4), np.float32)
        H = np.zeros((6, 6), np.float64)
        conv, nit, nlin = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self._h, self._lib.gorio_apd_align(self._h, _p(g, C.c_float), _p(T, C.c_float), _p(H, C.c_double), C.byref(conv), C.byref(nit), C.byref(nlin)))
        self._final = T
        self._converged = bool(conv.value)
        return dict(T=T, H=H, converged=bool(conv.value), nr_iterations=nit.value, n_linearize=nlin.value)

    def hasConverged(self):  # noqa: N802
        return self._converged

    def getFinalTransformation(self):  # noqa: N802
        return self._final

    def linearize(self, T):
        T = np.ascontiguousarray(T, np.float64)
        H = np.zeros((6, 6), np.float64)
        b = np.zeros(6, np.float64)
        err = C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_linearize(self._h, _p(T, C.c_double), _p(H, C.c_double), _p(b, C.c_double), C.byref(err)))
        return err.value, H, b

    def evaluateCost(self, relative_pose):  # noqa: N802 -- lsq_registration_impl.hpp:50-52
        return self.linearize(np.asarray(relative_pose, np.float32).astype(np.float64))

    def compute_error(self, T):
        T = np.ascontiguousarray(T, np.float64)
        err = C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_compute_error(self._h, _p(T, C.c_double), C.byref(err)))
        return err.value

    def getCorrespondences(self):  # noqa: N802
        corr = np.empty(self._n_src, np.int32)
        sqd = np.empty(self._n_src, np.float32)
        _check(self._h, self._lib.gorio_apd_get_correspondences(self._h, _p(corr, C.c_int), _p(sqd, C.c_float), self._n_src))
        return corr, sqd

    def getMahalanobis(self):  # noqa: N802
        m = np.empty((self._n_src, 4, 4), np.float64)
        _check(self._h, self._lib.gorio_apd_get_mahalanobis(self._h, _p(m, C.c_double), self._n_src))
        return m

    def transformSource(self, T):  # noqa: N802
        T = np.ascontiguousarray(T, np.float32)
        out = np.empty((self._n_src, 3), np.float32)
        _check(self._h, self._lib.gorio_apd_transform_source(self._h, _p(T, C.c_float), _p(out, C.c_float), self._n_src, 12))
        return out

    def getFitnessScore(self, T=None, max_range=np.finfo(np.float64).max, inlier_dist=0.5):  # noqa: N802
        """(pcl getFitnessScore(max_range), inlier fraction of scan_matching_odometry_nodelet.cpp:677-689 with its 0.5 m bound)."""
        T = np.ascontiguousarray(self._final if T is None else T, np.float32)
        score, inl = C.c_double(0.0), C.c_double(0.0)
        _check(self._h, self._lib.gorio_apd_fitness_score(self._h, _p(T, C.c_float), C.c_double(max_range), C.c_double(inlier_dist), C.byref(score), C.byref(inl)))
        return score.value, inl.value

    def setProfiling(self, on):  # noqa: N802
        _check(self._h, self._lib.gorio_apd_set_profiling(self._h, int(bool(on))))

    def getStageTimes(self):  # noqa: N802
        s = (C.c_double * 8)()
        c = (C.c_int * 8)()
        _check(self._h, self._lib.gorio_apd_get_stage_times(self._h, s, c))
        return list(s), list(c)


class Keyframe(C.Structure):
    """gorio_apd_keyframe (include/gorio_apd.h)."""
    _fields_ = [("xyz", C.c_void_p), ("label", C.c_void_p), ("n", C.c_int), ("point_stride_bytes", C.c_int), ("rel_pose", C.c_void_p)]


class DeviceCloud(C.Structure):
    """gorio_apd_device_cloud (include/gorio_apd.h)."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("label", C.c_void_p), ("n", C.c_int)]


class DeviceInputs:
    """Descriptor arrays for gorio_apd_set_clouds_device_batch, built once for a list of objects whose inputs live in
    device-resident SoA buffers: sources / targets = lists of ((x, y, z, label) device addresses, n) per object, or None."""

    def __init__(self, objs, sources=None, targets=None):
        self.objs = list(objs)
        n = len(self.objs)
        self.handles = (C.c_void_p * n)(*[o._h for o in self.objs])

        def pack(lst):
            if lst is None:
                return None
            arr = (DeviceCloud * n)()
            for i, (ptrs, cnt) in enumerate(lst):
                arr[i].x, arr[i].y, arr[i].z = ptrs[0], ptrs[1], ptrs[2]
                arr[i].label = ptrs[3] if len(ptrs) > 3 and ptrs[3] else None
                arr[i].n = int(cnt)
            return arr
        self.src, self.tgt = pack(sources), pack(targets)
        self._ns = None if sources is None else [int(c) for _, c in sources]
        self._nt = None if targets is None else [int(c) for _, c in targets]

    def apply(self):
        """setInputSource / setInputTarget of every object from its device buffers: one C call, one copy launch."""
        lib = load_library()
        rc = lib.gorio_apd_set_clouds_device_batch(self.handles, len(self.objs), self.src, self.tgt)
        _check(self.objs[0]._h, rc)
        for i, o in enumerate(self.objs):
            if self._ns is not None:
                o._n_src = self._ns[i]
            if self._nt is not None:
                o._n_tgt = self._nt[i]


def _run_align_batch(objs, guesses, call):
    """What the batched aligns share: the guesses (identity by default), the result arrays and the handle array.  call(handles, n, g, T,
    conv, nit) makes the C call; its code is checked against objs[0].  Stores every object's _final / _converged, returns (T, conv, nit)."""
    n = len(objs)
    g = np.ascontiguousarray(np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)) if guesses is None else guesses, np.float32).reshape(n, 16)
    T = np.zeros((n, 4, 4), np.float32)
    conv = np.zeros(n, np.int32)
    nit = np.zeros(n, np.int32)
    arr = (C.c_void_p * n)(*[o._h for o in objs])
    _check(objs[0]._h, call(arr, n, _p(g, C.c_float), _p(T, C.c_float), _p(conv, C.c_int), _p(nit, C.c_int)))
    for q, o in enumerate(objs):
        o._final = T[q]
        o._converged = bool(conv[q])
    return T, conv, nit


def _batch_diag(fn, lead, names):
    vals = [C.c_int(0) for _ in names]
    _check(lead._h, fn(lead._h, *[C.byref(v) for v in vals]))
    return {k: v.value for k, v in zip(names, vals)}


def align_batch(objs, guesses=None):
    """gorio_apd_align_batch over a list of ApdGicp objects (all on one device).  Returns a list of result dicts."""
    lib = load_library()
    n = len(objs)
    H = np.zeros((n, 6, 6), np.float64)
    nlin = np.zeros(n, np.int32)
    T, conv, nit = _run_align_batch(objs, guesses, lambda arr, n, g, T, conv, nit: lib.gorio_apd_align_batch(arr, n, g, T, _p(H, C.c_double), conv, nit, _p(nlin, C.c_int)))
    return [dict(T=T[q], H=H[q], converged=bool(conv[q]), nr_iterations=int(nit[q]), n_linearize=int(nlin[q])) for q in range(n)]


def gicp_omp_align_batch(objs, guesses=None):
    """gorio_apd_gicp_omp_align_batch over a list of ApdGicp objects in GICP_OMP mode (all on one device): their aligns in lock-step
    rounds, every result bit for bit the one of the object's own align().  Returns the list of dicts align() returns, each with
    batch_diag = dict(rounds, launches) of the whole batch.  An empty list makes no call."""
    if len(objs) == 0:
        return []
    lib = load_library()
    nev = np.zeros(len(objs), np.int32)
    T, conv, nit = _run_align_batch(objs, guesses, lambda arr, n, g, T, conv, nit: lib.gorio_apd_gicp_omp_align_batch(arr, n, g, T, conv, nit, _p(nev, C.c_int)))
    diag = _batch_diag(lib.gorio_apd_gicp_omp_batch_diag, objs[0], ("rounds", "launches"))
    return [dict(T=T[q], H=np.zeros((6, 6), np.float64), converged=bool(conv[q]), nr_iterations=int(nit[q]), n_linearize=int(nev[q]), batch_diag=dict(diag)) for q in range(len(objs))]


def icp_align_batch(objs, guesses=None):
    """gorio_apd_icp_align_batch over a list of ApdGicp objects in ICP mode (all on one device): their aligns in lock-step rounds, every
    result bit for bit the one of the object's own align().  Returns the list of dicts align() returns (n_linearize = the object's
    correspondence passes), each with batch_diag = dict(rounds, launches) of the whole batch.  An empty list makes no call."""
    if len(objs) == 0:
        return []
    lib = load_library()
    T, conv, nit = _run_align_batch(objs, guesses, lib.gorio_apd_icp_align_batch)
    diag = _batch_diag(lib.gorio_apd_icp_batch_diag, objs[0], ("rounds", "launches"))
    out = []
    for q, o in enumerate(objs):
        d = o.icp_diag()  # passes = iterations, plus the pass that found fewer than 3 pairs (state 5) when the align ended there
        out.append(dict(T=T[q], H=np.zeros((6, 6), np.float64), converged=bool(conv[q]), nr_iterations=int(nit[q]), n_linearize=d["iterations"] + (d["state"] == 5),
                        batch_diag=dict(diag)))
    return out


def gicp_mp_align_batch(objs, guesses=None):
    """gorio_apd_gicp_mp_align_batch over a list of ApdGicp objects in GICP_MP mode (all on one device; parameters and radii may
    differ): their aligns in lock-step rounds over one batched radius search per round, every result bit for bit the one of the
    object's own align().  Returns the list of dicts align() returns (H = the last pass's, n_linearize = the object's passes); the
    first carries batch_diag = dict(rounds, launches, syncs, max_round_launches) of the whole batch.  An empty list makes no call."""
    if len(objs) == 0:
        return []
    lib = load_library()
    T, conv, nit = _run_align_batch(objs, guesses, lib.gorio_apd_gicp_mp_align_batch)
    diag = _batch_diag(lib.gorio_apd_gicp_mp_batch_diag, objs[0], ("rounds", "launches", "syncs", "max_round_launches"))
    out = []
    for q, o in enumerate(objs):
        H = np.zeros((6, 6), np.float64)
        _check(o._h, lib.gorio_apd_gicp_mp_last_hessian(o._h, _p(H, C.c_double)))
        out.append(dict(T=T[q], H=H, converged=bool(conv[q]), nr_iterations=int(nit[q]), n_linearize=o.gicp_mp_diag()["passes"]))
    out[0]["batch_diag"] = diag
    return out


def fitness_score_batch(regs, Ts=None, max_range=np.finfo(np.float64).max, inlier_dist=0.0):
    """gorio_apd_fitness_score_batch over a list of ApdGicp objects (all on one device): the getFitnessScore / inlier fraction of every
    object at its pose in one pass.  Ts: n poses (4x4), or None for every object's last final transformation.  inlier_dist <= 0 means the
    nodelet's 0.5 m.  Returns (scores, inlier_fractions), float64 arrays equal bit for bit to the single getFitnessScore calls."""
    lib = load_library()
    n = len(regs)
    scores = np.zeros(n, np.float64)
    inl = np.zeros(n, np.float64)
    if n == 0:
        return scores, inl
    T = np.ascontiguousarray(np.stack([o._final for o in regs]) if Ts is None else Ts, np.float32).reshape(n, 16)
    arr = (C.c_void_p * n)(*[o._h for o in regs])
    rc = lib.gorio_apd_fitness_score_batch(arr, n, _p(T, C.c_float), C.c_double(max_range), C.c_double(inlier_dist), _p(scores, C.c_double), _p(inl, C.c_double))
    _check(regs[0]._h, rc)
    return scores, inl
