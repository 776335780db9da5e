"""ABI checks of fast_gicp::FastVGICPCuda on the registration handle (GORIO_METHOD_VGICP_CUDA): declarations, the enumerator, refusals that
need no device, and the sizes the other tests pin."""
import ctypes as C
import importlib
import os
import re

import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_vgicp_cuda_params", "gorio_apd_get_vgicp_cuda_params", "gorio_apd_vgicp_cuda_get_points", "gorio_apd_vgicp_cuda_get_voxels",
       "gorio_apd_vgicp_cuda_get_pairs"]
INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5


def header(gorio):
    return open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS
    for member in ("set_vgicp_cuda_params", "get_vgicp_cuda_params", "vgicp_cuda_points", "vgicp_cuda_voxels", "vgicp_cuda_pairs"):
        assert callable(getattr(gorio.ApdGicp, member))


def test_declared_signatures(gorio):
    text = re.sub(r"/\*.*?\*/", " ", header(gorio), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in [
        "int gorio_apd_set_vgicp_cuda_params(gorio_apd_t* h, int nn_method, double kernel_width, double kernel_max_dist);",
        "int gorio_apd_get_vgicp_cuda_params(const gorio_apd_t* h, int* nn_method, double* kernel_width, double* kernel_max_dist);",
        "int gorio_apd_vgicp_cuda_get_points(gorio_apd_t* h, int which, int capacity, int* n, float* cov_raw, int* n_kept, int* kept_index, float* cov);",
        "int gorio_apd_vgicp_cuda_get_voxels(gorio_apd_t* h, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov);",
        "int gorio_apd_vgicp_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel);",
    ]:
        assert decl in text, decl


def test_enumerator_is_six_and_the_pinned_ones_stay(gorio):
    text = re.sub(r"/\*.*?\*/", "", header(gorio), flags=re.S)
    vals = {}
    for name in ("gorio_method", "gorio_method_pcl", "gorio_method_fast_ndt", "gorio_method_fast_vgicp_cuda"):
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % name, text).group(1)
        vals[name] = {k: int(v) for k, v in re.findall(r"(GORIO_METHOD_\w+) = (\d+)", body)}
    assert vals["gorio_method"] == dict(GORIO_METHOD_APDGICP=0, GORIO_METHOD_GICP=1, GORIO_METHOD_VGICP=2, GORIO_METHOD_GICP_OMP=3)
    assert vals["gorio_method_pcl"] == dict(GORIO_METHOD_ICP=4)
    assert vals["gorio_method_fast_ndt"] == dict(GORIO_METHOD_NDT_CUDA=5)
    assert vals["gorio_method_fast_vgicp_cuda"] == dict(GORIO_METHOD_VGICP_CUDA=6)
    body = re.search(r"typedef enum \{([^}]*)\} gorio_vgicp_cuda_nn;", text).group(1)
    assert dict(re.findall(r"GORIO_VGICP_CUDA_NN_(\w+) = (\d+)", body)) == dict(CPU_PARALLEL_KDTREE="0", GPU_BRUTEFORCE="1", GPU_RBF_KERNEL="2")
    assert apd.METHOD_VGICP_CUDA == 6 and (apd.NN_CPU_PARALLEL_KDTREE, apd.NN_GPU_BRUTEFORCE, apd.NN_GPU_RBF_KERNEL) == (0, 1, 2)
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15  # the new settings travel by a call of their own


def test_header_cites_the_reference_files(gorio):
    text = header(gorio)
    for name in ("fast_vgicp_cuda.hpp", "fast_vgicp_cuda_impl.hpp", "fast_vgicp_cuda.cu", "covariance_estimation.cu", "covariance_estimation_rbf.cu",
                 "covariance_regularization.cu", "gaussian_voxelmap.cu", "find_voxel_correspondences.cu", "compute_derivatives.cu"):
        assert name in text, name


def test_null_handle_refusals(gorio):
    lib = gorio.load_library()
    i, j, d, e = C.c_int(0), C.c_int(0), C.c_double(0), C.c_double(0)
    assert lib.gorio_apd_set_vgicp_cuda_params(None, 0, C.c_double(0.5), C.c_double(3.0)) == INVALID
    assert lib.gorio_apd_get_vgicp_cuda_params(None, C.byref(i), C.byref(d), C.byref(e)) == INVALID
    assert lib.gorio_apd_vgicp_cuda_get_points(None, 1, 0, C.byref(i), None, C.byref(j), None, None) == INVALID
    assert lib.gorio_apd_vgicp_cuda_get_voxels(None, 0, C.byref(i), None, None, None, None) == INVALID
    assert lib.gorio_apd_vgicp_cuda_get_pairs(None, 0, C.byref(i), None, None) == INVALID
    assert lib.gorio_apd_set_method(None, 6, C.c_double(1.0), 1, 0) == INVALID


@pytest.mark.gpu
def test_defaults_round_trip_and_bad_parameter_refusals(gorio, gpu):
    g = gorio.ApdGicp(device=gpu)
    lib, h = g._lib, g._h
    assert g.get_vgicp_cuda_params() == dict(nn_method=0, kernel_width=0.5, kernel_max_dist=3.0)  # fast_vgicp_cuda_impl.hpp:27, 31
    n, m = C.c_int(0), C.c_int(0)
    assert lib.gorio_apd_vgicp_cuda_get_points(h, 1, 0, C.byref(n), None, C.byref(m), None, None) == STATE  # another method's handle
    assert lib.gorio_apd_vgicp_cuda_get_voxels(h, 0, C.byref(n), None, None, None, None) == STATE
    assert lib.gorio_apd_vgicp_cuda_get_pairs(h, 0, C.byref(n), None, None) == STATE
    for bad in ((3, 0.5, 3.0), (-1, 0.5, 3.0), (0, 0.0, 3.0), (0, -0.5, 3.0), (0, float("nan"), 3.0), (0, 0.5, float("inf")), (2, float("inf"), 1.0)):
        assert lib.gorio_apd_set_vgicp_cuda_params(h, bad[0], C.c_double(bad[1]), C.c_double(bad[2])) == INVALID, bad
    assert g.get_vgicp_cuda_params() == dict(nn_method=0, kernel_width=0.5, kernel_max_dist=3.0)
    g.set_vgicp_cuda_params(apd.NN_GPU_RBF_KERNEL, 0.25, -1.0)  # stored in every method; max_dist <= 0 means 5 widths
    assert g.get_vgicp_cuda_params() == dict(nn_method=2, kernel_width=0.25, kernel_max_dist=-1.0)
    assert lib.gorio_apd_vgicp_cuda_get_points(h, 2, 0, C.byref(n), None, C.byref(m), None, None) == INVALID
    # set_method: the checks of NDTCuda
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, 7.0)
    assert lib.gorio_apd_set_method(h, 6, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == UNSUPPORTED  # radius 7 > 3
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, -1.0)
    assert lib.gorio_apd_set_method(h, 6, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == INVALID
    assert lib.gorio_apd_set_method(h, 6, C.c_double(0.0), apd.VOXEL_DIRECT7, 0) == UNSUPPORTED
    assert lib.gorio_apd_set_method(h, 6, C.c_double(1.0), 9, 0) == UNSUPPORTED
    assert g.get_method()["method"] == apd.METHOD_APDGICP  # nothing changed so far
    assert lib.gorio_apd_set_method(h, 2, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == UNSUPPORTED  # DIRECT_RADIUS stays refused for FastVGICP
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, 1.5)
    assert lib.gorio_apd_set_method(h, 6, C.c_double(0.5), apd.VOXEL_DIRECT_RADIUS, 77) == 0  # accepted here; voxel_mode is ignored
    assert g.get_method() == dict(method=6, voxel_resolution=0.5, voxel_search=apd.VOXEL_DIRECT_RADIUS, voxel_mode=apd.VOXEL_ADDITIVE)
    assert lib.gorio_apd_set_ndt_cuda_params(h, 1, C.c_double(3.5)) == UNSUPPORTED  # the radius is in use now
    assert lib.gorio_apd_vgicp_cuda_get_voxels(h, 0, C.byref(n), None, None, None, None) == STATE  # no target
    assert lib.gorio_apd_vgicp_cuda_get_pairs(h, 0, C.byref(n), None, None) == STATE  # no pairs
    assert lib.gorio_apd_set_method(h, 7, C.c_double(1.0), 2, 0) == UNSUPPORTED  # 7 stays unknown
