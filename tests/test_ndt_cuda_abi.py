"""ABI checks of fast_gicp::NDTCuda on the registration handle (GORIO_METHOD_NDT_CUDA): declarations, the enumerator, refusals that need
no device, and the sizes the other tests pin."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_ndt_cuda_params", "gorio_apd_get_ndt_cuda_params", "gorio_apd_ndt_cuda_get_voxels", "gorio_apd_ndt_cuda_get_pairs"]
INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5


def header(gorio):
    return open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS
    for member in ("set_ndt_cuda_params", "get_ndt_cuda_params", "ndt_cuda_voxels", "ndt_cuda_pairs"):
        assert callable(getattr(gorio.ApdGicp, member))


def test_declared_signatures(gorio):
    text = re.sub(r"/\*.*?\*/", " ", header(gorio), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in [
        "int gorio_apd_set_ndt_cuda_params(gorio_apd_t* h, int distance_mode, double radius);",
        "int gorio_apd_get_ndt_cuda_params(const gorio_apd_t* h, int* distance_mode, double* radius);",
        "int gorio_apd_ndt_cuda_get_voxels(gorio_apd_t* h, int which, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov_raw, float* cov);",
        "int gorio_apd_ndt_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel);",
    ]:
        assert decl in text, decl


def test_enumerator_is_five_and_the_pinned_ones_stay(gorio):
    text = re.sub(r"/\*.*?\*/", "", header(gorio), flags=re.S)
    vals = {}
    for name in ("gorio_method", "gorio_method_pcl", "gorio_method_fast_ndt"):
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % name, text).group(1)
        vals[name] = {k: int(v) for k, v in re.findall(r"(GORIO_METHOD_\w+) = (\d+)", body)}
    assert vals["gorio_method"] == dict(GORIO_METHOD_APDGICP=0, GORIO_METHOD_GICP=1, GORIO_METHOD_VGICP=2, GORIO_METHOD_GICP_OMP=3)
    assert vals["gorio_method_pcl"] == dict(GORIO_METHOD_ICP=4)
    assert vals["gorio_method_fast_ndt"] == dict(GORIO_METHOD_NDT_CUDA=5)
    body = re.search(r"typedef enum \{([^}]*)\} gorio_ndt_cuda_distance;", text).group(1)
    assert dict(re.findall(r"(GORIO_NDT_CUDA_\w+) = (\d+)", body)) == dict(GORIO_NDT_CUDA_P2D="0", GORIO_NDT_CUDA_D2D="1")
    assert apd.METHOD_NDT_CUDA == 5 and (apd.NDT_CUDA_P2D, apd.NDT_CUDA_D2D) == (0, 1)
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15  # the new settings travel by a call of their own


def test_null_handle_refusals(gorio):
    lib = gorio.load_library()
    i, d = C.c_int(0), C.c_double(0)
    assert lib.gorio_apd_set_ndt_cuda_params(None, 1, C.c_double(1.0)) == INVALID
    assert lib.gorio_apd_get_ndt_cuda_params(None, C.byref(i), C.byref(d)) == INVALID
    assert lib.gorio_apd_ndt_cuda_get_voxels(None, 1, 0, C.byref(i), None, None, None, None, None) == INVALID
    assert lib.gorio_apd_ndt_cuda_get_pairs(None, 0, C.byref(i), None, None) == INVALID
    assert lib.gorio_apd_set_method(None, 5, C.c_double(1.0), 1, 0) == INVALID


@pytest.mark.gpu
def test_defaults_round_trip_and_range_refusals(gorio, gpu):
    g = gorio.ApdGicp(device=gpu)
    lib, h = g._lib, g._h
    assert g.get_ndt_cuda_params() == dict(distance_mode=apd.NDT_CUDA_D2D, radius=-1.0)  # ndt_cuda.cu:21, ndt_cuda.hpp:55
    n = C.c_int(0)
    assert lib.gorio_apd_ndt_cuda_get_voxels(h, 1, 0, C.byref(n), None, None, None, None, None) == STATE  # another method's handle
    assert lib.gorio_apd_ndt_cuda_get_pairs(h, 0, C.byref(n), None, None) == STATE
    assert lib.gorio_apd_set_ndt_cuda_params(h, 2, C.c_double(1.0)) == INVALID
    assert lib.gorio_apd_set_ndt_cuda_params(h, 0, C.c_double(float("nan"))) == INVALID
    g.set_ndt_cuda_params(apd.NDT_CUDA_P2D, 7.0)  # stored in every mode; not in use, so not range-checked yet
    assert g.get_ndt_cuda_params() == dict(distance_mode=0, radius=7.0)
    assert lib.gorio_apd_set_method(h, 5, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == UNSUPPORTED  # radius 7 > 3
    g.set_ndt_cuda_params(apd.NDT_CUDA_P2D, -1.0)
    assert lib.gorio_apd_set_method(h, 5, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == INVALID
    assert lib.gorio_apd_set_method(h, 5, C.c_double(0.0), apd.VOXEL_DIRECT7, 0) == UNSUPPORTED
    assert lib.gorio_apd_set_method(h, 5, C.c_double(1.0), 9, 0) == UNSUPPORTED
    assert g.get_method()["method"] == apd.METHOD_APDGICP  # nothing changed so far
    assert lib.gorio_apd_set_method(h, 2, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == UNSUPPORTED  # DIRECT_RADIUS stays refused for FastVGICP
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, 1.5)
    assert lib.gorio_apd_set_method(h, 5, C.c_double(0.5), apd.VOXEL_DIRECT_RADIUS, 77) == 0  # voxel_mode is ignored
    assert g.get_method() == dict(method=5, voxel_resolution=0.5, voxel_search=apd.VOXEL_DIRECT_RADIUS, voxel_mode=apd.VOXEL_ADDITIVE)
    assert lib.gorio_apd_set_ndt_cuda_params(h, 1, C.c_double(3.5)) == UNSUPPORTED  # in use now
    assert lib.gorio_apd_set_ndt_cuda_params(h, 1, C.c_double(0.0)) == INVALID
    assert g.get_ndt_cuda_params() == dict(distance_mode=1, radius=1.5)
    assert lib.gorio_apd_set_method(h, 7, C.c_double(1.0), 2, 0) == UNSUPPORTED  # 7 stays unknown
