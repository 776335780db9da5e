"""ABI checks of fast_gicp::FastGICPMultiPoints on the registration handle (GORIO_METHOD_GICP_MP): declarations, the enumerator, refusals that
need no device, argument checks."""
import ctypes as C
import importlib
import os
import re

import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_gicp_mp_params", "gorio_apd_get_gicp_mp_params", "gorio_apd_gicp_mp_get_covariances", "gorio_apd_gicp_mp_pass", "gorio_apd_gicp_mp_get_neighbors",
       "gorio_apd_gicp_mp_get_merged", "gorio_apd_gicp_mp_diag"]
INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5


def header(gorio):
    return open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS
    for member in ("set_gicp_mp_params", "get_gicp_mp_params", "gicp_mp_covariances", "gicp_mp_pass", "gicp_mp_neighbors", "gicp_mp_merged", "gicp_mp_diag"):
        assert callable(getattr(gorio.ApdGicp, member))


def test_declared_signatures(gorio):
    text = re.sub(r"/\*.*?\*/", " ", header(gorio), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in [
        "int gorio_apd_set_gicp_mp_params(gorio_apd_t* h, double neighbor_search_radius);",
        "int gorio_apd_get_gicp_mp_params(const gorio_apd_t* h, double* neighbor_search_radius);",
        "int gorio_apd_gicp_mp_get_covariances(gorio_apd_t* h, int which, int capacity, int* n, float* cov);",
        "int gorio_apd_gicp_mp_pass(gorio_apd_t* h, const float T16[16], int* used, long long* total, double* H, double* g);",
        "int gorio_apd_gicp_mp_get_neighbors(gorio_apd_t* h, long long capacity, int* n_queries, long long* total, long long* offsets, int* idx, float* sqd);",
        "int gorio_apd_gicp_mp_get_merged(gorio_apd_t* h, int capacity, int* n, float* mean_B, float* cov_B, int* used);",
        "int gorio_apd_gicp_mp_diag(const gorio_apd_t* h, int* passes, int* used, long long* total, double* stage_seconds);",
    ]:
        assert decl in text, decl


def test_enumerator_is_eight_and_the_pinned_ones_stay(gorio):
    text = re.sub(r"/\*.*?\*/", "", header(gorio), flags=re.S)
    vals = {}
    for name in ("gorio_method", "gorio_method_pcl", "gorio_method_fast_ndt", "gorio_method_fast_vgicp_cuda", "gorio_method_fast_gicp_mp"):
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % name, text).group(1)
        vals[name] = {k: int(v) for k, v in re.findall(r"(GORIO_METHOD_\w+) = (\d+)", body)}
    assert vals["gorio_method"] == dict(GORIO_METHOD_APDGICP=0, GORIO_METHOD_GICP=1, GORIO_METHOD_VGICP=2, GORIO_METHOD_GICP_OMP=3)
    assert vals["gorio_method_pcl"] == dict(GORIO_METHOD_ICP=4)
    assert vals["gorio_method_fast_ndt"] == dict(GORIO_METHOD_NDT_CUDA=5)
    assert vals["gorio_method_fast_vgicp_cuda"] == dict(GORIO_METHOD_VGICP_CUDA=6)
    assert vals["gorio_method_fast_gicp_mp"] == dict(GORIO_METHOD_GICP_MP=8)
    assert 7 not in [v for d in vals.values() for v in d.values()]
    assert apd.METHOD_GICP_MP == 8
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15  # the radius travels by a call of its own


def test_header_cites_the_reference_files_and_states_the_open_points(gorio):
    text = header(gorio)
    for phrase in ("fast_gicp_mp.hpp", "fast_gicp_mp_impl.hpp", "fast_gicp_mp.cpp", "STANDS IN", "DEVIATIONS", "LDLT", "atan2", "t2 < 1e-12", "ascending (d, original index)"):
        assert phrase in text, phrase


def test_null_handle_refusals(gorio):
    lib = gorio.load_library()
    i, j, d, t = C.c_int(0), C.c_int(0), C.c_double(0), C.c_longlong(0)
    T = (C.c_float * 16)()
    assert lib.gorio_apd_set_gicp_mp_params(None, C.c_double(0.5)) == INVALID
    assert lib.gorio_apd_get_gicp_mp_params(None, C.byref(d)) == INVALID
    assert lib.gorio_apd_gicp_mp_get_covariances(None, 0, 0, C.byref(i), None) == INVALID
    assert lib.gorio_apd_gicp_mp_pass(None, T, C.byref(i), C.byref(t), None, None) == INVALID
    assert lib.gorio_apd_gicp_mp_get_neighbors(None, C.c_longlong(0), C.byref(i), C.byref(t), None, None, None) == INVALID
    assert lib.gorio_apd_gicp_mp_get_merged(None, 0, C.byref(i), None, None, None) == INVALID
    assert lib.gorio_apd_gicp_mp_diag(None, C.byref(i), C.byref(j), C.byref(t), None) == INVALID
    assert lib.gorio_apd_set_method(None, 8, C.c_double(1.0), 2, 0) == INVALID


@pytest.mark.gpu
def test_defaults_round_trip_and_refusals(gorio, gpu):
    g = gorio.ApdGicp(device=gpu)
    lib, h = g._lib, g._h
    assert g.get_gicp_mp_params() == dict(neighbor_search_radius=0.5)  # fast_gicp_mp_impl.hpp:35
    n, m, t = C.c_int(0), C.c_int(0), C.c_longlong(0)
    T = (C.c_float * 16)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
    assert lib.gorio_apd_gicp_mp_get_covariances(h, 0, 0, C.byref(n), None) == STATE  # another method's handle
    assert lib.gorio_apd_gicp_mp_pass(h, T, None, None, None, None) == STATE
    assert lib.gorio_apd_gicp_mp_get_neighbors(h, C.c_longlong(0), C.byref(n), C.byref(t), None, None, None) == STATE
    assert lib.gorio_apd_gicp_mp_get_merged(h, 0, C.byref(n), None, None, None) == STATE
    assert lib.gorio_apd_gicp_mp_diag(h, C.byref(n), C.byref(m), C.byref(t), None) == STATE
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        assert lib.gorio_apd_set_gicp_mp_params(h, C.c_double(bad)) == INVALID, bad
    assert g.get_gicp_mp_params() == dict(neighbor_search_radius=0.5)
    g.set_gicp_mp_params(0.25)  # stored in every method
    assert g.get_gicp_mp_params() == dict(neighbor_search_radius=0.25)
    assert lib.gorio_apd_set_method(h, 7, C.c_double(1.0), 2, 0) == UNSUPPORTED  # 7 stays unknown
    assert lib.gorio_apd_set_method(h, 9, C.c_double(1.0), 2, 0) == UNSUPPORTED
    assert g.get_method()["method"] == apd.METHOD_APDGICP
    assert lib.gorio_apd_set_method(h, 8, C.c_double(-3.0), 77, 99) == 0  # the voxel arguments are ignored, as for ICP
    assert g.get_method() == dict(method=8, voxel_resolution=1.0, voxel_search=apd.VOXEL_DIRECT1, voxel_mode=apd.VOXEL_ADDITIVE)
    assert lib.gorio_apd_gicp_mp_get_covariances(h, 2, 0, C.byref(n), None) == INVALID
    assert lib.gorio_apd_gicp_mp_get_covariances(h, 0, 0, C.byref(n), None) == STATE  # no source
    assert lib.gorio_apd_gicp_mp_pass(h, T, None, None, None, None) == STATE  # no clouds
    assert lib.gorio_apd_gicp_mp_get_neighbors(h, C.c_longlong(0), C.byref(n), C.byref(t), None, None, None) == STATE  # no pass
    assert lib.gorio_apd_gicp_mp_get_merged(h, 0, C.byref(n), None, None, None) == STATE
    assert lib.gorio_apd_gicp_mp_diag(h, C.byref(n), C.byref(m), C.byref(t), None) == 0 and (n.value, m.value, t.value) == (0, 0, 0)
    Td, e = (C.c_double * 16)(), C.c_double(0)
    assert lib.gorio_apd_linearize(h, Td, None, None, C.byref(e)) == UNSUPPORTED
    assert lib.gorio_apd_compute_error(h, Td, C.byref(e)) == UNSUPPORTED
    assert lib.gorio_apd_get_correspondences(h, None, None, 0) == UNSUPPORTED
    buf = (C.c_double * 16)()
    assert lib.gorio_apd_get_mahalanobis(h, buf, 0) == UNSUPPORTED
    assert lib.gorio_apd_debug_set_shard(h, 2, 0) == STATE
    assert lib.gorio_apd_calculate_covariances(h) == STATE
