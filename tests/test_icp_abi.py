"""ABI checks of ICP on the registration handle: symbols and signatures, the enumerator, parameter round trip, refusals without a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_icp_params", "gorio_apd_get_icp_params", "gorio_apd_icp_diag", "gorio_apd_icp_step", "gorio_apd_icp_align_batch", "gorio_apd_icp_batch_diag"]
INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5
DBL_MAX = np.finfo(np.float64).max


def header(gorio):
    return open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS
    assert callable(gorio.icp_align_batch)
    for member in ("set_icp_params", "get_icp_params", "icp_step", "icp_diag"):
        assert callable(getattr(gorio.ApdGicp, member))


def test_declared_signatures(gorio):
    text = re.sub(r"/\*.*?\*/", " ", header(gorio), flags=re.S)
    text = re.sub(r"\s+", " ", text)
    for decl in [
        "int gorio_apd_set_icp_params(gorio_apd_t* h, int use_reciprocal, double euclidean_fitness_epsilon, double transformation_rotation_epsilon);",
        "int gorio_apd_get_icp_params(const gorio_apd_t* h, int* use_reciprocal, double* euclidean_fitness_epsilon, double* transformation_rotation_epsilon);",
        "int gorio_apd_icp_diag(const gorio_apd_t* h, int* iterations, int* state, double* mse, int* pairs);",
        "int gorio_apd_icp_step(gorio_apd_t* h, const float T16[16], int* pairs, double sums17[17], float T_est16[16]);",
        "int gorio_apd_icp_align_batch(gorio_apd_t** handles, int count, const float* guesses , float* T_out , int* converged, int* nr_iterations );",
        "int gorio_apd_icp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches);",
    ]:
        assert decl in text, decl


def test_enumerator_is_four_and_the_others_stay(gorio):
    text = re.sub(r"/\*.*?\*/", "", header(gorio), flags=re.S)
    vals = {}
    for name in ("gorio_method", "gorio_method_pcl"):  # both feed the `method` argument of gorio_apd_set_method
        body = re.search(r"typedef enum \{([^}]*)\} %s;" % name, text).group(1)
        vals.update((k, int(v)) for k, v in re.findall(r"(GORIO_METHOD_\w+) = (\d+)", body))
    assert vals == dict(GORIO_METHOD_APDGICP=0, GORIO_METHOD_GICP=1, GORIO_METHOD_VGICP=2, GORIO_METHOD_GICP_OMP=3, GORIO_METHOD_ICP=4)
    assert apd.METHOD_ICP == 4
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15  # the ICP parameters travel by a call of their own


def test_null_handle_and_empty_batch(gorio):
    lib = gorio.load_library()
    i, d = C.c_int(0), C.c_double(0)
    assert lib.gorio_apd_set_icp_params(None, 0, C.c_double(0.0), C.c_double(0.0)) == INVALID
    assert lib.gorio_apd_get_icp_params(None, C.byref(i), C.byref(d), C.byref(d)) == INVALID
    assert lib.gorio_apd_icp_diag(None, None, None, None, None) == INVALID
    assert lib.gorio_apd_icp_step(None, None, None, None, None) == INVALID
    assert lib.gorio_apd_icp_batch_diag(None, None, None) == INVALID
    assert lib.gorio_apd_icp_align_batch(None, 0, None, None, None, None) == 0  # count == 0 is OK
    assert lib.gorio_apd_icp_align_batch(None, 1, None, None, None, None) == INVALID
    assert lib.gorio_apd_icp_align_batch(None, -1, None, None, None, None) == INVALID
    assert gorio.icp_align_batch([]) == []


def test_without_a_device_create_reports_it(gorio):
    """As for the other methods: a handle exists only with a usable device, so without one nothing of ICP can be reached."""
    lib = gorio.load_library()
    h = C.c_void_p()
    rc = lib.gorio_apd_create(C.byref(h), 0)
    assert rc in (0, NO_DEVICE)
    if rc == NO_DEVICE:
        assert not h.value
        with pytest.raises(gorio.GorioError) as e:
            gorio.ApdGicp(device=0)
        assert e.value.code == NO_DEVICE
    else:
        lib.gorio_apd_destroy(h)


@pytest.mark.gpu
def test_defaults_round_trip_and_refusals(gorio, gpu):
    g = gorio.ApdGicp(device=gpu)
    assert g.get_icp_params() == dict(use_reciprocal=False, euclidean_fitness_epsilon=-DBL_MAX, transformation_rotation_epsilon=0.0)
    lib, h = g._lib, g._h
    assert lib.gorio_apd_set_icp_params(h, 2, C.c_double(0.0), C.c_double(0.0)) == INVALID
    assert lib.gorio_apd_set_icp_params(h, 0, C.c_double(float("nan")), C.c_double(0.0)) == INVALID
    assert lib.gorio_apd_set_icp_params(h, 0, C.c_double(0.0), C.c_double(float("nan"))) == INVALID
    assert g.get_icp_params()["use_reciprocal"] is False
    g.set_icp_params(True, 1e-3, 1.0 - 1e-7)  # stored in every mode
    assert g.get_icp_params() == dict(use_reciprocal=True, euclidean_fitness_epsilon=1e-3, transformation_rotation_epsilon=1.0 - 1e-7)
    # the icp calls of another method's handle
    T = (C.c_float * 16)()
    assert g.get_method()["method"] == apd.METHOD_APDGICP
    assert lib.gorio_apd_icp_step(h, T, None, None, None) == STATE
    assert lib.gorio_apd_icp_diag(h, None, None, None, None) == STATE
    assert lib.gorio_apd_icp_batch_diag(h, None, None) == STATE
    # the method: 4 is accepted whatever the voxel arguments, 7 stays unknown
    assert lib.gorio_apd_set_method(h, 4, C.c_double(-1.0), 3, 9) == 0 and g.get_method()["method"] == 4
    assert lib.gorio_apd_set_method(h, 7, C.c_double(1.0), 2, 0) == UNSUPPORTED
    assert g.get_icp_params()["use_reciprocal"] is True
    assert g.icp_diag() == dict(iterations=0, state=0, mse=0.0, pairs=-1)
    assert lib.gorio_apd_icp_step(h, T, None, None, None) == STATE  # no clouds yet
