"""ABI checks of GICP_OMP on the registration handle: symbols, the enumerator, defaults and refusals."""
import ctypes as C
import importlib
import os
import re

import pytest

apd = importlib.import_module("go-rio_amd.apd")
NEW = ["gorio_apd_set_gicp_omp_params", "gorio_apd_get_gicp_omp_params", "gorio_apd_gicp_omp_update", "gorio_apd_gicp_omp_evaluate", "gorio_apd_gicp_omp_diag"]
INVALID, STATE, UNSUPPORTED = -1, -3, -5


def test_new_symbols_exported_and_bound(gorio):
    lib = gorio.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in apd.APD_SYMBOLS


def test_enumerator_is_three_and_the_others_stay(gorio):
    text = open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()
    body = re.search(r"typedef enum \{([^}]*)\} gorio_method;", text).group(1)
    vals = dict((k, int(v)) for k, v in re.findall(r"(GORIO_METHOD_\w+) = (\d+)", body))
    assert vals == dict(GORIO_METHOD_APDGICP=0, GORIO_METHOD_GICP=1, GORIO_METHOD_VGICP=2, GORIO_METHOD_GICP_OMP=3)
    assert apd.METHOD_GICP_OMP == 3 and (apd.GICP_OMP_F, apd.GICP_OMP_DF, apd.GICP_OMP_FDF) == (0, 1, 2)
    assert C.sizeof(gorio.ApdParams) == 96 and len(gorio.ApdParams._fields_) == 15  # the two new parameters travel by a call of their own


def test_null_handle_is_refused(gorio):
    lib = gorio.load_library()
    e, m = C.c_double(0), C.c_int(0)
    assert lib.gorio_apd_set_gicp_omp_params(None, C.c_double(1e-3), 20) == INVALID
    assert lib.gorio_apd_get_gicp_omp_params(None, C.byref(e), C.byref(m)) == INVALID
    assert lib.gorio_apd_gicp_omp_update(None, None, None, C.byref(m)) == INVALID
    assert lib.gorio_apd_gicp_omp_evaluate(None, None, 0, None, None) == INVALID
    assert lib.gorio_apd_gicp_omp_diag(None, None, None, None, None) == INVALID


@pytest.mark.gpu
def test_defaults_and_parameter_refusals(gorio, gpu):
    g = gorio.ApdGicp(device=gpu)
    assert g.getGicpOmpParams() == (0.001, 20)
    lib, h = g._lib, g._h
    assert lib.gorio_apd_set_gicp_omp_params(h, C.c_double(1e-3), 0) == INVALID
    assert lib.gorio_apd_set_gicp_omp_params(h, C.c_double(0.0), 20) == INVALID
    assert lib.gorio_apd_set_gicp_omp_params(h, C.c_double(-1.0), 20) == INVALID
    assert lib.gorio_apd_set_gicp_omp_params(h, C.c_double(float("nan")), 20) == INVALID
    assert g.getGicpOmpParams() == (0.001, 20)
    g.setGicpOmpParams(0.01, 7)
    assert g.getGicpOmpParams() == (0.01, 7)
    # the method: 3 is accepted whatever the voxel arguments, the pinned refusals stay
    assert g.get_method()["method"] == apd.METHOD_APDGICP
    assert lib.gorio_apd_set_method(h, 3, C.c_double(-1.0), 3, 9) == 0 and g.get_method()["method"] == 3
    assert lib.gorio_apd_set_method(h, 7, C.c_double(1.0), 2, 0) == UNSUPPORTED
    assert lib.gorio_apd_set_method(h, 2, C.c_double(1.0), apd.VOXEL_DIRECT_RADIUS, 0) == UNSUPPORTED
    # hooks of another method's handle, and before any pairs
    m = C.c_int(0)
    f = C.c_double(0)
    x = (C.c_double * 6)()
    assert lib.gorio_apd_gicp_omp_evaluate(h, x, 0, C.byref(f), None) == STATE
    g.set_method(apd.METHOD_GICP)
    assert lib.gorio_apd_gicp_omp_evaluate(h, x, 0, C.byref(f), None) == STATE
    assert lib.gorio_apd_gicp_omp_diag(h, None, None, None, C.byref(m)) == 0
