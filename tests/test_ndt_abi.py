"""CPU-side checks of the NDT boundary (include/gorio_ndt.h): the binding covers the header, the defaults are the constructor's
(NDT:47-76), there is no CPU fallback, unsupported settings are refused before any device is touched, and the product does not reach
into the test infrastructure.  The one check that needs a handle (align before set_target) is marked gpu."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))


def test_binding_covers_header(gorio):
    assert sorted(gorio.NDT_SYMBOLS) == _declared("gorio_ndt.h")
    lib = gorio.load_library()
    for name in gorio.NDT_SYMBOLS:
        assert hasattr(lib, name)


def test_struct_layouts(gorio):
    assert C.sizeof(gorio.ndt.NdtParams) == 56 and C.sizeof(gorio.ndt.NdtDiag) == 24


def test_default_params_are_the_constructors(gorio):
    p = gorio.ndt.default_params()
    assert (p.resolution, p.step_size, p.outlier_ratio, p.transformation_epsilon, p.max_iterations) == (1.0, 0.1, 0.55, 0.1, 35)
    assert (p.search, p.min_points_per_voxel, p.min_covar_eigvalue_mult) == (gorio.ndt.DIRECT7, 6, 0.01)
    assert (gorio.ndt.KDTREE, gorio.ndt.DIRECT26, gorio.ndt.DIRECT7, gorio.ndt.DIRECT1) == (0, 1, 2, 3)  # NDTH:52-57


def test_no_cpu_fallback_without_device(gorio):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = gorio.load_library()
    h = C.c_void_p()
    assert lib.gorio_ndt_create(C.byref(h), 0) == -2  # GORIO_ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(gorio.GorioError):
        gorio.Ndt()


def test_unsupported_settings_refused_before_device(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    for field, value in (("search", gorio.ndt.KDTREE), ("search", 7), ("resolution", 0.0), ("resolution", -0.5)):
        p = gorio.ndt.default_params()
        setattr(p, field, value)
        assert lib.gorio_ndt_set_params(None, C.byref(p)) == -5, (field, value)  # GORIO_ERR_UNSUPPORTED
    assert b"KDTREE" in lib.gorio_ndt_last_error() or b"resolution" in lib.gorio_ndt_last_error()
    assert lib.gorio_ndt_set_params(None, C.byref(gorio.ndt.default_params())) == -1  # a good value, no handle
    assert lib.gorio_ndt_align(None, None, None, None, None, None, None) == -1


@pytest.mark.gpu
def test_align_before_set_target_is_a_state_error(gpu, gorio):
    import numpy as np

    n = gorio.Ndt(device=gpu)
    n.set_source(np.zeros((10, 3), np.float32))
    with pytest.raises(gorio.GorioError) as e:
        n.align()
    assert e.value.code == -3  # GORIO_ERR_STATE
    n.close()


def test_library_does_not_reference_the_test_infrastructure():
    """No product file includes, imports, links or opens anything under oracle/ or tests/."""
    bad = re.compile(r"oracle|import\s+ndt_restatement|from\s+ndt_restatement|#include\s*[<\"][^>\"]*tests/|open\([^)]*tests/")
    for rel in ("go-rio_amd/csrc/apd_ndt.hip", "go-rio_amd/ndt.py", "include/gorio_ndt.h", "go-rio_amd/host/pclomp/ndt_omp.h", "go-rio_amd/host/test/ndt_sequence.cpp"):
        m = bad.search(open(os.path.join(ROOT, rel)).read())
        assert m is None, (rel, m.group(0))
