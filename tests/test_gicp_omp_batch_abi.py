"""CPU-side checks of the batched GICP_OMP boundary (gorio_apd_gicp_omp_align_batch / _batch_diag of include/gorio_apd.h): the symbols and
their documented signatures, the argument refusals that need no device, the empty Python batch, and that the product does not reach into
the test infrastructure."""
import ctypes as C
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def test_symbols_and_signatures(gorio):
    lib = gorio.load_library()
    apd = importlib.import_module("go-rio_amd.apd")
    for name in ("gorio_apd_gicp_omp_align_batch", "gorio_apd_gicp_omp_batch_diag"):
        assert name in apd.APD_SYMBOLS and getattr(lib, name) is not None
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gorio_apd.h")).read(), flags=re.S)
    header = re.sub(r"\s+", " ", header)
    assert ("int gorio_apd_gicp_omp_align_batch(gorio_apd_t** handles, int count, const float* guesses , float* T_out , int* converged, int* nr_iterations, "
            "int* n_evaluations );") in header
    assert "int gorio_apd_gicp_omp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches);" in header
    assert gorio.gicp_omp_align_batch is apd.gicp_omp_align_batch


def test_argument_refusals_need_no_device(gorio):
    lib = gorio.load_library()
    g = (C.c_float * 16)()
    T = (C.c_float * 16)()
    one = (C.c_void_p * 1)(None)
    assert lib.gorio_apd_gicp_omp_align_batch(None, 1, g, T, None, None, None) == INVALID  # a null array
    assert lib.gorio_apd_gicp_omp_align_batch(one, -1, g, T, None, None, None) == INVALID  # count < 0
    assert lib.gorio_apd_gicp_omp_align_batch(one, 1, g, T, None, None, None) == INVALID  # a null entry
    assert lib.gorio_apd_gicp_omp_align_batch(one, 1, None, T, None, None, None) == INVALID  # no guesses
    assert lib.gorio_apd_gicp_omp_align_batch(one, 1, g, None, None, None, None) == INVALID  # no T_out
    assert lib.gorio_apd_gicp_omp_align_batch(None, 0, None, None, None, None, None) == 0  # count == 0 is GORIO_OK whatever else is passed
    assert lib.gorio_apd_gicp_omp_align_batch(one, 0, g, T, None, None, None) == 0
    assert lib.gorio_apd_gicp_omp_batch_diag(None, None, None) == INVALID


def test_empty_python_batch(gorio):
    assert gorio.gicp_omp_align_batch([]) == []
    assert gorio.gicp_omp_align_batch([], None) == []


def test_product_does_not_reference_the_test_infrastructure():
    """No product file includes, imports, links or opens anything under oracle/ or tests/."""
    bad = re.compile(r"oracle/|import\s+oracle|from\s+oracle|import\s+gicp_omp_restatement|from\s+gicp_omp_restatement|gicp_omp_batch_scenes|#include\s*[<\"][^>\"]*tests/|open\([^)]*tests/")
    for rel in ("go-rio_amd/csrc/apd_gicp_omp.hip", "go-rio_amd/csrc/gicp_bfgs.h", "go-rio_amd/apd.py", "include/gorio_apd.h", "go-rio_amd/host/pclomp/gicp_omp.h",
                "go-rio_amd/host/test/gicp_omp_batch.cpp", "go-rio_amd/host/test/gicp_bfgs_machine.cpp"):
        m = bad.search(open(os.path.join(ROOT, rel)).read())
        assert m is None, (rel, m.group(0))
