"""CPU-side checks of the batched NDT boundary (gorio_ndt_align_batch, gorio_ndt_set_target_shared of include/gorio_ndt.h): struct
layout, the argument refusals that need no device, and that the product does not reach into the test infrastructure."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_stats_layout(gorio):
    assert C.sizeof(gorio.ndt.NdtBatchStats) == 12
    assert gorio.NdtBatchStats is gorio.ndt.NdtBatchStats


def test_argument_refusals_need_no_device(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    T = (C.c_float * 16)()
    assert lib.gorio_ndt_align_batch(None, 1, None, T, None, None, None, None, None) == -1  # GORIO_ERR_INVALID
    one = (C.c_void_p * 1)(None)
    assert lib.gorio_ndt_align_batch(one, -1, None, T, None, None, None, None, None) == -1
    assert lib.gorio_ndt_align_batch(one, 1, None, None, None, None, None, None, None) == -1  # no T_out
    assert lib.gorio_ndt_align_batch(one, 1, None, T, None, None, None, None, None) == -1  # a NULL entry
    assert b"handle 0" in lib.gorio_ndt_last_error()
    stats = gorio.ndt.NdtBatchStats(7, 7, 7)
    assert lib.gorio_ndt_align_batch(None, 0, None, None, None, None, None, None, None) == 0
    assert lib.gorio_ndt_align_batch(None, 0, None, None, None, None, None, None, C.byref(stats)) == 0
    assert (stats.rounds, stats.evaluations, stats.launches) == (0, 0, 0)
    assert lib.gorio_ndt_set_target_shared(None, None) == -1


def test_empty_python_batch(gorio):
    res, stats = gorio.ndt.align_batch([])
    assert res == [] and stats.rounds == 0


def test_product_does_not_reference_the_test_infrastructure():
    """No product file includes, imports, links or opens anything under oracle/ or tests/."""
    bad = re.compile(r"oracle|import\s+ndt_restatement|from\s+ndt_restatement|#include\s*[<\"][^>\"]*tests/|open\([^)]*tests/")
    for rel in ("go-rio_amd/csrc/apd_ndt.hip", "go-rio_amd/ndt.py", "include/gorio_ndt.h", "go-rio_amd/host/pclomp/ndt_omp.h", "go-rio_amd/host/test/ndt_sequence.cpp",
                "go-rio_amd/host/test/ndt_batch.cpp"):
        m = bad.search(open(os.path.join(ROOT, rel)).read())
        assert m is None, (rel, m.group(0))
