"""CPU-side checks of gorio_search_radius_batch (include/gorio_search.h): exported, bound, declared with the signature the header
documents, and its argument rules that need no device -- count == 0, count < 0, null arrays, a null handle -- answered before any device
call, each with its own message.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SIGNATURE = ("int gorio_search_radius_batch(gorio_search_t** handles, int count, const float* const* q_xyz, const int* nq, const int* stride_bytes, const double* radius, "
             "const int* max_nn, int* const* count_out, long long* totals);")


def test_symbol_exported_bound_and_declared(gorio):
    lib = gorio.load_library()
    assert hasattr(lib, "gorio_search_radius_batch") and "gorio_search_radius_batch" in gorio.SEARCH_SYMBOLS
    assert callable(gorio.Search.radius_batch)
    text = open(os.path.join(ROOT, "include", "gorio_search.h")).read()
    assert SIGNATURE in re.sub(r"\s+", " ", text)
    doc = text[:text.index("int gorio_search_radius_batch(")]
    doc = re.sub(r"\s*\n \*\s?", " ", doc[doc.rindex("/*"):])  # the comment as running text
    for word in ("bit for bit", "ONE synchronisation", "q_xyz[j] == NULL", "count == 0", "GORIO_ERR_INVALID", "the same handle twice", "GORIO_ERR_UNSUPPORTED", "job <j>"):
        assert word in doc, word
    assert gorio.Search.radius_batch([], [], 0.5) == []  # an empty batch makes no call


def test_arguments_refused_before_any_device_call(gorio):
    lib = gorio.load_library()
    lib.gorio_search_last_error.restype = C.c_char_p
    q = np.zeros((4, 3), np.float32)
    hs = (C.c_void_p * 2)(None, None)
    qp = (C.c_void_p * 2)(q.ctypes.data, q.ctypes.data)
    nq, st, r, m = (C.c_int * 2)(4, 4), (C.c_int * 2)(12, 12), (C.c_double * 2)(0.5, 0.5), (C.c_int * 2)(0, 0)
    tot = (C.c_longlong * 2)(-7, -7)
    fn = lib.gorio_search_radius_batch
    assert fn(None, 0, None, None, None, None, None, None, None) == 0  # count == 0 touches nothing
    assert fn(hs, -1, qp, nq, st, r, m, None, tot) == INVALID and b"count" in lib.gorio_search_last_error()
    for args in ((None, 2, qp, nq, st, r, m, None, tot), (hs, 2, None, nq, st, r, m, None, tot), (hs, 2, qp, None, st, r, m, None, tot), (hs, 2, qp, nq, None, r, m, None, tot),
                 (hs, 2, qp, nq, st, None, m, None, tot), (hs, 2, qp, nq, st, r, None, None, tot), (hs, 2, qp, nq, st, r, m, None, None)):
        assert fn(*args) == INVALID and b"null array" in lib.gorio_search_last_error()
    assert fn(hs, 2, qp, nq, st, r, m, None, tot) == INVALID and b"job 0: null handle" in lib.gorio_search_last_error()
    assert list(tot) == [-7, -7]
