"""CPU-side checks of the cross-database Scan Context section (include/gorio_sc_cross.h): the symbols and the binding cover the header,
gorio_sc.h brings the section with it after gorio_sc_pairs.h, GORIO_SC_TOP_MAX is the binding's, null handles are refused with a text,
and the C++ drop-in and its driver build against the stand-ins.  No GPU (a handle cannot exist without one: the checks that need a
handle are in tests/test_sc_cross_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
INVALID = -1
NAMES = ["gorio_sc_cross_counters", "gorio_sc_cross_detect", "gorio_sc_cross_distance_matrix", "gorio_sc_cross_distance_pairs", "gorio_sc_cross_top_matches"]


def _text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_symbols_and_binding_cover_the_header(gorio):
    txt = _text("gorio_sc_cross.h")
    assert sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt))) == sorted(gorio.SC_CROSS_SYMBOLS) == NAMES
    lib = gorio.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    flat = " ".join(txt.split())
    assert "int gorio_sc_cross_distance_pairs(gorio_sc_t* Q, gorio_sc_t* D, const int* q, const int* c, int count, double* dist, int* shift);" in flat
    assert ("int gorio_sc_cross_distance_matrix(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* cols, int n_cols, double* dist, "
            "int* shift);") in flat
    assert ("int gorio_sc_cross_top_matches(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* col_end, int k, int* index, double* dist, "
            "int* shift);") in flat
    assert ("int gorio_sc_cross_detect(gorio_sc_t* Q, gorio_sc_t* D, int count, const int* query_index, const int* const* candidates, const int* n_candidates, "
            "int* loop_id, float* yaw_rad, double* min_dist);") in flat
    assert "int gorio_sc_cross_counters(const gorio_sc_t* Q, long long* calls, long long* pairs, long long* launches, long long* synchronisations);" in flat
    # the header says what it is: an extension with no counterpart in the reference
    whole = open(os.path.join(ROOT, "include", "gorio_sc_cross.h")).read()
    assert "EXTENSION with no counterpart in the Go-RIO sources" in whole
    # gorio_sc.h brings the section with it, after gorio_sc_pairs.h, and declares nothing of it itself
    sc_h = open(os.path.join(ROOT, "include", "gorio_sc.h")).read()
    assert 0 < sc_h.index('#include "gorio_sc_pairs.h"') < sc_h.index('#include "gorio_sc_cross.h"')
    assert not set(NAMES) & set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", _text("gorio_sc.h") + _text("gorio_sc_pairs.h")))
    for m in ("cross_distance_pairs", "cross_distance_matrix", "top_matches", "cross_detect", "cross_counters"):
        assert callable(getattr(gorio.ScanContext, m)), m
    assert re.search(rf"#define GORIO_SC_TOP_MAX {gorio.scan_context.TOP_MAX}\b", txt) and gorio.scan_context.TOP_MAX == 8


def test_null_handles_are_refused_with_a_text(gorio):
    lib = gorio.load_library()
    lib.gorio_sc_last_error.restype = C.c_char_p
    out = (C.c_double * 2)(7.0, 7.0)
    ints = (C.c_int * 2)(7, 7)
    idx = (C.c_int * 2)(0, 0)
    lists = (C.c_void_p * 1)(C.addressof(idx))
    assert lib.gorio_sc_cross_distance_pairs(None, None, idx, idx, 2, out, ints) == INVALID and b"cross_distance_pairs" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_cross_distance_matrix(None, idx, 2, None, idx, 2, out, None) == INVALID and b"cross_distance_matrix" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_cross_top_matches(None, idx, 2, None, None, 1, ints, out, None) == INVALID and b"cross_top_matches" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_cross_detect(None, None, 1, idx, lists, ints, ints, (C.c_float * 1)(), out) == INVALID and b"cross_detect" in lib.gorio_sc_last_error()
    assert b"null query handle" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_cross_counters(None, None, None, None, None) == INVALID and b"cross_counters" in lib.gorio_sc_last_error()
    # even with a count of 0: the handles are looked at first, nothing else is
    assert lib.gorio_sc_cross_distance_pairs(None, None, None, None, 0, None, None) == INVALID
    assert lib.gorio_sc_cross_distance_matrix(None, None, 0, None, None, 0, None, None) == INVALID
    assert lib.gorio_sc_cross_top_matches(None, None, 0, None, None, 0, None, None, None) == INVALID
    assert list(out) == [7.0, 7.0] and list(ints) == [7, 7]  # a refused call writes nothing


def test_dropin_and_driver_build(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_cross_sequence", "test/sc_exhaustive_sequence"])
    assert os.path.exists(os.path.join(HOST, "test", "sc_cross_sequence"))
    hdr = open(os.path.join(HOST, "scan_context", "Scancontext.h")).read()
    for member in ("distanceBtnScanContextBatch(const SCManager& db", "distanceMatrix(const SCManager& db", "topMatches(const SCManager& db", "topMatches(int k, int min_gap)",
                   "detectLoopClosureIDAgainst(const SCManager& db"):
        assert member in hdr, member
    rules = open(os.path.join(HOST, "Makefile")).read()
    assert "test/sc_cross_sequence:" in rules and "test/sc_cross_sequence" in rules[rules.index("clean:"):]
