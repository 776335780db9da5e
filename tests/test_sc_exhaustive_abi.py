"""CPU-side checks of the exhaustive Scan Context section (include/gorio_sc_pairs.h): the symbols and the binding cover the header,
gorio_sc.h brings the section with it, the argument errors that need no handle are reported as gorio_sc.h prescribes, and the C++
drop-in and its driver build against the stand-ins.  No GPU (a handle cannot exist without one: the checks that need a handle are in
tests/test_sc_exhaustive_gpu.py)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
INVALID = -1
NAMES = ["gorio_sc_best_matches", "gorio_sc_detect_exhaustive", "gorio_sc_distance_matrix", "gorio_sc_distance_pairs", "gorio_sc_pairs_counters"]


def _text(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def test_symbols_and_binding_cover_the_header(gorio):
    txt = _text("gorio_sc_pairs.h")
    assert sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt))) == sorted(gorio.SC_PAIRS_SYMBOLS) == NAMES
    lib = gorio.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
    flat = " ".join(txt.split())
    assert "int gorio_sc_distance_pairs(gorio_sc_t* h, const int* q, const int* c, int count, double* dist, int* shift);" in flat
    assert "int gorio_sc_distance_matrix(gorio_sc_t* h, const int* rows, int n_rows, const int* cols, int n_cols, double* dist, int* shift);" in flat
    assert "int gorio_sc_best_matches(gorio_sc_t* h, const int* rows, int n_rows, int min_gap, int* best_index, double* best_dist, int* best_shift);" in flat
    assert ("int gorio_sc_detect_exhaustive(gorio_sc_t* h, int count, const int* query_index, const int* const* candidates, const int* n_candidates, int* loop_id, "
            "float* yaw_rad, double* min_dist);") in flat
    assert "int gorio_sc_pairs_counters(const gorio_sc_t* h, long long* calls, long long* pairs, long long* launches, long long* synchronisations);" in flat
    # gorio_sc.h brings the section with it, at its end, and declares nothing of it itself
    sc_h = open(os.path.join(ROOT, "include", "gorio_sc.h")).read()
    assert sc_h.rstrip().endswith("#endif /* GORIO_SC_H */") and '#include "gorio_sc_pairs.h"' in sc_h[sc_h.rindex("gorio_sc_last_error"):]
    assert not set(NAMES) & set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", _text("gorio_sc.h")))
    for m in ("distance_pairs", "distance_matrix", "best_matches", "detect_exhaustive", "pairs_counters"):
        assert callable(getattr(gorio.ScanContext, m)), m
    S = gorio.scan_context
    for name, v in (("GORIO_SC_TILE_ROWS", S.TILE_ROWS), ("GORIO_SC_TILE_COLS", S.TILE_COLS), ("GORIO_SC_PAIRS_PER_GROUP", S.PAIRS_PER_GROUP)):
        assert re.search(rf"#define {name} {v}\b", txt), name


def test_null_handle_is_refused_with_a_text(gorio):
    lib = gorio.load_library()
    lib.gorio_sc_last_error.restype = C.c_char_p
    out = (C.c_double * 2)(7.0, 7.0)
    ints = (C.c_int * 2)(7, 7)
    idx = (C.c_int * 2)(0, 0)
    lists = (C.c_void_p * 1)(C.addressof(idx))
    assert lib.gorio_sc_distance_pairs(None, idx, idx, 2, out, ints) == INVALID and b"distance_pairs" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_distance_matrix(None, idx, 2, idx, 2, out, None) == INVALID and b"distance_matrix" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_best_matches(None, idx, 2, 1, ints, out, None) == INVALID and b"best_matches" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_detect_exhaustive(None, 1, idx, lists, ints, ints, (C.c_float * 1)(), out) == INVALID and b"detect_exhaustive" in lib.gorio_sc_last_error()
    assert lib.gorio_sc_pairs_counters(None, None, None, None, None) == INVALID and b"pairs_counters" in lib.gorio_sc_last_error()
    # even with a count of 0: the handle is looked at first, nothing else is
    assert lib.gorio_sc_distance_pairs(None, None, None, 0, None, None) == INVALID
    assert lib.gorio_sc_distance_matrix(None, None, 0, None, 0, None, None) == INVALID
    assert list(out) == [7.0, 7.0] and list(ints) == [7, 7]  # a refused call writes nothing


def test_dropin_and_driver_build(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_exhaustive_sequence", "test/sc_sequence"])
    assert os.path.exists(os.path.join(HOST, "test", "sc_exhaustive_sequence"))
    hdr = open(os.path.join(HOST, "scan_context", "Scancontext.h")).read()
    for member in ("distanceBtnScanContextBatch", "distanceMatrix", "bestMatches", "detectLoopClosureIDExhaustive"):
        assert member in hdr, member
