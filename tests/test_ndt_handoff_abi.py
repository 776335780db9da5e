"""CPU-side checks of the NDT hand-offs and the batched score (gorio_ndt_set_source_from_scan, _set_target_from_scan,
_set_target_from_apd, gorio_ndt_calculate_score_batch of include/gorio_ndt.h): the symbols are declared, exported and bound with the
declared signatures, and the argument refusals come before any device call."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "gorio_ndt_set_source_from_scan": "int gorio_ndt_set_source_from_scan(gorio_ndt_t* ndt, struct gorio_scan* scan);",
    "gorio_ndt_set_target_from_scan": "int gorio_ndt_set_target_from_scan(gorio_ndt_t* ndt, struct gorio_scan* scan);",
    "gorio_ndt_set_target_from_apd": "int gorio_ndt_set_target_from_apd(gorio_ndt_t* ndt, struct gorio_apd* apd);",
    "gorio_ndt_calculate_score_batch": "int gorio_ndt_calculate_score_batch(gorio_ndt_t* const* handles, int count, const float* T, double* score);",
}
INVALID = -1  # GORIO_ERR_INVALID


def _header():
    txt = open(os.path.join(ROOT, "include", "gorio_ndt.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_symbols_are_declared_exported_and_bound(gorio):
    txt = _header()
    lib = gorio.load_library()
    for name, decl in NEW.items():
        assert decl in txt, name  # the declared signature, token for token
        assert hasattr(lib, name), name
        assert name in gorio.NDT_SYMBOLS
    # the header stays self-contained: the other handle types are forward declarations, not includes
    assert "struct gorio_scan;" in txt and "struct gorio_apd;" in txt and "#include" not in txt
    for member in ("set_source_from_scan", "set_target_from_scan", "set_target_from_apd"):
        assert callable(getattr(gorio.Ndt, member))
    assert callable(gorio.ndt.calculate_score_batch)


def test_null_handles_are_refused_and_the_text_names_the_entry(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    for name in ("gorio_ndt_set_source_from_scan", "gorio_ndt_set_target_from_scan", "gorio_ndt_set_target_from_apd"):
        assert getattr(lib, name)(None, None) == INVALID, name
        assert name[len("gorio_ndt_"):].encode() in lib.gorio_ndt_last_error(), (name, lib.gorio_ndt_last_error())


def test_a_null_producer_is_refused_before_the_ndt_handle_is_read(gorio):
    """A pipeline needs no device until its first load, so one can be made here: it has produced no frame, but the NULL NDT handle is
    reported first."""
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    pipe = gorio.prep.ScanPipeline(gorio.prep.scan_default_params())
    assert lib.gorio_ndt_set_source_from_scan(None, pipe.h) == INVALID
    assert lib.gorio_ndt_set_target_from_scan(None, pipe.h) == INVALID
    assert b"null handle" in lib.gorio_ndt_last_error()
    pipe.close()


def test_score_batch_argument_refusals_need_no_device(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    score = (C.c_double * 2)(7.0, 7.0)
    one = (C.c_void_p * 1)(None)
    assert lib.gorio_ndt_calculate_score_batch(None, 0, None, None) == 0  # count == 0: OK, nothing touched
    assert lib.gorio_ndt_calculate_score_batch(one, 0, None, score) == 0 and score[0] == 7.0
    assert lib.gorio_ndt_calculate_score_batch(one, -1, None, score) == INVALID
    assert b"calculate_score_batch" in lib.gorio_ndt_last_error()
    assert lib.gorio_ndt_calculate_score_batch(None, 1, None, score) == INVALID  # no handle array
    assert lib.gorio_ndt_calculate_score_batch(one, 1, None, None) == INVALID  # no score
    assert lib.gorio_ndt_calculate_score_batch(one, 1, None, score) == INVALID  # a NULL entry
    assert b"calculate_score_batch: handle 0" in lib.gorio_ndt_last_error()
    assert score[0] == 7.0 and score[1] == 7.0


def test_empty_python_batch(gorio):
    s = gorio.ndt.calculate_score_batch([])
    assert s.shape == (0,)


def test_new_driver_does_not_reference_the_test_infrastructure():
    bad = re.compile(r"oracle|import\s+ndt_restatement|from\s+ndt_restatement|#include\s*[<\"][^>\"]*tests/|open\([^)]*tests/")
    m = bad.search(open(os.path.join(ROOT, "go-rio_amd/host/test/ndt_scan_sequence.cpp")).read())
    assert m is None, m.group(0)
