"""include/gorio_scan_batch.h without a GPU: the symbols and their declarations, and every argument and state error of the batch calls, each
with its code and with text that names the member, before any device call (gorio_scan_create makes no device side)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

OK, INVALID, STATE, UNSUPPORTED = 0, -1, -3, -5


def _err(lib):
    lib.gorio_scan_last_error.restype = C.c_char_p
    return lib.gorio_scan_last_error().decode()


@pytest.fixture()
def handles(gorio):
    lib = gorio.load_library()
    hs = []
    for dev in (0, 0, 0, 1):  # the fourth lives on another device; create checks and stores, nothing more
        h = C.c_void_p()
        assert lib.gorio_scan_create(C.byref(h), dev, C.byref(gorio.prep.scan_default_params())) == OK
        hs.append(h)
    yield hs
    for h in hs:
        lib.gorio_scan_destroy(h)


def _load_args(hs, n=None, stride=None, raws=None):
    count = len(hs)
    raws = raws if raws is not None else [np.ones((4, 5), np.float32) for _ in hs]
    base = [r.__array_interface__["data"][0] for r in raws]
    arr = (C.c_void_p * count)(*hs)
    xyz = (C.c_void_p * count)(*base)
    pw = (C.c_void_p * count)(*[b + 12 for b in base])
    dop = (C.c_void_p * count)(*[b + 16 for b in base])
    nn = (C.c_int * count)(*(n if n is not None else [len(r) for r in raws]))
    st = (C.c_int * count)(*(stride if stride is not None else [20] * count))
    ng, nv = (C.c_int * count)(), (C.c_int * count)()
    return [arr, count, xyz, pw, dop, nn, st, ng, nv], raws


RESULT_BYTES = 80  # sizeof(gorio_scan_result): 3 ints + pad, 6 doubles, 3 ints + pad


def _run_args(hs, n_iter=None, samples=None):
    count = len(hs)
    arr = (C.c_void_p * count)(*hs)
    sp = (C.c_void_p * count)(*(samples if samples is not None else [None] * count))
    ni = (C.c_int * count)(*(n_iter if n_iter is not None else [0] * count))
    wp = (C.c_void_p * count)(*([None] * count))
    res = (C.c_byte * (RESULT_BYTES * count))()  # the call must not get to write it
    codes = (C.c_int * count)()
    return [arr, count, sp, ni, wp, res, codes]


def test_symbols_are_exported_and_declared(gorio):
    lib = gorio.load_library()
    header = open(os.path.join(gorio.INCLUDE_DIR, "gorio_scan_batch.h")).read()
    for name in gorio.prep.SCAN_BATCH_SYMBOLS:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert '#include "gorio_scan_batch.h"' in open(os.path.join(gorio.INCLUDE_DIR, "gorio_scan.h")).read()
    assert int(re.search(r"#define GORIO_SCAN_BATCH_MAX (\d+)", header).group(1)) == gorio.prep.SCAN_BATCH_MAX == 1024
    assert C.sizeof(gorio.prep.ScanResult) == RESULT_BYTES


def test_count_zero_is_ok_and_touches_nothing(gorio):
    lib = gorio.load_library()
    assert lib.gorio_scan_load_batch(None, 0, None, None, None, None, None, None, None) == OK
    assert lib.gorio_scan_run_batch(None, 0, None, None, None, None, None) == OK
    assert gorio.prep.scan_run_batch([], [], []) == []
    ng, nv = gorio.prep.scan_load_batch([], [])
    assert len(ng) == 0 and len(nv) == 0


def test_load_batch_argument_errors_name_the_member(gorio, handles):
    lib = gorio.load_library()
    good = handles[:3]
    args, keep = _load_args(good)
    for k in (0, 2, 3, 4, 5, 6, 7, 8):  # every pointer of the call
        a = list(args)
        a[k] = None
        assert lib.gorio_scan_load_batch(*a) == INVALID, k
        assert "load_batch" in _err(lib)
    a = list(args)
    a[1] = -1
    assert lib.gorio_scan_load_batch(*a) == INVALID and "count" in _err(lib)
    args, keep = _load_args([good[0], None, good[2]])
    assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[1]" in _err(lib)
    args, keep = _load_args([good[0], good[1], good[0]])  # a handle listed twice
    assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[2]" in _err(lib) and "twice" in _err(lib)
    args, keep = _load_args([good[0], handles[3]])  # handles on different devices
    assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[1]" in _err(lib) and "device" in _err(lib)
    for stride in (0, 2, 18, -4):
        args, keep = _load_args(good, stride=[20, 20, stride])
        assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[2]" in _err(lib) and "stride" in _err(lib), stride
    args, keep = _load_args(good, n=[4, -1, 4])
    assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[1]" in _err(lib)
    args, keep = _load_args(good)
    args[3][1] = None  # a member with points and no power column
    assert lib.gorio_scan_load_batch(*args) == INVALID and "handles[1]" in _err(lib)


def test_load_batch_limits_are_unsupported(gorio, handles):
    lib = gorio.load_library()
    many = [handles[i % 3] for i in range(1025)]  # the count is refused before the members are looked at
    args, keep = _load_args(many)
    assert lib.gorio_scan_load_batch(*args) == UNSUPPORTED and "1024" in _err(lib)
    args = _run_args(many)
    assert lib.gorio_scan_run_batch(*args) == UNSUPPORTED and "1024" in _err(lib)
    # more than 2^31 - 1 raw points in all: the sizes are added up before a point is read
    args, keep = _load_args(handles[:3], n=[2**30, 2**30, 4])
    assert lib.gorio_scan_load_batch(*args) == UNSUPPORTED and "2^31" in _err(lib)


def test_run_batch_argument_and_state_errors_name_the_member(gorio, handles):
    lib = gorio.load_library()
    good = handles[:3]
    args = _run_args(good)
    for k in (0, 2, 3, 5, 6):  # ang_vel (4) may be NULL as a whole
        a = list(args)
        a[k] = None
        assert lib.gorio_scan_run_batch(*a) == INVALID, k
        assert "run_batch" in _err(lib)
    a = list(args)
    a[1] = -2
    assert lib.gorio_scan_run_batch(*a) == INVALID and "count" in _err(lib)
    assert lib.gorio_scan_run_batch(*_run_args([good[0], None])) == INVALID and "handles[1]" in _err(lib)
    assert lib.gorio_scan_run_batch(*_run_args([good[1], good[1]])) == INVALID and "handles[1]" in _err(lib) and "twice" in _err(lib)
    assert lib.gorio_scan_run_batch(*_run_args([good[0], good[1], handles[3]])) == INVALID and "handles[2]" in _err(lib) and "device" in _err(lib)
    assert lib.gorio_scan_run_batch(*_run_args(good, n_iter=[0, 0, -1])) == INVALID and "handles[2]" in _err(lib)
    assert lib.gorio_scan_run_batch(*_run_args(good, n_iter=[0, 3, 0])) == INVALID and "handles[1]" in _err(lib)  # iterations without samples
    # no member has a load
    args = _run_args(good)
    assert lib.gorio_scan_run_batch(*args) == STATE and "handles[0]" in _err(lib) and "no scan loaded" in _err(lib)
    assert bytes(args[5]) == bytes(RESULT_BYTES * 3) and list(args[6]) == [0, 0, 0]  # nothing was written


def test_handle_error_and_diag_before_any_batch(gorio, handles):
    lib = gorio.load_library()
    lib.gorio_scan_handle_error.restype = C.c_char_p
    assert lib.gorio_scan_handle_error(handles[0]) == b"" and lib.gorio_scan_handle_error(None) == b""
    r, l, s = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.gorio_scan_batch_diag(handles[0], C.byref(r), C.byref(l), C.byref(s)) == OK and (r.value, l.value, s.value) == (0, 0, 0)
    assert lib.gorio_scan_batch_diag(None, C.byref(r), C.byref(l), C.byref(s)) == INVALID
