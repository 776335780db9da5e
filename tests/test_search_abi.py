"""CPU-side checks of the search boundary (include/gorio_search.h): the binding covers the header, arguments are refused before any
device call (so the refusals are the same with and without a GPU, and name the argument), there is no CPU fallback, and the C++
drop-in and its driver build against the stand-ins.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -5


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))


def test_binding_covers_header(gorio):
    assert sorted(gorio.SEARCH_SYMBOLS) == _declared("gorio_search.h")
    lib = gorio.load_library()
    for name in gorio.SEARCH_SYMBOLS:
        assert hasattr(lib, name)
    assert gorio.Search is gorio.search.Search and gorio.search.MAX_K == 32


@pytest.fixture(scope="module")
def lib(gorio):
    lib = gorio.load_library()
    lib.gorio_search_last_error.restype = C.c_char_p
    return lib


def _p(a):
    return C.c_void_p(a.__array_interface__["data"][0])


def _refused(lib, rc, code, word):
    assert rc == code
    assert word in lib.gorio_search_last_error().decode()


def test_knn_arguments_refused_before_any_device_call(lib):
    """Without a handle no device call is possible; the argument rules still answer, each with its own message."""
    q = np.zeros((4, 3), np.float32)
    idx, sqd, cnt = np.zeros((4, 32), np.int32), np.zeros((4, 32), np.float32), np.zeros(4, np.int32)
    for fn in (lib.gorio_search_knn, lib.gorio_search_knn_device):
        _refused(lib, fn(None, _p(q), 4, 12, 0, _p(idx), _p(sqd), _p(cnt)), INVALID, "k must be at least 1")
        _refused(lib, fn(None, _p(q), 4, 12, -3, _p(idx), _p(sqd), _p(cnt)), INVALID, "k must be at least 1")
        _refused(lib, fn(None, _p(q), 4, 12, 33, _p(idx), _p(sqd), _p(cnt)), UNSUPPORTED, "at most 32")
        _refused(lib, fn(None, _p(q), 4, 12, 5, None, _p(sqd), _p(cnt)), INVALID, "null output")
        _refused(lib, fn(None, _p(q), 4, 12, 5, _p(idx), None, _p(cnt)), INVALID, "null output")
        _refused(lib, fn(None, _p(q), -1, 12, 5, _p(idx), _p(sqd), _p(cnt)), INVALID, "nq")
        for stride in (0, 8, 14, -12):
            _refused(lib, fn(None, _p(q), 4, stride, 5, _p(idx), _p(sqd), _p(cnt)), INVALID, "stride_bytes")
        _refused(lib, fn(None, _p(q), 4, 12, 5, _p(idx), _p(sqd), _p(cnt)), INVALID, "null handle")
    assert (idx == 0).all() and (sqd == 0).all() and (cnt == 0).all()


def test_radius_arguments_refused_before_any_device_call(lib):
    q = np.zeros((4, 3), np.float32)
    cnt = np.zeros(4, np.int32)
    total = C.c_longlong(-7)
    for fn in (lib.gorio_search_radius, lib.gorio_search_radius_device):
        for r in (0.0, -1.0, float("nan"), float("inf"), float("-inf")):
            _refused(lib, fn(None, _p(q), 4, 12, C.c_double(r), 0, _p(cnt), C.byref(total)), INVALID, "radius")
        _refused(lib, fn(None, _p(q), 4, 12, C.c_double(1.0), -1, _p(cnt), C.byref(total)), INVALID, "max_nn")
        _refused(lib, fn(None, _p(q), 4, 12, C.c_double(1.0), 0, _p(cnt), None), INVALID, "null total")
        _refused(lib, fn(None, _p(q), -2, 12, C.c_double(1.0), 0, _p(cnt), C.byref(total)), INVALID, "nq")
        _refused(lib, fn(None, _p(q), 4, 10, C.c_double(1.0), 0, _p(cnt), C.byref(total)), INVALID, "stride_bytes")
        _refused(lib, fn(None, _p(q), 4, 12, C.c_double(1.0), 0, _p(cnt), C.byref(total)), INVALID, "null handle")
    assert total.value == -7
    _refused(lib, lib.gorio_search_radius_get(None, None, None, None, C.c_longlong(0)), INVALID, "null handle")


def test_cloud_arguments_refused_before_any_device_call(lib):
    xyz = np.zeros((4, 3), np.float32)
    _refused(lib, lib.gorio_search_set_cloud(None, _p(xyz), -1, 12), INVALID, "bad cloud")
    _refused(lib, lib.gorio_search_set_cloud(None, None, 4, 12), INVALID, "bad cloud")
    _refused(lib, lib.gorio_search_set_cloud(None, _p(xyz), 4, 6), INVALID, "bad cloud")
    _refused(lib, lib.gorio_search_set_cloud(None, _p(xyz), 4, 12), INVALID, "null handle")
    _refused(lib, lib.gorio_search_set_cloud_device(None, None, None, None, 4), INVALID, "bad cloud")
    _refused(lib, lib.gorio_search_set_cloud_from_apd(None, None, 0), INVALID, "null argument")
    _refused(lib, lib.gorio_search_set_cloud_from_keyframe(None, None, 0), INVALID, "null argument")
    _refused(lib, lib.gorio_search_get_counters(None, None, None, None), INVALID, "null handle")
    _refused(lib, lib.gorio_search_cloud_size(None, None), INVALID, "null argument")
    _refused(lib, lib.gorio_search_create(None, 0), INVALID, "null argument")
    h = C.c_void_p()
    _refused(lib, lib.gorio_search_create(C.byref(h), -1), INVALID, "device")
    lib.gorio_search_destroy(None)  # a no-op


def test_no_cpu_fallback_without_device(gorio, lib):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    assert lib.gorio_search_create(C.byref(h), 0) == NO_DEVICE
    assert not h.value
    with pytest.raises(gorio.GorioError):
        gorio.Search()


def test_dropin_and_driver_build(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/search_sequence"])
    assert os.path.exists(os.path.join(HOST, "test", "search_sequence"))
