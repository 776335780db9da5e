"""include/gorio_keyframes.h without a GPU: the symbols, and the argument and state checks that come before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

INVALID, NO_DEVICE, STATE = -1, -2, -3


def _declared(gorio, header):
    txt = open(os.path.join(gorio.INCLUDE_DIR, header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))


def test_every_symbol_is_exported_and_bound(gorio):
    lib = gorio.load_library()
    names = _declared(gorio, "gorio_keyframes.h")
    assert len(names) == 17
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(gorio.keyframes.KF_SYMBOLS) == names
    # every consumer is a method of the class that takes the keyframe
    for cls, methods in ((gorio.ApdGicp, ("setInputSourceKeyframe", "setInputTargetKeyframe", "setInputTargetSubmapKeyframes")),
                         (gorio.Ndt, ("set_source_from_keyframe", "set_target_from_keyframe")), (gorio.ScanContext, ("add_keyframes",)),
                         (gorio.KeyframeStore, ("add", "add_from_scan", "add_from_apd", "release", "count", "info", "get", "counters"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)


def test_info_struct_matches_the_header(gorio):
    txt = open(os.path.join(gorio.INCLUDE_DIR, "gorio_keyframes.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} gorio_kf_info_t;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in re.findall(r"int\s+([^;]+);", body) for f in decl.split(",")]
    assert fields == [k for k, _ in gorio.keyframes.KeyframeInfo._fields_]
    assert C.sizeof(gorio.keyframes.KeyframeInfo) == 4 * len(fields)


def _err(lib):
    lib.gorio_kf_last_error.restype = C.c_char_p
    return lib.gorio_kf_last_error().decode()


def test_bad_arguments_are_refused_before_any_device_call(gorio):
    lib = gorio.load_library()
    h = C.c_void_p()
    assert lib.gorio_kf_create(None, 0) == INVALID
    assert lib.gorio_kf_create(C.byref(h), -1) == INVALID and not h.value and "create" in _err(lib)
    assert lib.gorio_kf_create(C.byref(h), 0) == 0 and h.value  # arguments only: the device side is made by the first add
    pts = np.ones((4, 5), np.float32)
    base = pts.__array_interface__["data"][0]
    x, it, lb = C.c_void_p(base), C.c_void_p(base + 12), C.c_void_p(base + 16)
    kid = C.c_int(77)
    add = lib.gorio_kf_add
    assert add(None, x, it, lb, 4, 20, C.byref(kid)) == INVALID and add(h, x, it, lb, 4, 20, None) == INVALID
    assert add(h, None, it, lb, 4, 20, C.byref(kid)) == INVALID and add(h, x, it, lb, -1, 20, C.byref(kid)) == INVALID
    assert add(h, x, it, lb, 4, 8, C.byref(kid)) == INVALID and add(h, x, it, lb, 4, 18, C.byref(kid)) == INVALID
    assert "add" in _err(lib) and kid.value == 77
    assert lib.gorio_kf_add_from_scan(h, None, C.byref(kid)) == INVALID and lib.gorio_kf_add_from_scan(None, None, C.byref(kid)) == INVALID
    assert lib.gorio_kf_add_from_apd(h, None, 0, None, 4, C.byref(kid)) == INVALID
    # ids: nothing has been added, so every id is out of range
    info = gorio.keyframes.KeyframeInfo()
    for bad in (-1, 0, 3):
        assert lib.gorio_kf_release(h, bad) == INVALID and "has not been added" in _err(lib)
        assert lib.gorio_kf_info(h, bad, C.byref(info)) == INVALID
        assert lib.gorio_kf_get(h, bad, x, None, None, 20, 4) == INVALID
    assert lib.gorio_kf_release(None, 0) == INVALID and lib.gorio_kf_info(h, 0, None) == INVALID and lib.gorio_kf_info(None, 0, C.byref(info)) == INVALID
    assert lib.gorio_kf_get(None, 0, x, None, None, 20, 4) == INVALID and lib.gorio_kf_get(h, 0, x, None, None, 8, 4) == INVALID
    assert lib.gorio_kf_get(h, 0, None, it, None, 6, 4) == INVALID and lib.gorio_kf_get(h, 0, x, None, None, 20, -1) == INVALID
    a, r = C.c_int(9), C.c_int(9)
    assert lib.gorio_kf_count(None, C.byref(a), C.byref(r)) == INVALID
    assert lib.gorio_kf_count(h, C.byref(a), C.byref(r)) == 0 and (a.value, r.value) == (0, 0)
    u, d, c = C.c_longlong(9), C.c_longlong(9), C.c_longlong(9)
    assert lib.gorio_kf_get_counters(None, None, None, None) == INVALID
    assert lib.gorio_kf_get_counters(h, C.byref(u), C.byref(d), C.byref(c)) == 0 and (u.value, d.value, c.value) == (0, 0, 0)
    # consumers: null handles and null stores
    ids = (C.c_int * 1)(0)
    T = (C.c_double * 16)(*np.eye(4).reshape(-1))
    n = C.c_int(5)
    assert lib.gorio_apd_set_source_from_keyframe(None, h, 0) == INVALID and lib.gorio_apd_set_target_from_keyframe(None, h, 0) == INVALID
    assert lib.gorio_apd_set_target_submap_keyframes(None, h, ids, T, 1, C.c_double(0.0), C.byref(n)) == INVALID
    assert lib.gorio_ndt_set_source_from_keyframe(None, h, 0) == INVALID and lib.gorio_ndt_set_target_from_keyframe(None, h, 0) == INVALID
    assert lib.gorio_sc_add_keyframes(None, h, ids, 1, None) == INVALID
    lib.gorio_kf_destroy(h)
    lib.gorio_kf_destroy(None)


def test_no_cpu_fallback_without_device(gorio):
    """Without a HIP device create succeeds (it stores its arguments), the first add refuses, and the Python class raises."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = gorio.load_library()
    h = C.c_void_p()
    assert lib.gorio_kf_create(C.byref(h), 0) == 0
    pts = np.ones((4, 3), np.float32)
    kid = C.c_int(-5)
    assert lib.gorio_kf_add(h, C.c_void_p(pts.__array_interface__["data"][0]), None, None, 4, 12, C.byref(kid)) == NO_DEVICE
    assert lib.gorio_kf_add(h, None, None, None, 0, 12, C.byref(kid)) == NO_DEVICE  # an empty keyframe needs the device side too
    assert kid.value == -5 and "no usable HIP device" in _err(lib)
    a, r = C.c_int(9), C.c_int(9)
    assert lib.gorio_kf_count(h, C.byref(a), C.byref(r)) == 0 and (a.value, r.value) == (0, 0)  # a failed call changes nothing
    lib.gorio_kf_destroy(h)
    store = gorio.KeyframeStore()
    with pytest.raises(gorio.GorioError) as e:
        store.add(pts)
    assert e.value.code == NO_DEVICE
    store.close()
