"""include/gorio_map.h without a GPU: the symbols, the info struct, and the argument and state checks that come before any device call.

One refusal the header lists cannot be met without a device: GORIO_ERR_NO_DEVICE from generate.  generate checks its arguments and ids
first (as the header promises), a valid id needs a keyframe, and a keyframe needs the device (gorio_kf_add refuses without one).  Without
a device generate therefore ends at "has not been added"; what is checked here is that it does, and that nothing changed after it.  The
same holds for a released id (GORIO_ERR_STATE): tests/test_map_cloud_gpu.py covers it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5


def _err(lib):
    lib.gorio_map_last_error.restype = C.c_char_p
    return lib.gorio_map_last_error().decode()


def test_every_symbol_is_exported_and_bound(gorio):
    lib = gorio.load_library()
    txt = open(os.path.join(gorio.INCLUDE_DIR, "gorio_map.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) == 8
    for name in names:
        assert hasattr(lib, name), name
    assert sorted(gorio.map_cloud.MAP_SYMBOLS) == names == sorted(gorio.MAP_SYMBOLS)
    for m in ("generate", "generate_only", "get", "info", "counters", "capacities", "close"):
        assert callable(getattr(gorio.MapCloud, m)), m


def test_info_struct_matches_the_header(gorio):
    txt = open(os.path.join(gorio.INCLUDE_DIR, "gorio_map.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} gorio_map_info_t;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, name, dim in re.findall(r"(int|double)\s+([a-z_0-9]+)(?:\[(\d+)\])?\s*;", body):
        base = C.c_int if ctype == "int" else C.c_double
        fields.append((name, base * int(dim) if dim else base))
    got = gorio.map_cloud.MapInfo._fields_
    assert [k for k, _ in fields] == [k for k, _ in got] == ["n_listed", "n_kept", "n_finite", "n_voxels", "anchor", "min_k", "max_k"]
    assert all(C.sizeof(a) == C.sizeof(b) and a._type_ == b._type_ if hasattr(a, "_length_") else a is b for (_, a), (_, b) in zip(fields, got))
    assert C.sizeof(gorio.map_cloud.MapInfo) == 4 * 4 + 3 * 8 + 6 * 4 and gorio.map_cloud.MapInfo.anchor.offset == 16


def _state(gorio, lib, m):
    info = gorio.map_cloud.MapInfo()
    assert lib.gorio_map_info(m, C.byref(info)) == 0
    g, d, u = C.c_longlong(9), C.c_longlong(9), C.c_longlong(9)
    assert lib.gorio_map_get_counters(m, C.byref(g), C.byref(d), C.byref(u)) == 0
    caps = (C.c_longlong * 6)(*([9] * 6))
    assert lib.gorio_map_get_capacities(m, caps) == 0
    return bytes(info), (g.value, d.value, u.value), list(caps)


def test_bad_arguments_are_refused_before_any_device_call(gorio):
    lib = gorio.load_library()
    m, kf, kf1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.gorio_map_create(None, 0) == INVALID
    assert lib.gorio_map_create(C.byref(m), -1) == INVALID and not m.value and "create" in _err(lib)
    assert lib.gorio_map_create(C.byref(m), 0) == 0 and m.value  # arguments only
    assert lib.gorio_kf_create(C.byref(kf), 0) == 0 and lib.gorio_kf_create(C.byref(kf1), 1) == 0
    fresh = _state(gorio, lib, m)
    assert fresh == (bytes(C.sizeof(gorio.map_cloud.MapInfo)), (0, 0, 0), [0] * 6)
    ids = (C.c_int * 2)(0, 1)
    T = (C.c_double * 32)(*np.tile(np.eye(4).reshape(-1), 2))
    n = C.c_int(77)
    gen = lib.gorio_map_generate
    res = C.c_double(0.05)
    # null arguments
    assert gen(None, kf, ids, T, 1, res, C.byref(n)) == INVALID and gen(m, None, ids, T, 1, res, C.byref(n)) == INVALID
    assert gen(m, kf, None, T, 1, res, C.byref(n)) == INVALID and gen(m, kf, ids, None, 1, res, C.byref(n)) == INVALID
    assert gen(m, kf, ids, T, 1, res, None) == INVALID and "null" in _err(lib)
    # count <= 0: the reference returns nullptr
    for count in (0, -3):
        assert gen(m, kf, ids, T, count, res, C.byref(n)) == INVALID and "count" in _err(lib)
    assert gen(m, kf, ids, T, 65536, res, C.byref(n)) == UNSUPPORTED
    # a NaN resolution; a non-finite pose entry in the rows that are read (the fourth row is not)
    assert gen(m, kf, ids, T, 1, C.c_double(np.nan), C.byref(n)) == INVALID and "resolution" in _err(lib)
    for bad in (np.nan, np.inf, -np.inf):
        Tb = (C.c_double * 32)(*T)
        Tb[16 + 7] = bad
        assert gen(m, kf, ids, Tb, 2, res, C.byref(n)) == INVALID and "pose 1" in _err(lib)
        assert gen(m, kf, ids, Tb, 1, res, C.byref(n)) == INVALID and "has not been added" in _err(lib)  # pose 1 is not read with count 1
    Tb = (C.c_double * 32)(*T)
    Tb[13] = np.nan  # row 3 is never read
    assert gen(m, kf, ids, Tb, 1, res, C.byref(n)) == INVALID and "has not been added" in _err(lib)
    # a store on another device
    assert gen(m, kf1, ids, T, 1, res, C.byref(n)) == INVALID and "one device" in _err(lib)
    # ids never added (nothing has been): with the text of the keyframe store
    for first in (0, -1, 5):
        ids[0] = first
        assert gen(m, kf, ids, T, 1, res, C.byref(n)) == INVALID and "keyframe %d has not been added (0 keyframes)" % first in _err(lib)
        assert gen(m, kf, ids, T, 1, C.c_double(0.0), C.byref(n)) == INVALID
    assert n.value == 77
    # get: null handle, stride, capacity; before the first generate it hands out 0 points and writes nothing
    out = np.full((4, 4), 5.0, np.float32)
    x, it = C.c_void_p(out.__array_interface__["data"][0]), C.c_void_p(out.__array_interface__["data"][0] + 12)
    get = lib.gorio_map_get
    assert get(None, x, it, 16, 4) == INVALID
    assert get(m, x, it, 8, 4) == INVALID and get(m, x, it, 18, 4) == INVALID and get(m, None, it, 2, 4) == INVALID and get(m, None, it, 6, 4) == INVALID
    assert get(m, x, it, 16, -1) == INVALID and "get" in _err(lib)
    assert get(m, x, it, 16, 4) == 0 and get(m, None, it, 4, 0) == 0 and get(m, None, None, 4, 0) == 0 and (out == 5.0).all()
    # the other calls
    info = gorio.map_cloud.MapInfo()
    assert lib.gorio_map_info(None, C.byref(info)) == INVALID and lib.gorio_map_info(m, None) == INVALID
    assert lib.gorio_map_get_counters(None, None, None, None) == INVALID and lib.gorio_map_get_counters(m, None, None, None) == 0
    caps = (C.c_longlong * 6)()
    assert lib.gorio_map_get_capacities(None, caps) == INVALID and lib.gorio_map_get_capacities(m, None) == INVALID
    assert _state(gorio, lib, m) == fresh  # a failed call changes nothing
    lib.gorio_map_destroy(m)
    lib.gorio_map_destroy(None)
    lib.gorio_kf_destroy(kf)
    lib.gorio_kf_destroy(kf1)


def test_no_cpu_fallback_without_device(gorio):
    """Without a HIP device no keyframe can exist, so generate ends at its id check and the class raises; nothing changes after it."""
    import torch

    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    if not torch.cuda.is_available():
        with pytest.raises(gorio.GorioError) as e:
            store.add(np.ones((4, 3), np.float32))
        assert e.value.code == NO_DEVICE
    n_added = store.count()[0]
    before = (mc.info(), mc.counters(), mc.capacities())
    for res in (0.05, 0.0):
        with pytest.raises(gorio.GorioError) as e:
            mc.generate(store, [n_added], [np.eye(4)], res)
        assert e.value.code == INVALID and "has not been added" in str(e.value)
    with pytest.raises(ValueError):
        mc.generate(store, [0, 1], [np.eye(4)], 0.05)
    assert (mc.info(), mc.counters(), mc.capacities()) == before
    xyz, inten = mc.get()
    assert xyz.shape == (0, 3) and inten.shape == (0,)
    mc.close()
    store.close()
