"""CPU-side checks of the radius-neighbourhood boundary of include/gorio_ndt.h: the new entries exist in the library and in the binding,
refuse NULL handles before any device is touched, and gorio_ndt_params did not grow (the switch is a call of its own, KDTREE stays a
refused value of params.search)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gorio_ndt_set_radius_search", "gorio_ndt_get_radius_search", "gorio_ndt_get_centroids", "gorio_ndt_get_neighbours")


def test_new_symbols_exist_and_refuse_null_handles(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    for name in NEW:
        assert name in gorio.NDT_SYMBOLS and hasattr(lib, name), name
    e, n = C.c_int(7), C.c_int(7)
    assert lib.gorio_ndt_set_radius_search(None, 1) == -1  # GORIO_ERR_INVALID
    assert b"set_radius_search" in lib.gorio_ndt_last_error()
    assert lib.gorio_ndt_get_radius_search(None, C.byref(e)) == -1 and e.value == 7
    assert lib.gorio_ndt_get_centroids(None, 0, C.byref(n), None, None) == -1 and n.value == 7
    assert lib.gorio_ndt_get_neighbours(None, None, None, None, C.c_longlong(0)) == -1


def test_params_struct_did_not_grow(gorio):
    txt = open(os.path.join(ROOT, "include", "gorio_ndt.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} gorio_ndt_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"^\s*(?:double|int)\s+(\w+);", body, flags=re.M)
    assert fields == ["resolution", "step_size", "outlier_ratio", "transformation_epsilon", "max_iterations", "search", "min_points_per_voxel", "min_covar_eigvalue_mult"]
    assert [f for f, _ in gorio.ndt.NdtParams._fields_] == fields and C.sizeof(gorio.ndt.NdtParams) == 56
    enum = re.search(r"enum gorio_ndt_search \{(.*?)\}", txt).group(1)
    assert dict(re.findall(r"GORIO_NDT_(\w+) = (\d)", enum)) == dict(KDTREE="0", DIRECT26="1", DIRECT7="2", DIRECT1="3")


def test_kdtree_refusal_names_the_new_call(gorio):
    lib = gorio.load_library()
    lib.gorio_ndt_last_error.restype = C.c_char_p
    p = gorio.ndt.default_params()
    p.search = gorio.ndt.KDTREE
    assert lib.gorio_ndt_set_params(None, C.byref(p)) == -5  # GORIO_ERR_UNSUPPORTED, as before
    assert b"gorio_ndt_set_radius_search" in lib.gorio_ndt_last_error()


def test_round_launch_bound_is_the_headers(gorio):
    f = gorio.ndt.radius_round_launch_bound
    assert [f(n) for n in (1, 4096, 4097, 8192, 8193, 16384)] == [14, 14, 16, 16, 19, 19]
