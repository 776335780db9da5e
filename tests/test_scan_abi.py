"""include/gorio_scan.h without a GPU: the symbols, the documented defaults, and the argument and state checks that come before any device call."""
import ctypes as C

import numpy as np

import scan_pipeline_restatement as sr

INVALID, STATE = -1, -3


def test_symbols_exist(gorio):
    lib = gorio.load_library()
    for name in gorio.prep.SCAN_SYMBOLS:
        assert hasattr(lib, name), name


def test_status_codes_are_those_of_gorio_apd_h(gorio):
    import os
    import re

    text = open(os.path.join(gorio.INCLUDE_DIR, "gorio_apd.h")).read()
    codes = dict((k, int(v)) for k, v in re.findall(r"(GORIO_ERR_[A-Z_]+)\s*=\s*(-?\d+)", text))
    assert codes["GORIO_ERR_INVALID"] == INVALID and codes["GORIO_ERR_STATE"] == STATE


def test_default_params_are_the_nodelets(gorio):
    p = gorio.prep.scan_default_params()
    d = sr.default_params()
    assert p.power_threshold == 0.0 and np.array_equal(np.array(p.rotation[:]).reshape(3, 3), np.eye(3))
    assert p.enable_dynamic_object_removal == 0 and p.deskew == 1 and p.scan_period == 0.1
    assert (p.distance_near, p.distance_far, p.z_low, p.z_high) == (1.0, 100.0, -5.0, 20.0)
    assert p.outlier_method == gorio.prep.OUTLIER_STATISTICAL and (p.mean_k, p.stddev_mul, p.radius, p.min_neighbors) == (20, 1.0, 2.0, 2)
    assert p.ground == 1 and (p.dbscan_core_min_pts, p.dbscan_eps, p.dbscan_min_cluster_size, p.dbscan_max_cluster_size) == (10, 0.9, 20, 25000)
    for k in ("power_threshold", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul", "radius", "min_neighbors",
              "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size"):
        assert getattr(p, k) == getattr(d, k), k
    assert bool(p.enable_dynamic_object_removal) == d.enable_dynamic_object_removal and bool(p.deskew) == d.deskew and bool(p.ground) == d.ground
    g, r = gorio.ground.default_params(), gorio.prep.reve_default_config()  # the nested structs are their own defaults: the layout lines up
    assert bytes(p.ground_params) == bytes(g) and bytes(p.reve) == bytes(r)
    assert p.reve.n_ransac_points == 5 and p.ground_params.num_iter == 4


def _err(lib):
    lib.gorio_scan_last_error.restype = C.c_char_p
    return lib.gorio_scan_last_error().decode()


def test_bad_arguments_are_refused_before_any_device_call(gorio):
    lib = gorio.load_library()
    P = gorio.prep.scan_default_params
    h = C.c_void_p()
    assert lib.gorio_scan_create(None, 0, C.byref(P())) == INVALID and lib.gorio_scan_create(C.byref(h), 0, None) == INVALID
    assert lib.gorio_scan_create(C.byref(h), -1, C.byref(P())) == INVALID
    for kw in (dict(outlier_method=7), dict(mean_k=0), dict(mean_k=32), dict(distance_far=float("inf")), dict(z_low=float("nan")), dict(outlier_method=2, radius=0.0),
               dict(outlier_method=2, min_neighbors=-1), dict(scan_period=float("inf"))):
        assert lib.gorio_scan_create(C.byref(h), 0, C.byref(P(**kw))) == INVALID and not h.value, kw
        assert "create" in _err(lib)
    bad = P()
    bad.reve.n_ransac_points = 2
    assert lib.gorio_scan_create(C.byref(h), 0, C.byref(bad)) == INVALID
    bad = P()
    bad.rotation[4] = float("nan")
    assert lib.gorio_scan_create(C.byref(h), 0, C.byref(bad)) == INVALID

    assert lib.gorio_scan_create(C.byref(h), 0, C.byref(P())) == 0 and h.value  # parameters only: the device side is made by the first load
    pts = np.ones((4, 5), np.float32)
    base = pts.__array_interface__["data"][0]
    x, pw, dp = C.c_void_p(base), C.c_void_p(base + 12), C.c_void_p(base + 16)
    ng, nv = C.c_int(7), C.c_int(7)
    load = lib.gorio_scan_load
    assert load(None, x, pw, dp, 4, 20, C.byref(ng), C.byref(nv)) == INVALID
    assert load(h, None, pw, dp, 4, 20, C.byref(ng), C.byref(nv)) == INVALID and load(h, x, None, dp, 4, 20, C.byref(ng), C.byref(nv)) == INVALID
    assert load(h, x, pw, None, 4, 20, C.byref(ng), C.byref(nv)) == INVALID and load(h, x, pw, dp, -1, 20, C.byref(ng), C.byref(nv)) == INVALID
    assert load(h, x, pw, dp, 4, 18, C.byref(ng), C.byref(nv)) == INVALID and load(h, x, pw, dp, 4, 0, C.byref(ng), C.byref(nv)) == INVALID
    assert load(h, x, pw, dp, 4, 20, None, C.byref(nv)) == INVALID and load(h, x, pw, dp, 4, 20, C.byref(ng), None) == INVALID
    assert "load" in _err(lib)
    res = gorio.prep.ScanResult()
    assert lib.gorio_scan_run(None, None, 0, None, C.byref(res)) == INVALID and lib.gorio_scan_run(h, None, 0, None, None) == INVALID
    assert lib.gorio_scan_run(h, None, 3, None, C.byref(res)) == INVALID and lib.gorio_scan_run(h, None, -1, None, C.byref(res)) == INVALID
    cnt = C.c_int(5)
    assert lib.gorio_scan_get_stage(h, 6, None, 0, C.byref(cnt)) == INVALID and lib.gorio_scan_get_stage(h, -1, None, 0, C.byref(cnt)) == INVALID
    assert lib.gorio_scan_get_stage(h, 0, None, 0, None) == INVALID and lib.gorio_scan_get_stage(None, 0, None, 0, C.byref(cnt)) == INVALID
    assert lib.gorio_scan_get_stage(h, 3, None, 0, C.byref(cnt)) == 0 and cnt.value == 0  # nothing ran: every stage is empty
    assert lib.gorio_scan_get_counters(None, None, None, None) == INVALID
    u, b, d = C.c_longlong(9), C.c_longlong(9), C.c_longlong(9)
    assert lib.gorio_scan_get_counters(h, C.byref(u), C.byref(b), C.byref(d)) == 0 and (u.value, b.value, d.value) == (0, 0, 0)
    assert lib.gorio_scan_get_output(h, None, None, None, None, 6, 0) == INVALID and lib.gorio_scan_get_output(None, None, None, None, None, 24, 0) == INVALID
    assert lib.gorio_apd_set_source_from_scan(None, h) == INVALID and lib.gorio_apd_set_target_from_scan(None, h) == INVALID
    lib.gorio_scan_destroy(h)
    lib.gorio_scan_destroy(None)


def test_run_and_reads_before_a_load_are_state_errors(gorio):
    lib = gorio.load_library()
    h = C.c_void_p()
    assert lib.gorio_scan_create(C.byref(h), 0, C.byref(gorio.prep.scan_default_params())) == 0
    res = gorio.prep.ScanResult()
    assert lib.gorio_scan_run(h, None, 0, None, C.byref(res)) == STATE and "gorio_scan_load" in _err(lib)
    out = np.zeros((4, 6), np.float32)
    assert lib.gorio_scan_get_output(h, C.c_void_p(out.__array_interface__["data"][0]), None, None, None, 24, 4) == STATE
    lib.gorio_scan_destroy(h)
