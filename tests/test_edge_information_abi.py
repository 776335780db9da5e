"""include/gorio_kf_edges.h without a GPU: the symbols and structs, every argument check (all of them come before any device call), the
constructor's defaults of InformationMatrixCalculator, the use_const_inf_matrix branch, and the host arithmetic from a score to the
information against a Python restatement (through the C++ driver's --weights mode: the ABI has no hook for it)."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

INVALID, NO_DEVICE, STATE, UNSUPPORTED = -1, -2, -3, -5
DBL_MAX = float(np.finfo(np.float64).max)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "edge_information_sequence")
SCORES = [0.0, 1e-3, 0.49, 0.5, 3.0, DBL_MAX]


def _header(gorio):
    return open(os.path.join(gorio.INCLUDE_DIR, "gorio_kf_edges.h")).read()


def _err(lib):
    lib.gorio_kf_last_error.restype = C.c_char_p
    return lib.gorio_kf_last_error().decode()


def restated_information(score, a=20.0, thresh=0.5, min_sx=0.1, max_sx=5.0, min_sq=0.05, max_sq=0.2):
    """information_matrix_calculator.cpp:39-49 with weight() of its header: double arithmetic, w rounded to float, 1 / w in double."""
    def weight(max_x, min_y, max_y, x):
        y = (1.0 - math.exp(-a * x)) / (1.0 - math.exp(-a * max_x))
        return min_y + (max_y - min_y) * y

    w_x = np.float32(weight(thresh, min_sx ** 2, max_sx ** 2, score))
    w_q = np.float32(weight(thresh, min_sq ** 2, max_sq ** 2, score))
    return 1.0 / float(w_x), 1.0 / float(w_q)


def test_symbols_and_structs_match_the_header(gorio):
    lib = gorio.load_library()
    txt = re.sub(r"/\*.*?\*/", "", _header(gorio), flags=re.S)
    names = sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))
    assert names == sorted(gorio.keyframes.KF_EDGE_SYMBOLS) == sorted(["gorio_kf_edge_fitness", "gorio_kf_default_inf_params", "gorio_kf_edge_information", "gorio_kf_edge_counters"])
    for name in names:
        assert hasattr(lib, name), name
    flat = " ".join(txt.split())
    assert "int gorio_kf_edge_fitness(gorio_kf_t* kf, const gorio_kf_edge* edges, int count, double max_range, double* score, long long* n_in_range);" in flat
    assert "void gorio_kf_default_inf_params(gorio_inf_params* p);" in flat
    assert "int gorio_kf_edge_information(gorio_kf_t* kf, const gorio_inf_params* p, const gorio_kf_edge* edges, int count, double* inf_diag, double* score);" in flat
    assert "int gorio_kf_edge_counters(const gorio_kf_t* kf, long long* calls, long long* edges_scored, long long* index_builds, long long* synchronisations);" in flat
    # the store's header brings the edge section with it
    assert '#include "gorio_kf_edges.h"' in open(os.path.join(gorio.INCLUDE_DIR, "gorio_keyframes.h")).read()
    # struct layouts as the header declares them
    edge = re.search(r"typedef struct \{([^{}]*)\} gorio_kf_edge;", txt).group(1)
    assert [f.strip() for f in edge.split(";") if f.strip()] == ["int target_id", "int source_id", "double relpose[16]"]
    assert [k for k, _ in gorio.keyframes.KfEdge._fields_] == ["target_id", "source_id", "relpose"] and C.sizeof(gorio.keyframes.KfEdge) == 8 + 128
    par = re.search(r"typedef struct \{([^{}]*)\} gorio_inf_params;", txt).group(1)
    fields = [f.strip() for decl in re.findall(r"(?:int|double)\s+([^;]+);", par) for f in decl.split(",")]
    assert fields == [k for k, _ in gorio.keyframes.InfParams._fields_] and C.sizeof(gorio.keyframes.InfParams) == 8 + 8 * 8
    for m in ("edge_fitness", "edge_information", "edge_counters"):
        assert callable(getattr(gorio.KeyframeStore, m)), m


def test_defaults_are_the_constructors(gorio):
    """information_matrix_calculator.cpp:15-24 (what the nodelet constructs), not the 2.5 of the header's unused load()."""
    lib = gorio.load_library()
    p = gorio.keyframes.InfParams()
    lib.gorio_kf_default_inf_params.restype = None
    lib.gorio_kf_default_inf_params(C.byref(p))
    assert p.use_const_inf_matrix == 0
    assert (p.const_stddev_x, p.const_stddev_q, p.var_gain_a) == (0.5, 0.1, 20.0)
    assert (p.min_stddev_x, p.max_stddev_x, p.min_stddev_q, p.max_stddev_q) == (0.1, 5.0, 0.05, 0.2)
    assert p.fitness_score_thresh == 0.5
    lib.gorio_kf_default_inf_params(None)  # tolerated


def test_every_argument_check_comes_before_the_device(gorio):
    """A store made by gorio_kf_create has no device side yet: every refusal below is reached on a machine without a GPU."""
    lib = gorio.load_library()
    K = gorio.keyframes
    h = C.c_void_p()
    assert lib.gorio_kf_create(C.byref(h), 0) == 0
    tab, _ = K.edge_table([(0, 0, np.eye(4))])
    score = (C.c_double * 2)(7.0, 7.0)
    nr = (C.c_longlong * 2)(7, 7)
    inf = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    p = K.InfParams()
    lib.gorio_kf_default_inf_params.restype = None
    lib.gorio_kf_default_inf_params(C.byref(p))
    big = C.c_double(DBL_MAX)
    fit, info, cnt = lib.gorio_kf_edge_fitness, lib.gorio_kf_edge_information, lib.gorio_kf_edge_counters
    # null arguments
    assert fit(None, tab, 1, big, score, nr) == INVALID and "edge_fitness" in _err(lib)
    assert fit(h, None, 1, big, score, nr) == INVALID and fit(h, tab, 1, big, None, nr) == INVALID
    assert info(None, C.byref(p), tab, 1, inf, score) == INVALID and "edge_information" in _err(lib)
    assert info(h, None, tab, 1, inf, score) == INVALID and info(h, C.byref(p), None, 1, inf, score) == INVALID and info(h, C.byref(p), tab, 1, None, score) == INVALID
    assert cnt(None, None, None, None, None) == INVALID
    # count
    assert fit(h, tab, -1, big, score, nr) == INVALID and info(h, C.byref(p), tab, -1, inf, score) == INVALID
    assert fit(h, None, 0, big, None, None) == 0 and info(h, C.byref(p), None, 0, None, None) == 0  # count == 0: nothing is looked at
    many = (K.KfEdge * 65536)()
    assert fit(h, many, 65536, big, (C.c_double * 65536)(), None) == UNSUPPORTED and "65535" in _err(lib)
    # ids never added (nothing has been): the text names the edge
    for tgt, src in ((0, 0), (-1, 0), (3, 5)):
        tab, _ = K.edge_table([(tgt, src, np.eye(4))])
        assert fit(h, tab, 1, big, score, nr) == INVALID and "edges[0]" in _err(lib) and "has not been added" in _err(lib)
        assert info(h, C.byref(p), tab, 1, inf, score) == INVALID and "edges[0]" in _err(lib)
    # NaN max_range
    assert fit(h, tab, 1, C.c_double(float("nan")), score, nr) == INVALID and "max_range" in _err(lib)
    # nothing was written, nothing was counted
    assert list(score) == [7.0, 7.0] and list(nr) == [7, 7] and list(inf) == [7.0] * 4
    v = [C.c_longlong(9) for _ in range(4)]
    assert cnt(h, *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [0, 0, 0, 0]
    assert cnt(h, None, None, None, None) == 0
    lib.gorio_kf_destroy(h)


def test_non_finite_relpose_is_refused(gorio):
    """INVALID without a device.  (Which entry the text names is checked where keyframes can exist: tests/test_edge_information_gpu.py.)"""
    lib = gorio.load_library()
    for bad in (float("nan"), float("inf"), -float("inf")):
        T = np.eye(4)
        T[1, 3] = bad
        h = C.c_void_p()
        assert lib.gorio_kf_create(C.byref(h), 0) == 0
        tab, _ = gorio.keyframes.edge_table([(0, 0, T)])
        assert lib.gorio_kf_edge_fitness(h, tab, 1, C.c_double(1.0), (C.c_double * 1)(), None) == INVALID
        lib.gorio_kf_destroy(h)


def test_const_information_needs_no_device_and_ignores_the_ids(gorio):
    store = gorio.KeyframeStore()  # no keyframe: every id is out of range, and nobody looks
    inf, _ = store.edge_information([(5, 9, np.eye(4)), (-3, 0, np.full((4, 4), np.nan))], use_const_inf_matrix=1)
    assert inf.tolist() == [[1 / 0.5, 1 / 0.1]] * 2  # divided by the standard deviations themselves, not their squares (IMC:32-33)
    inf, _ = store.edge_information([(0, 0, np.eye(4))], use_const_inf_matrix=True, const_stddev_x=0.25, const_stddev_q=4.0)
    assert inf.tolist() == [[4.0, 0.25]]
    assert store.edge_counters() == dict(calls=0, edges_scored=0, index_builds=0, synchronisations=0)
    with pytest.raises(TypeError):
        store.edge_information([], no_such_parameter=1)
    store.close()


def test_information_from_score_equals_the_restatement(gorio):
    """The library's host arithmetic (csrc/edge_information.h), printed by the driver for a table of scores, against math.exp / numpy.float32:
    the same libm on the same machine, so one ulp of a double and nothing more."""
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/edge_information_sequence"])
    r = subprocess.run([DRIVER, "--weights"] + [repr(s) for s in SCORES], capture_output=True, text=True, check=True)
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    assert len(lines) == len(SCORES)
    for s, l in zip(SCORES, lines):
        assert float.fromhex(l["score"]) == s
        rx, rq = restated_information(s)
        print(s, float.fromhex(l["inf_x"]), rx, float.fromhex(l["inf_q"]), rq)
        assert float.fromhex(l["inf_x"]) == pytest.approx(rx, rel=2.3e-16, abs=0.0)
        assert float.fromhex(l["inf_q"]) == pytest.approx(rq, rel=2.3e-16, abs=0.0)
        assert (float.fromhex(l["const_x"]), float.fromhex(l["const_q"])) == (1 / 0.5, 1 / 0.1)
    # what the table is there for: the variance runs from min^2 at a perfect fit to max^2 at the threshold; past it exp(-a x) is 0 (DBL_MAX included)
    x = [float.fromhex(l["inf_x"]) for l in lines]
    assert x[0] == pytest.approx(100.0, rel=1e-6) and x[3] == pytest.approx(1 / 25.0, rel=1e-6) and x[0] > x[1] > x[2] > x[3] >= x[4] == x[5] > 0.0
