"""ctypes binding of include/gorio_keyframes.h: the keyframe store on the GPU (no numerics here, no CPU fallback).  The consumers are
methods of the classes that take a keyframe: ApdGicp.setInputSourceKeyframe / setInputTargetKeyframe / setInputTargetSubmapKeyframes,
Ndt.set_source_from_keyframe / set_target_from_keyframe, ScanContext.add_keyframes."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

KF_SYMBOLS = ["gorio_kf_create", "gorio_kf_destroy", "gorio_kf_add", "gorio_kf_add_from_scan", "gorio_kf_add_from_apd", "gorio_kf_release", "gorio_kf_count", "gorio_kf_info",
              "gorio_kf_get", "gorio_kf_get_counters", "gorio_kf_last_error", "gorio_apd_set_source_from_keyframe", "gorio_apd_set_target_from_keyframe",
              "gorio_ndt_set_source_from_keyframe", "gorio_ndt_set_target_from_keyframe", "gorio_apd_set_target_submap_keyframes", "gorio_sc_add_keyframes"]


KF_EDGE_SYMBOLS = ["gorio_kf_edge_fitness", "gorio_kf_default_inf_params", "gorio_kf_edge_information", "gorio_kf_edge_counters"]  # include/gorio_kf_edges.h

DBL_MAX = float(np.finfo(np.float64).max)


class KfEdge(C.Structure):
    """gorio_kf_edge (include/gorio_kf_edges.h)."""
    _fields_ = [("target_id", C.c_int), ("source_id", C.c_int), ("relpose", C.c_double * 16)]


class InfParams(C.Structure):
    """gorio_inf_params (include/gorio_kf_edges.h)."""
    _fields_ = [("use_const_inf_matrix", C.c_int)] + [(k, C.c_double) for k in ("const_stddev_x", "const_stddev_q", "var_gain_a", "min_stddev_x", "max_stddev_x", "min_stddev_q",
                                                                                 "max_stddev_q", "fitness_score_thresh")]


def edge_table(edges):
    """A gorio_kf_edge array from an iterable of (target_id, source_id, relpose 4 x 4)."""
    edges = list(edges)
    tab = (KfEdge * max(len(edges), 1))()
    for e, (tgt, src, T) in enumerate(edges):
        tab[e].target_id, tab[e].source_id = int(tgt), int(src)
        tab[e].relpose[:] = np.asarray(T, np.float64).reshape(16).tolist()
    return tab, len(edges)


class KeyframeInfo(C.Structure):
    """gorio_kf_info_t (include/gorio_keyframes.h)."""
    _fields_ = [(k, C.c_int) for k in ("n", "resident", "has_intensity", "cov_count", "cov_k", "cov_reg", "index_built", "sharers")]


def _ptr(a, offset=0):
    return C.c_void_p(a.__array_interface__["data"][0] + offset)


class KeyframeStore:
    """gorio_kf_t: keyframe clouds resident on one GPU under ids 0, 1, 2, ... (never reused)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.lib.gorio_kf_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self._check(self.lib.gorio_kf_create(C.byref(self.h), int(device)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_kf_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_kf_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, xyz, intensity=None, label=None):
        """A keyframe from host arrays: xyz [n, 3], intensity [n] or None, label [n] or None.  Returns its id."""
        xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
        n = xyz.shape[0]
        buf = np.zeros((max(n, 1), 5), np.float32)
        buf[:n, :3] = xyz
        if intensity is not None:
            buf[:n, 3] = np.asarray(intensity, np.float32).reshape(-1)
        if label is not None:
            buf[:n, 4] = np.asarray(label, np.float32).reshape(-1)
        kid = C.c_int(-1)
        self._check(self.lib.gorio_kf_add(self.h, _ptr(buf), _ptr(buf, 12) if intensity is not None else None, _ptr(buf, 16) if label is not None else None, n, 20, C.byref(kid)))
        return kid.value

    def add_from_scan(self, scan):
        """The output of a prep.ScanPipeline's last OK run, shared: no point is copied."""
        kid = C.c_int(-1)
        self._check(self.lib.gorio_kf_add_from_scan(self.h, scan.h, C.byref(kid)))
        return kid.value

    def add_from_apd(self, reg, which, intensity=None):
        """The source (which = 0) or target (1) an ApdGicp holds now, shared with its covariances, search index and voxel map."""
        col = None if intensity is None else np.ascontiguousarray(intensity, np.float32).reshape(-1)
        if col is not None and col.shape[0] != (reg._n_src if which == 0 else reg._n_tgt):
            raise ValueError("intensity must have one value per point")
        kid = C.c_int(-1)
        self._check(self.lib.gorio_kf_add_from_apd(self.h, reg._h, int(which), _ptr(col) if col is not None and col.size else None, 4, C.byref(kid)))
        return kid.value

    def release(self, kid):
        self._check(self.lib.gorio_kf_release(self.h, int(kid)))

    def count(self):
        a, r = C.c_int(0), C.c_int(0)
        self._check(self.lib.gorio_kf_count(self.h, C.byref(a), C.byref(r)))
        return a.value, r.value

    def info(self, kid):
        i = KeyframeInfo()
        self._check(self.lib.gorio_kf_info(self.h, int(kid), C.byref(i)))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def get(self, kid, intensity=True):
        """(xyz [n, 3], intensity [n] or None, label [n]) of a resident keyframe."""
        n = self.info(kid)["n"]
        buf = np.zeros((max(n, 1), 5), np.float32)
        self._check(self.lib.gorio_kf_get(self.h, int(kid), _ptr(buf), _ptr(buf, 12) if intensity else None, _ptr(buf, 16), 20, buf.shape[0]))
        buf = buf[:n]
        return buf[:, :3].copy(), (buf[:, 3].copy() if intensity else None), buf[:, 4].copy()

    def counters(self):
        u, d, c = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.gorio_kf_get_counters(self.h, C.byref(u), C.byref(d), C.byref(c)))
        return dict(point_uploads=u.value, point_downloads=d.value, device_copies=c.value)

    # pose-graph edges (include/gorio_kf_edges.h): edges = iterable of (target_id, source_id, relpose 4 x 4)
    def edge_fitness(self, edges, max_range=None):
        """InformationMatrixCalculator::calc_fitness_score for every edge in one pass: (score [count] float64, n_in_range [count] int64).
        max_range is the reference's (a squared distance); None = DBL_MAX."""
        tab, count = edge_table(edges)
        score = np.zeros(max(count, 1), np.float64)
        nr = np.zeros(max(count, 1), np.int64)
        self._check(self.lib.gorio_kf_edge_fitness(self.h, tab, count, C.c_double(DBL_MAX if max_range is None else max_range), _ptr(score), _ptr(nr)))
        return score[:count], nr[:count]

    def default_inf_params(self):
        p = InfParams()
        self.lib.gorio_kf_default_inf_params.restype = None
        self.lib.gorio_kf_default_inf_params(C.byref(p))
        return p

    def edge_information(self, edges, **params):
        """InformationMatrixCalculator::calc_information_matrix for every edge in one pass: (inf_diag [count, 2] = (1 / w_x, 1 / w_q), score
        [count]).  params: fields of gorio_inf_params that differ from the reference constructor's defaults."""
        p = self.default_inf_params()
        for k, v in params.items():
            if k not in dict(InfParams._fields_):
                raise TypeError(f"unknown information parameter {k!r}")
            setattr(p, k, int(v) if k == "use_const_inf_matrix" else float(v))
        tab, count = edge_table(edges)
        inf = np.zeros((max(count, 1), 2), np.float64)
        score = np.zeros(max(count, 1), np.float64)
        self._check(self.lib.gorio_kf_edge_information(self.h, C.byref(p), tab, count, _ptr(inf), _ptr(score)))
        return inf[:count], score[:count]

    def edge_counters(self):
        v = [C.c_longlong(0) for _ in range(4)]
        self._check(self.lib.gorio_kf_edge_counters(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "edges_scored", "index_builds", "synchronisations"), (x.value for x in v)))
