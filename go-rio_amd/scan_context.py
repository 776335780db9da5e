"""ctypes binding of include/gorio_sc.h: the Intensity Scan Context loop-candidate search on the GPU (no numerics here, no CPU
fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

SC_SYMBOLS = ["gorio_sc_add_scans", "gorio_sc_create", "gorio_sc_default_params", "gorio_sc_destroy", "gorio_sc_detect", "gorio_sc_detect_batch",
              "gorio_sc_distance", "gorio_sc_get_descriptor", "gorio_sc_get_state", "gorio_sc_last_error"]
# include/gorio_sc_pairs.h, the exhaustive section (an extension: listed pairs, matrices, best matches, detect without the tree)
SC_PAIRS_SYMBOLS = ["gorio_sc_best_matches", "gorio_sc_detect_exhaustive", "gorio_sc_distance_matrix", "gorio_sc_distance_pairs", "gorio_sc_pairs_counters"]
# include/gorio_sc_cross.h, the cross-database section (an extension as well: the same calls between two handles, the K best per keyframe)
SC_CROSS_SYMBOLS = ["gorio_sc_cross_counters", "gorio_sc_cross_detect", "gorio_sc_cross_distance_matrix", "gorio_sc_cross_distance_pairs", "gorio_sc_cross_top_matches"]
TOP_MAX = 8  # GORIO_SC_TOP_MAX
RINGS, SECTORS = 40, 20
EXCLUDE_RECENT = 10  # GORIO_SC_EXCLUDE_RECENT
TILE_ROWS, TILE_COLS, PAIRS_PER_GROUP = 8, 8, 4  # GORIO_SC_TILE_ROWS, GORIO_SC_TILE_COLS, GORIO_SC_PAIRS_PER_GROUP


class ScParams(C.Structure):
    _fields_ = [("sc_dist_thresh", C.c_double), ("azimuth_range", C.c_double)]


class ScDiag(C.Structure):
    _fields_ = [("early_return", C.c_int), ("rebuilt", C.c_int), ("counter", C.c_int), ("snapshot_size", C.c_int), ("n_found", C.c_int),
                ("position", C.c_int * 3), ("key_dist", C.c_float * 3), ("keyframe", C.c_int * 3), ("sc_dist", C.c_double * 3), ("sc_shift", C.c_int * 3)]


def _ptr(a):
    return C.c_void_p(a.__array_interface__["data"][0])


def diag_dict(d):
    out = {}
    for name, _ in d._fields_:
        v = getattr(d, name)
        out[name] = np.array(v[:]) if hasattr(v, "_length_") else v
    out["key_dist"] = out["key_dist"].astype(np.float32)
    return out


def default_params():
    lib = load_library()
    p = ScParams()
    lib.gorio_sc_default_params(C.byref(p))
    return p


def _points(xyz, intensity):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    pts = np.zeros((max(xyz.shape[0], 1), 4), np.float32)
    pts[:xyz.shape[0], :3] = xyz
    pts[:xyz.shape[0], 3] = np.asarray(intensity, np.float32).reshape(-1)
    return pts, xyz.shape[0]


class ScanContext:
    """SCManager (include/scan_context/Scancontext.h) on the GPU: a keyframe database of descriptors plus the loop-candidate
    search with its tree-making counter and snapshot."""

    def __init__(self, params=None, device=0, **overrides):
        self.lib = load_library()
        self.lib.gorio_sc_last_error.restype = C.c_char_p
        p = default_params() if params is None else params
        for k, v in overrides.items():
            setattr(p, k, v)
        self.params = p
        self.h = C.c_void_p()
        self._check(self.lib.gorio_sc_create(C.byref(self.h), int(device), C.byref(p)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_sc_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_sc_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_scans(self, clouds):
        """makeAndSaveScancontextAndKeys for every (xyz [n, 3], intensity [n]) in order, one launch; returns the first index."""
        k = len(clouds)
        pts = [_points(x, i) for x, i in clouds]
        X = (C.c_void_p * k)(*[p.__array_interface__["data"][0] for p, _ in pts])
        I = (C.c_void_p * k)(*[p.__array_interface__["data"][0] + 12 for p, _ in pts])
        N = (C.c_int * k)(*[n for _, n in pts])
        S = (C.c_int * k)(*([16] * k))
        first = C.c_int(-1)
        self._check(self.lib.gorio_sc_add_scans(self.h, k, X, I, N, S, C.byref(first)))
        return first.value

    def add_keyframes(self, store, ids):
        """makeAndSaveScancontextAndKeys for the listed entries of a keyframes.KeyframeStore, in order, without a host copy; returns the
        first index."""
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        first = C.c_int(-1)
        self._check(self.lib.gorio_sc_add_keyframes(self.h, store.h, _ptr(ids) if ids.size else None, int(ids.size), C.byref(first)))
        return first.value

    def add_scan(self, xyz, intensity):
        return self.add_scans([(xyz, intensity)])

    def state(self):
        n, c, m = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.gorio_sc_get_state(self.h, C.byref(n), C.byref(c), C.byref(m), None, 0))
        snap = np.zeros(max(m.value, 1), np.int32)
        self._check(self.lib.gorio_sc_get_state(self.h, None, None, None, _ptr(snap), snap.shape[0]))
        return {"n_scans": n.value, "counter": c.value, "snapshot": snap[:m.value].copy()}

    def descriptor(self, index):
        """(desc [40, 20], ring_key [40], sector_key [20]) of a stored keyframe, float64."""
        d = np.zeros((RINGS, SECTORS), np.float64)
        r = np.zeros(RINGS, np.float64)
        s = np.zeros(SECTORS, np.float64)
        self._check(self.lib.gorio_sc_get_descriptor(self.h, int(index), _ptr(d), _ptr(r), _ptr(s)))
        return d, r, s

    def distance(self, i, j):
        """distanceBtnScanContext(desc[i], desc[j]) -> (dist, shift)."""
        dist, shift = C.c_double(), C.c_int()
        self._check(self.lib.gorio_sc_distance(self.h, int(i), int(j), C.byref(dist), C.byref(shift)))
        return dist.value, shift.value

    def detect(self, query_index, candidates):
        """detectLoopClosureID -> (loop_id, yaw_rad (float32), min_dist, diag dict)."""
        cand = np.ascontiguousarray(candidates, np.int32).reshape(-1)
        lid, yaw, md = C.c_int(), C.c_float(), C.c_double()
        d = ScDiag()
        self._check(self.lib.gorio_sc_detect(self.h, int(query_index), _ptr(cand) if cand.size else None, int(cand.size), C.byref(lid), C.byref(yaw), C.byref(md),
                                             C.byref(d)))
        return lid.value, np.float32(yaw.value), md.value, diag_dict(d)

    def detect_batch(self, query_indices, candidate_lists):
        """`count` detect calls in order in one device pass -> list of (loop_id, yaw_rad, min_dist, diag dict)."""
        k = len(query_indices)
        cands = [np.ascontiguousarray(c, np.int32).reshape(-1) for c in candidate_lists]
        Q = (C.c_int * k)(*[int(q) for q in query_indices])
        P = (C.c_void_p * k)(*[c.__array_interface__["data"][0] if c.size else None for c in cands])
        N = (C.c_int * k)(*[c.size for c in cands])
        lid, yaw, md = (C.c_int * k)(), (C.c_float * k)(), (C.c_double * k)()
        d = (ScDiag * k)()
        self._check(self.lib.gorio_sc_detect_batch(self.h, k, Q, P, N, lid, yaw, md, d))
        return [(lid[i], np.float32(yaw[i]), md[i], diag_dict(d[i])) for i in range(k)]

    # ---- include/gorio_sc_pairs.h: every value is, bit for bit, what distance() gives for the pair
    def _indices(self, a):
        if a is None:
            return None, self.state()["n_scans"]
        a = np.ascontiguousarray(a, np.int32).reshape(-1)
        return a, int(a.size)

    def _pairs(self, name, fn, handles, q, c):
        q = np.ascontiguousarray(q, np.int32).reshape(-1)
        c = np.ascontiguousarray(c, np.int32).reshape(-1)
        if q.size != c.size:
            raise ValueError(f"{name}: q and c differ in length")
        dist, shift = np.zeros(q.size, np.float64), np.zeros(q.size, np.int32)
        self._check(fn(*handles, _ptr(q), _ptr(c), int(q.size), _ptr(dist), _ptr(shift)))
        return dist, shift

    def _matrix(self, fn, other, rows, cols, want_dist, want_shift):
        """other None: the one-handle call, whose columns are this handle's and which takes no second handle before them."""
        r, nr = self._indices(rows)
        c, nc = (self if other is None else other)._indices(cols)
        dist = np.zeros((nr, nc), np.float64) if want_dist else None
        shift = np.zeros((nr, nc), np.int32) if want_shift else None
        col_handle = [] if other is None else [other.h]
        self._check(fn(self.h, None if r is None else _ptr(r), nr, *col_handle, None if c is None else _ptr(c), nc,
                       None if dist is None else _ptr(dist), None if shift is None else _ptr(shift)))
        return dist, shift

    def _detect_lists(self, name, fn, handles, query_indices, candidate_lists):
        k = len(query_indices)
        cands = [np.ascontiguousarray(c, np.int32).reshape(-1) for c in candidate_lists]
        if len(cands) != k:
            raise ValueError(f"{name}: one candidate list per query")
        Q = (C.c_int * k)(*[int(q) for q in query_indices])
        P = (C.c_void_p * k)(*[c.__array_interface__["data"][0] if c.size else None for c in cands])
        N = (C.c_int * k)(*[c.size for c in cands])
        lid, yaw, md = (C.c_int * k)(), (C.c_float * k)(), (C.c_double * k)()
        self._check(fn(*handles, k, Q, P, N, lid, yaw, md))
        return [(lid[i], np.float32(yaw[i]), md[i]) for i in range(k)]

    def _counters(self, fn):
        v = [C.c_longlong() for _ in range(4)]
        self._check(fn(self.h, *[C.byref(x) for x in v]))
        return dict(zip(("calls", "pairs", "launches", "synchronisations"), [x.value for x in v]))

    def distance_pairs(self, q, c):
        """d(q[k], c[k]) for listed pairs in one launch -> (dist [count] float64, shift [count] int32)."""
        return self._pairs("distance_pairs", self.lib.gorio_sc_distance_pairs, (self.h,), q, c)

    def distance_matrix(self, rows=None, cols=None, want_dist=True, want_shift=True):
        """d(rows[i], cols[j]) for every pair -> (dist [n_rows, n_cols] float64, shift int32); None for rows / cols means every scan,
        an output not wanted comes back as None."""
        return self._matrix(self.lib.gorio_sc_distance_matrix, None, rows, cols, want_dist, want_shift)

    def best_matches(self, rows=None, min_gap=EXCLUDE_RECENT):
        """Per row r the minimum of d(r, c) over 0 <= c <= r - min_gap, ties to the lower c -> (index [n] int32, dist [n] float64,
        shift [n] int32); (-1, 1e7, 0) where there is no candidate or none scores below 1e7."""
        r, nr = self._indices(rows)
        idx, dist, shift = np.zeros(nr, np.int32), np.zeros(nr, np.float64), np.zeros(nr, np.int32)
        self._check(self.lib.gorio_sc_best_matches(self.h, None if r is None else _ptr(r), nr, int(min_gap), _ptr(idx), _ptr(dist), _ptr(shift)))
        return idx, dist, shift

    def detect_exhaustive(self, query_indices, candidate_lists):
        """detectLoopClosureID with the tree stage replaced by all candidates, for every query in one pass -> list of (loop_id, yaw_rad
        (float32), min_dist).  Stateless: counter and snapshot are untouched."""
        return self._detect_lists("detect_exhaustive", self.lib.gorio_sc_detect_exhaustive, (self.h,), query_indices, candidate_lists)

    def pairs_counters(self):
        return self._counters(self.lib.gorio_sc_pairs_counters)

    # ---- include/gorio_sc_cross.h: this handle is the query side, `other` the database side (only read); every value has the bits
    # distance() gives on a handle that holds both descriptors
    def cross_distance_pairs(self, other, q, c):
        """d(self[q[k]], other[c[k]]) for listed pairs in one launch -> (dist [count] float64, shift [count] int32)."""
        return self._pairs("cross_distance_pairs", self.lib.gorio_sc_cross_distance_pairs, (self.h, other.h), q, c)

    def cross_distance_matrix(self, other, rows=None, cols=None, want_dist=True, want_shift=True):
        """d(self[rows[i]], other[cols[j]]) for every pair -> (dist [n_rows, n_cols] float64, shift int32); None for rows means every scan
        of this handle, for cols every scan of `other`; an output not wanted comes back as None."""
        return self._matrix(self.lib.gorio_sc_cross_distance_matrix, other, rows, cols, want_dist, want_shift)

    def top_matches(self, other=None, rows=None, col_end=None, k=3):
        """Per row r of this handle the k best of d(r, c) over the scans 0 <= c < col_end[i] of `other` (None: this handle itself; col_end
        None: every scan), ascending in (dist, index) -> (index [n, k] int32, dist [n, k] float64, shift [n, k] int32); slots beyond what
        scores below 1e7 hold (-1, 1e7, 0)."""
        other = self if other is None else other
        r, nr = self._indices(rows)
        e = None if col_end is None else np.ascontiguousarray(col_end, np.int32).reshape(-1)
        if e is not None and e.size != nr:
            raise ValueError("top_matches: one col_end per row")
        k = int(k)
        kk = max(k, 0)
        idx, dist, shift = np.zeros((nr, kk), np.int32), np.zeros((nr, kk), np.float64), np.zeros((nr, kk), np.int32)
        self._check(self.lib.gorio_sc_cross_top_matches(self.h, None if r is None else _ptr(r), nr, other.h, None if e is None else _ptr(e), k, _ptr(idx), _ptr(dist),
                                                        _ptr(shift)))
        return idx, dist, shift

    def cross_detect(self, other, query_indices, candidate_lists):
        """For every query of this handle the strict minimum of d(query, c) over its list of `other`'s scans, in list order, with this
        handle's threshold -> list of (loop_id, yaw_rad (float32), min_dist).  No early return, no recent-keyframe filter."""
        return self._detect_lists("cross_detect", self.lib.gorio_sc_cross_detect, (self.h, other.h), query_indices, candidate_lists)

    def cross_counters(self):
        return self._counters(self.lib.gorio_sc_cross_counters)
