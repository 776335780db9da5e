"""ctypes binding of include/gorio_search.h: exact batched k-NN and radius queries against a cloud resident on the GPU (no numerics
here, no CPU fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

SEARCH_SYMBOLS = ["gorio_search_create", "gorio_search_destroy", "gorio_search_set_cloud", "gorio_search_set_cloud_device", "gorio_search_set_cloud_from_apd",
                  "gorio_search_set_cloud_from_keyframe", "gorio_search_cloud_size", "gorio_search_get_counters", "gorio_search_knn", "gorio_search_knn_device",
                  "gorio_search_radius", "gorio_search_radius_device", "gorio_search_radius_batch", "gorio_search_radius_get", "gorio_search_last_error"]
MAX_K = 32


def _ptr(a):
    return C.c_void_p(a.__array_interface__["data"][0])


def _queries(q):
    if q is None:
        return None, None
    q = np.ascontiguousarray(q, np.float32).reshape(-1, 3)
    return q, (q if q.shape[0] else np.zeros((1, 3), np.float32))


class Search:
    """gorio_search_t: one cloud on one GPU with its exact index, answering k-NN and radius queries for arbitrary points.  The
    *_device methods take raw device addresses (ints)."""

    def __init__(self, device=0):
        self.lib = load_library()
        self.lib.gorio_search_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self._check(self.lib.gorio_search_create(C.byref(self.h), int(device)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_search_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_search_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the cloud
    def set_cloud(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        buf = xyz if xyz.shape[0] else np.zeros((1, 3), np.float32)
        self._check(self.lib.gorio_search_set_cloud(self.h, _ptr(buf), int(xyz.shape[0]), 12))

    def set_cloud_device(self, d_x, d_y, d_z, n):
        self._check(self.lib.gorio_search_set_cloud_device(self.h, C.c_void_p(d_x), C.c_void_p(d_y), C.c_void_p(d_z), int(n)))

    def set_cloud_from_apd(self, reg, which):
        """The source (which = 0) or target (1) an ApdGicp holds now, shared: no point copy, no second index."""
        self._check(self.lib.gorio_search_set_cloud_from_apd(self.h, reg._h, int(which)))

    def set_cloud_from_keyframe(self, store, kid):
        self._check(self.lib.gorio_search_set_cloud_from_keyframe(self.h, store.h, int(kid)))

    def cloud_size(self):
        n = C.c_int(0)
        self._check(self.lib.gorio_search_cloud_size(self.h, C.byref(n)))
        return n.value

    def counters(self):
        u, b, d = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.gorio_search_get_counters(self.h, C.byref(u), C.byref(b), C.byref(d)))
        return dict(point_uploads=u.value, index_builds=b.value, result_downloads=d.value)

    # ---- k-NN
    def knn(self, queries, k):
        """(idx [nq, k] int32, sqd [nq, k] float32, count [nq] int32); queries None = the cloud's own points in original order."""
        q, buf = _queries(queries)
        nq = self.cloud_size() if q is None else q.shape[0]
        idx = np.zeros((max(nq, 1), max(int(k), 1)), np.int32)
        sqd = np.zeros((max(nq, 1), max(int(k), 1)), np.float32)
        cnt = np.zeros(max(nq, 1), np.int32)
        self._check(self.lib.gorio_search_knn(self.h, None if q is None else _ptr(buf), nq, 12, int(k), _ptr(idx), _ptr(sqd), _ptr(cnt)))
        return idx[:nq], sqd[:nq], cnt[:nq]

    def knn_device(self, d_q, nq, stride_bytes, k, d_idx, d_sqd, d_count):
        """Enqueues on the device's launch stream and returns; d_q 0 / None = the cloud's own points."""
        self._check(self.lib.gorio_search_knn_device(self.h, C.c_void_p(d_q) if d_q else None, int(nq), int(stride_bytes), int(k), C.c_void_p(d_idx), C.c_void_p(d_sqd),
                                                     C.c_void_p(d_count) if d_count else None))

    # ---- radius
    def radius(self, queries, radius, max_nn=0):
        """Runs the search and keeps the CSR on the device; returns (count [nq] int32, total)."""
        q, buf = _queries(queries)
        nq = self.cloud_size() if q is None else q.shape[0]
        cnt = np.zeros(max(nq, 1), np.int32)
        total = C.c_longlong(-1)
        self._check(self.lib.gorio_search_radius(self.h, None if q is None else _ptr(buf), nq, 12, C.c_double(radius), int(max_nn), _ptr(cnt), C.byref(total)))
        self._r_nq = nq
        return cnt[:nq], total.value

    def radius_device(self, d_q, nq, stride_bytes, radius, max_nn=0):
        cnt = np.zeros(max(int(nq), 1), np.int32)
        total = C.c_longlong(-1)
        self._check(self.lib.gorio_search_radius_device(self.h, C.c_void_p(d_q) if d_q else None, int(nq), int(stride_bytes), C.c_double(radius), int(max_nn), _ptr(cnt),
                                                        C.byref(total)))
        self._r_nq = int(nq)
        return cnt[:nq], total.value

    def radius_get(self, total, capacity=None):
        """(offsets [nq + 1] int64, idx [total] int32, sqd [total] float32) of the last radius call."""
        cap = int(total if capacity is None else capacity)
        offs = np.zeros(self._r_nq + 1, np.int64)
        idx = np.zeros(max(cap, 1), np.int32)
        sqd = np.zeros(max(cap, 1), np.float32)
        self._check(self.lib.gorio_search_radius_get(self.h, _ptr(offs), _ptr(idx), _ptr(sqd), C.c_longlong(cap)))
        return offs, idx[:total], sqd[:total]

    @staticmethod
    def radius_batch(searches, queries, radius, max_nn=0):
        """gorio_search_radius_batch: job j = searches[j].radius(queries[j], radius[j], max_nn[j]) followed by radius_get, all jobs in one
        set of launches.  queries: one array (or None: the cloud's own points) per job; radius / max_nn: one value per job, or a scalar
        for all.  Returns per job (count [nq] int32, total, offsets [nq + 1] int64, idx [total] int32, sqd [total] float32)."""
        n = len(searches)
        if n == 0:
            return []
        lib = searches[0].lib
        radius = [float(radius)] * n if np.isscalar(radius) else [float(r) for r in radius]
        max_nn = [int(max_nn)] * n if np.isscalar(max_nn) else [int(m) for m in max_nn]
        qs = [_queries(q) for q in queries]
        nq = [s.cloud_size() if q is None else q.shape[0] for s, (q, _) in zip(searches, qs)]
        cnt = [np.zeros(max(k, 1), np.int32) for k in nq]
        hs = (C.c_void_p * n)(*[s.h for s in searches])
        qp = (C.c_void_p * n)(*[None if q is None else _ptr(buf) for q, buf in qs])
        cp = (C.c_void_p * n)(*[_ptr(c) for c in cnt])
        totals = (C.c_longlong * n)(*([-1] * n))
        rc = lib.gorio_search_radius_batch(hs, n, qp, (C.c_int * n)(*nq), (C.c_int * n)(*([12] * n)), (C.c_double * n)(*radius), (C.c_int * n)(*max_nn), cp, totals)
        searches[0]._check(rc)
        out = []
        for j, s in enumerate(searches):
            s._r_nq = nq[j]
            out.append((cnt[j][:nq[j]], int(totals[j])) + s.radius_get(int(totals[j])))
        return out
