"""ctypes binding of include/gorio_ndt.h: NDT_OMP registration (pclomp::NormalDistributionsTransform, DIRECT1 / 7 / 26) and the radius
neighbourhood of pcl::NormalDistributionsTransform / pclomp's KDTREE on the GPU (no numerics here, no CPU fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

NDT_SYMBOLS = ["gorio_ndt_align", "gorio_ndt_align_batch", "gorio_ndt_calculate_score", "gorio_ndt_calculate_score_batch", "gorio_ndt_create", "gorio_ndt_default_params",
               "gorio_ndt_derivatives", "gorio_ndt_destroy", "gorio_ndt_get_capacities", "gorio_ndt_get_centroids", "gorio_ndt_get_neighbours", "gorio_ndt_get_params",
               "gorio_ndt_get_radius_search", "gorio_ndt_get_voxels", "gorio_ndt_hessian", "gorio_ndt_last_error", "gorio_ndt_set_params", "gorio_ndt_set_radius_search", "gorio_ndt_set_source", "gorio_ndt_set_source_device", "gorio_ndt_set_source_from_scan", "gorio_ndt_set_target", "gorio_ndt_set_target_device",
               "gorio_ndt_set_target_from_apd", "gorio_ndt_set_target_from_scan", "gorio_ndt_set_target_shared"]
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3  # pclomp::NeighborSearchMethod


class NdtParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("step_size", C.c_double), ("outlier_ratio", C.c_double), ("transformation_epsilon", C.c_double),
                ("max_iterations", C.c_int), ("search", C.c_int), ("min_points_per_voxel", C.c_int), ("min_covar_eigvalue_mult", C.c_double)]


class NdtDiag(C.Structure):
    _fields_ = [("n_derivatives", C.c_int), ("n_hessians", C.c_int), ("n_mt_iterations", C.c_int), ("score", C.c_double)]


class NdtBatchStats(C.Structure):
    """What one align_batch did: lock-step rounds (device round trips), evaluations summed over the handles, kernel launches."""
    _fields_ = [("rounds", C.c_int), ("evaluations", C.c_int), ("launches", C.c_int)]


def _ptr(a):
    return C.c_void_p(a.__array_interface__["data"][0])


def default_params():
    lib = load_library()
    p = NdtParams()
    lib.gorio_ndt_default_params(C.byref(p))
    return p


def radius_round_launch_bound(max_radius_source):
    """Launches one round of align_batch may take when handles with the radius switch on take part (include/gorio_ndt.h): 14 + s,
    s = 0 up to 4096 points in the largest such source, m (m + 3) / 2 for 4096 * 2^m."""
    m = 0
    while 4096 << m < int(max_radius_source):
        m += 1
    return 14 + m * (m + 3) // 2


class Ndt:
    """pclomp::NormalDistributionsTransform on the GPU; keyword arguments are fields of gorio_ndt_params.  radius_search=True makes it
    pcl::NormalDistributionsTransform (pclomp's KDTREE): every neighbourhood is the radius search over the leaf centroids."""

    def __init__(self, device=0, radius_search=False, **params):
        self.lib = load_library()
        self.lib.gorio_ndt_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self._n_source = None  # known for sources set from the host or from device arrays
        self._check(self.lib.gorio_ndt_create(C.byref(self.h), int(device)))
        if params:
            self.set_params(**params)
        if radius_search:
            self.set_radius_search(True)

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_ndt_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_ndt_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_params(self):
        p = NdtParams()
        self._check(self.lib.gorio_ndt_get_params(self.h, C.byref(p)))
        return p

    def set_params(self, **params):
        p = self.get_params()
        for k, v in params.items():
            setattr(p, k, v)
        self._check(self.lib.gorio_ndt_set_params(self.h, C.byref(p)))

    def set_radius_search(self, enable):
        """Switch the radius neighbourhood on or off; params.search is kept and rules again when it is off."""
        self._check(self.lib.gorio_ndt_set_radius_search(self.h, int(bool(enable))))

    def get_radius_search(self):
        e = C.c_int()
        self._check(self.lib.gorio_ndt_get_radius_search(self.h, C.byref(e)))
        return bool(e.value)

    def centroids(self):
        """The centroid cloud of the radius mode: (xyz float32 [C, 3], leaf_pos int32 [C]: the centroid's leaf in voxels() order)."""
        n = C.c_int()
        self._check(self.lib.gorio_ndt_get_centroids(self.h, 0, C.byref(n), None, None))
        c = n.value
        xyz, pos = np.zeros((max(c, 1), 3), np.float32), np.zeros(max(c, 1), np.int32)
        self._check(self.lib.gorio_ndt_get_centroids(self.h, max(c, 1), C.byref(n), _ptr(xyz), _ptr(pos)))
        return xyz[:c], pos[:c]

    def neighbours(self, n_source=None):
        """The CSR of the last radius evaluation: (offsets int64 [source size + 1], leaf_pos int32 [total], sqd float32 [total]).
        n_source: the source's size, needed when the source came from a scan pipeline or a keyframe store."""
        n_source = self._n_source if n_source is None else int(n_source)
        if n_source is None:
            raise ValueError("neighbours: pass n_source for a source that was handed over on the device")
        offs = np.zeros(n_source + 1, np.int64)
        self._check(self.lib.gorio_ndt_get_neighbours(self.h, _ptr(offs), None, None, 0))
        total = int(offs[-1])
        pos, sqd = np.zeros(max(total, 1), np.int32), np.zeros(max(total, 1), np.float32)
        self._check(self.lib.gorio_ndt_get_neighbours(self.h, _ptr(offs), _ptr(pos), _ptr(sqd), max(total, 1)))
        return offs, pos[:total], sqd[:total]

    def set_target(self, xyz):
        a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._check(self.lib.gorio_ndt_set_target(self.h, _ptr(a) if a.size else None, a.shape[0], 12))

    def set_source(self, xyz):
        a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._check(self.lib.gorio_ndt_set_source(self.h, _ptr(a) if a.size else None, a.shape[0], 12))
        self._n_source = a.shape[0]

    def set_target_shared(self, owner):
        """This handle's target becomes owner's current target: points and voxel map exist once on the device."""
        self._check(self.lib.gorio_ndt_set_target_shared(self.h, owner.h))

    def set_target_device(self, x, y, z, n):
        """x, y, z: device addresses (int) of float arrays of the handle's device."""
        self._check(self.lib.gorio_ndt_set_target_device(self.h, C.c_void_p(x), C.c_void_p(y), C.c_void_p(z), int(n)))

    def set_source_device(self, x, y, z, n):
        self._check(self.lib.gorio_ndt_set_source_device(self.h, C.c_void_p(x), C.c_void_p(y), C.c_void_p(z), int(n)))
        self._n_source = int(n)

    def set_source_from_scan(self, scan):
        """The output of a prep.ScanPipeline's last OK run becomes the source: one device-to-device copy, no host round trip."""
        self._check(self.lib.gorio_ndt_set_source_from_scan(self.h, scan.h))
        self._n_source = None

    def set_target_from_scan(self, scan):
        self._check(self.lib.gorio_ndt_set_target_from_scan(self.h, scan.h))

    def set_target_from_apd(self, apd):
        """The current target of a registration object (apd.ApdGicp: what setInputTargetSubmap assembled, say) becomes the target."""
        self._check(self.lib.gorio_ndt_set_target_from_apd(self.h, apd._h))

    def set_source_from_keyframe(self, store, kid):
        """A keyframes.KeyframeStore entry becomes the source: one device-to-device copy of x, y, z."""
        self._check(self.lib.gorio_ndt_set_source_from_keyframe(self.h, store.h, int(kid)))
        self._n_source = None

    def set_target_from_keyframe(self, store, kid):
        self._check(self.lib.gorio_ndt_set_target_from_keyframe(self.h, store.h, int(kid)))

    def capacities(self):
        """Elements the device buffers hold: dict of target, source, leaves, keys."""
        c = (C.c_longlong * 4)()
        self._check(self.lib.gorio_ndt_get_capacities(self.h, c))
        return {"target": c[0], "source": c[1], "leaves": c[2], "keys": c[3]}

    def voxels(self):
        """The leaves in ascending leaf index: dict of leaf_index, nr_points, mean [L, 3], cov_raw / cov / icov [L, 3, 3], min_b, div_b."""
        n = C.c_int()
        min_b, div_b = np.zeros(3, np.int32), np.zeros(3, np.int32)
        self._check(self.lib.gorio_ndt_get_voxels(self.h, 0, C.byref(n), None, None, None, None, None, None, _ptr(min_b), _ptr(div_b)))
        L = n.value
        idx, cnt = np.zeros(max(L, 1), np.int32), np.zeros(max(L, 1), np.int32)
        mean = np.zeros((max(L, 1), 3))
        raw, cov, icov = (np.zeros((max(L, 1), 3, 3)) for _ in range(3))
        self._check(self.lib.gorio_ndt_get_voxels(self.h, max(L, 1), C.byref(n), _ptr(idx), _ptr(cnt), _ptr(mean), _ptr(raw), _ptr(cov), _ptr(icov), None, None))
        return {"leaf_index": idx[:L], "nr_points": cnt[:L], "mean": mean[:L], "cov_raw": raw[:L], "cov": cov[:L], "icov": icov[:L], "min_b": min_b, "div_b": div_b}

    def derivatives(self, p, compute_hessian=True):
        """computeDerivatives at pose vector p -> (score, gradient [6], hessian [6, 6] or None)."""
        p = np.ascontiguousarray(p, np.float64).reshape(6)
        s = C.c_double()
        g, H = np.zeros(6), np.zeros((6, 6))
        self._check(self.lib.gorio_ndt_derivatives(self.h, _ptr(p), int(bool(compute_hessian)), C.byref(s), _ptr(g), _ptr(H) if compute_hessian else None))
        return s.value, g, (H if compute_hessian else None)

    def hessian(self, p):
        """computeHessian at pose vector p -> [6, 6]."""
        p = np.ascontiguousarray(p, np.float64).reshape(6)
        H = np.zeros((6, 6))
        self._check(self.lib.gorio_ndt_hessian(self.h, _ptr(p), _ptr(H)))
        return H

    def calculate_score(self, T):
        T = np.ascontiguousarray(T, np.float32).reshape(4, 4)
        s = C.c_double()
        self._check(self.lib.gorio_ndt_calculate_score(self.h, _ptr(T), C.byref(s)))
        return s.value

    def align(self, guess=None):
        """computeTransformation -> dict: T (float32 4x4), converged, nr_iterations, trans_probability, n_derivatives, n_hessians, n_mt, score."""
        g = None if guess is None else np.ascontiguousarray(guess, np.float32).reshape(4, 4)
        T = np.zeros((4, 4), np.float32)
        conv, nr, prob, d = C.c_int(), C.c_int(), C.c_double(), NdtDiag()
        self._check(self.lib.gorio_ndt_align(self.h, None if g is None else _ptr(g), _ptr(T), C.byref(conv), C.byref(nr), C.byref(prob), C.byref(d)))
        return _result(T, conv.value, nr.value, prob.value, d)


def _result(T, conv, nr, prob, d):
    return {"T": T, "converged": bool(conv), "nr_iterations": int(nr), "trans_probability": float(prob), "n_derivatives": d.n_derivatives,
            "n_hessians": d.n_hessians, "n_mt": d.n_mt_iterations, "score": d.score}


def align_batch(handles, guesses=None):
    """computeTransformation for every handle (Ndt objects of one device) in lock-step through ONE gorio_ndt_align_batch.
    guesses: None (identity for all) or one 4x4 per handle.  Returns (results, stats): results[i] is the dict Ndt.align returns for
    handles[i], bit for bit; stats is an NdtBatchStats."""
    handles = list(handles)
    count = len(handles)
    stats = NdtBatchStats()
    if count == 0:
        return [], stats
    lib = handles[0].lib
    g = None
    if guesses is not None:
        g = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in guesses]), np.float32)
        if g.shape[0] != count:
            raise ValueError("align_batch: one guess per handle")
    hs = (C.c_void_p * count)(*[h.h.value for h in handles])
    T = np.zeros((count, 4, 4), np.float32)
    conv, nr = np.zeros(count, np.int32), np.zeros(count, np.int32)
    prob = np.zeros(count, np.float64)
    diag = (NdtDiag * count)()
    handles[0]._check(lib.gorio_ndt_align_batch(hs, count, None if g is None else _ptr(g), _ptr(T), _ptr(conv), _ptr(nr), _ptr(prob), diag, C.byref(stats)))
    return [_result(T[i].copy(), conv[i], nr[i], prob[i], diag[i]) for i in range(count)], stats


def calculate_score_batch(handles, Ts=None):
    """calculateScore for every handle (Ndt objects of one device) through ONE gorio_ndt_calculate_score_batch.  Ts: None (identity for
    all) or one 4x4 per handle.  Returns a float64 array: element i is what handles[i].calculate_score(Ts[i]) returns, bit for bit."""
    handles = list(handles)
    count = len(handles)
    score = np.zeros(count, np.float64)
    if count == 0:
        return score
    lib = handles[0].lib
    t = None
    if Ts is not None:
        t = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(4, 4) for x in Ts]), np.float32)
        if t.shape[0] != count:
            raise ValueError("calculate_score_batch: one transform per handle")
    hs = (C.c_void_p * count)(*[h.h.value for h in handles])
    handles[0]._check(lib.gorio_ndt_calculate_score_batch(hs, count, None if t is None else _ptr(t), _ptr(score)))
    return score
