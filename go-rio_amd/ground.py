"""ctypes binding of include/gorio_ground.h: Patchwork++ ground segmentation on the GPU (no numerics here, no CPU fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

GROUND_SYMBOLS = ["gorio_ground_create", "gorio_ground_default_params", "gorio_ground_destroy", "gorio_ground_estimate", "gorio_ground_estimate_batch",
                  "gorio_ground_get_diagnostics", "gorio_ground_get_state", "gorio_ground_last_error", "gorio_ground_set_state"]
MAX_FITS = 9
DECISIONS = {0: "skipped", 1: "not_upright", 2: "far", 3: "heading", 4: "flat", 5: "tgr_revert", 6: "tgr_reject"}


class GroundParams(C.Structure):
    _fields_ = [("enable_RNR", C.c_int), ("enable_RVPF", C.c_int), ("enable_TGR", C.c_int), ("num_iter", C.c_int), ("num_lpr", C.c_int), ("num_min_pts", C.c_int),
                ("RNR_ver_angle_thr", C.c_double), ("RNR_intensity_thr", C.c_double), ("sensor_height", C.c_double), ("th_seeds", C.c_double),
                ("th_dist", C.c_double), ("th_seeds_v", C.c_double), ("th_dist_v", C.c_double), ("max_range", C.c_double), ("min_range", C.c_double),
                ("uprightness_thr", C.c_double), ("adaptive_seed_selection_margin", C.c_double), ("num_sectors_each_zone", C.c_int * 4),
                ("num_rings_each_zone", C.c_int * 4), ("max_flatness_storage", C.c_int), ("max_elevation_storage", C.c_int), ("elevation_thr", C.c_double * 4),
                ("flatness_thr", C.c_double * 4)]


class PatchDiag(C.Structure):
    _fields_ = [("zone", C.c_int), ("ring", C.c_int), ("sector", C.c_int), ("concentric_idx", C.c_int), ("n_points", C.c_int), ("segment_offset", C.c_int),
                ("n_ground", C.c_int), ("decision", C.c_int), ("uprightness", C.c_double), ("elevation", C.c_double), ("flatness", C.c_double),
                ("line_variable", C.c_double), ("heading", C.c_double), ("mean", C.c_float * 3), ("cov", C.c_float * 9), ("singular_values", C.c_float * 3),
                ("normal", C.c_float * 3), ("d", C.c_float), ("n_fits", C.c_int), ("fit_points", C.c_int * MAX_FITS), ("lm_iterations", C.c_int * MAX_FITS),
                ("lm_termination", C.c_int * MAX_FITS)]


class FrameDiag(C.Structure):
    _fields_ = [("n_points", C.c_int), ("n_noise", C.c_int), ("n_out_of_range", C.c_int), ("n_patches", C.c_int), ("n_ground", C.c_int), ("n_erased", C.c_int),
                ("final_fit_points", C.c_int), ("final_lm_iterations", C.c_int), ("final_lm_termination", C.c_int), ("final_mean", C.c_float * 3),
                ("final_cov", C.c_float * 9), ("final_singular_values", C.c_float * 3), ("final_normal", C.c_float * 3), ("final_d", C.c_float)]


def _ptr(a):
    return C.c_void_p(a.__array_interface__["data"][0])


def _struct_dict(s):
    out = {}
    for name, _ in s._fields_:
        v = getattr(s, name)
        out[name] = np.array(v[:]) if hasattr(v, "_length_") else v
    return out


def default_params():
    lib = load_library()
    p = GroundParams()
    lib.gorio_ground_default_params(C.byref(p))
    return p


def _points(xyz, intensity):
    xyz = np.asarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [n, 3]")
    pts = np.zeros((xyz.shape[0], 4), np.float32)
    pts[:, :3] = xyz
    pts[:, 3] = np.asarray(intensity, np.float32).reshape(-1)
    return pts


class GroundSegmenter:
    """PatchWorkpp<PointT> (include/patchworkpp/patchworkpp.hpp) on the GPU: estimate() returns (ground_idx, nonground_idx), indices
    into the input in the reference's cloud_ground / cloud_nonground order."""

    def __init__(self, params=None, device=0, **overrides):
        self.lib = load_library()
        self.lib.gorio_ground_last_error.restype = C.c_char_p
        p = default_params() if params is None else params
        for k, v in overrides.items():
            if isinstance(getattr(p, k), C.Array):
                getattr(p, k)[:] = list(v)
            else:
                setattr(p, k, v)
        self.params = p
        self.h = C.c_void_p()
        self._check(self.lib.gorio_ground_create(C.byref(self.h), int(device), C.byref(p)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_ground_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_ground_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, xyz, intensity, id=1):
        pts = _points(xyz, intensity)
        n = pts.shape[0]
        order = np.full(max(n, 1), -1, np.int32)
        ng, no = C.c_int(0), C.c_int(0)
        self._check(self.lib.gorio_ground_estimate(self.h, _ptr(pts), C.c_void_p(pts.__array_interface__["data"][0] + 12), n, 16, int(id), _ptr(order), C.byref(ng),
                                                   C.byref(no)))
        return order[:ng.value].copy(), order[ng.value:no.value].copy()

    def get_state(self, stride=1000):
        e, f = (C.c_double * 4)(), (C.c_double * 4)()
        sh = C.c_double()
        ec, fc = (C.c_int * 4)(), (C.c_int * 4)()
        self._check(self.lib.gorio_ground_get_state(self.h, e, f, C.byref(sh), None, ec, None, fc, 0))
        stride = max(stride, max(ec[:] + fc[:]), 1)
        es = np.zeros((4, stride), np.float64)
        fs = np.zeros((4, stride), np.float64)
        self._check(self.lib.gorio_ground_get_state(self.h, e, f, C.byref(sh), _ptr(es), ec, _ptr(fs), fc, stride))
        return {"elevation_thr": np.array(e[:]), "flatness_thr": np.array(f[:]), "sensor_height": sh.value,
                "update_elevation": [es[r, :ec[r]].copy() for r in range(4)], "update_flatness": [fs[r, :fc[r]].copy() for r in range(4)]}

    def set_state(self, elevation_thr, flatness_thr, sensor_height, update_elevation=None, update_flatness=None):
        ue = [np.asarray(v, np.float64) for v in (update_elevation or [[]] * 4)]
        uf = [np.asarray(v, np.float64) for v in (update_flatness or [[]] * 4)]
        stride = max([len(v) for v in ue + uf] + [1])
        es = np.zeros((4, stride), np.float64)
        fs = np.zeros((4, stride), np.float64)
        for r in range(4):
            es[r, :len(ue[r])] = ue[r]
            fs[r, :len(uf[r])] = uf[r]
        ec = (C.c_int * 4)(*[len(v) for v in ue])
        fc = (C.c_int * 4)(*[len(v) for v in uf])
        self._check(self.lib.gorio_ground_set_state(self.h, (C.c_double * 4)(*elevation_thr), (C.c_double * 4)(*flatness_thr), C.c_double(sensor_height), _ptr(es), ec,
                                                    _ptr(fs), fc, stride))

    def diagnostics(self):
        fd = FrameDiag()
        self._check(self.lib.gorio_ground_get_diagnostics(self.h, C.byref(fd), None, 0, None, None, 0))
        n, P = fd.n_points, fd.n_patches
        pd = (PatchDiag * P)()
        label = np.zeros(n, np.int32)
        order = np.zeros(n, np.int32)
        self._check(self.lib.gorio_ground_get_diagnostics(self.h, None, pd, P, _ptr(label), _ptr(order), n))
        return {"frame": _struct_dict(fd), "patches": [_struct_dict(p) for p in pd], "point_label": label, "patch_order": order}


def estimate_batch(segmenters, clouds, id=1):
    """One launch over the patches of every (segmenter, (xyz, intensity)) pair; returns [(ground_idx, nonground_idx)]."""
    lib = load_library()
    lib.gorio_ground_last_error.restype = C.c_char_p
    k = len(segmenters)
    pts = [_points(x, i) for x, i in clouds]
    orders = [np.full(max(p.shape[0], 1), -1, np.int32) for p in pts]
    H = (C.c_void_p * k)(*[s.h.value for s in segmenters])
    X = (C.c_void_p * k)(*[p.__array_interface__["data"][0] for p in pts])
    I = (C.c_void_p * k)(*[p.__array_interface__["data"][0] + 12 for p in pts])
    N = (C.c_int * k)(*[p.shape[0] for p in pts])
    S = (C.c_int * k)(*([16] * k))
    O = (C.c_void_p * k)(*[o.__array_interface__["data"][0] for o in orders])
    ng, no = (C.c_int * k)(), (C.c_int * k)()
    rc = lib.gorio_ground_estimate_batch(H, k, X, I, N, S, int(id), O, ng, no)
    if rc < 0:
        msg = lib.gorio_ground_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return [(o[:ng[q]].copy(), o[ng[q]:no[q]].copy()) for q, o in enumerate(orders)]
