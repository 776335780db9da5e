"""ctypes binding of include/gorio_prep.h: preprocessing steps that feed the hot path, on the GPU (no numerics here, no CPU fallback)."""
import ctypes as C

import numpy as np

from .apd import GorioError, load_library

PREP_SYMBOLS = ["gorio_prep_dbscan_labels", "gorio_prep_radius_outlier_mask", "gorio_prep_statistical_outlier_mask", "gorio_prep_voxel_downsample", "gorio_prep_approx_voxel_downsample", "gorio_prep_approx_voxel_downsample_device", "gorio_prep_last_error", "gorio_prep_reve_default_config", "gorio_prep_reve_ransac_iterations", "gorio_prep_ego_velocity"]


def dbscan_labels(xyz, eps=0.9, core_min_pts=10, min_cluster_size=20, max_cluster_size=25000, device=0):
    """preprocessing_nodelet_ntu.cpp:518-568 with the nodelet's parameters as defaults: returns (labels float32 [n], n_clusters)."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [n, 3]")
    n = xyz.shape[0]
    lab = np.zeros(n, np.float32)
    nc = C.c_int(0)
    rc = lib.gorio_prep_dbscan_labels(int(device), C.c_void_p(xyz.__array_interface__["data"][0]), n, 12, C.c_double(eps), int(core_min_pts), int(min_cluster_size),
                                      int(max_cluster_size), C.c_void_p(lab.__array_interface__["data"][0]), 4, C.byref(nc))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return lab, nc.value


def voxel_downsample(xyz, leaf=0.1, device=0):
    """pcl::VoxelGrid (preprocessing_nodelet_ntu.cpp:137-139, 608-622): centroids [m,3], ordered by voxel index."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    out = np.zeros((n, 3), np.float32)
    m = C.c_int(0)
    rc = lib.gorio_prep_voxel_downsample(int(device), C.c_void_p(xyz.__array_interface__["data"][0]), n, 12, C.c_double(leaf), C.c_void_p(out.__array_interface__["data"][0]), 12, n, C.byref(m))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return out[:m.value].copy()


def approx_voxel_downsample(points, leaf, device=0):
    """pcl::ApproximateVoxelGrid (include/gorio_prep.h): points [n, F] float32, 3 <= F <= 8, columns 0..2 = x y z, every column averaged;
    leaf a scalar or three values.  Returns the filtered [m, F] array in the filter's flush order.  A refused cloud raises GorioError(-1)."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    pts = np.ascontiguousarray(points, np.float32)
    if pts.ndim != 2:
        raise ValueError("points must be [n, F]")
    n, nf = pts.shape
    lf = np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, np.float64).reshape(-1), (3,)), np.float64)
    offs = np.arange(nf, dtype=np.int32)
    out = np.zeros((max(n, 1), max(nf, 1)), np.float32)
    m = C.c_int(0)
    rc = lib.gorio_prep_approx_voxel_downsample(int(device), _ptr(pts) if n else None, n, 4 * nf, _ptr(offs), nf, _ptr(lf), _ptr(out), 4 * nf, n, C.byref(m))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return out[:m.value].copy()


def radius_outlier_mask(xyz, radius=2.0, min_neighbors=2, device=0):
    """pcl::RadiusOutlierRemoval (preprocessing_nodelet_ntu.cpp:163-171): boolean keep mask [n]."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [n, 3]")
    n = xyz.shape[0]
    keep = np.zeros(n, np.uint8)
    nk = C.c_int(0)
    rc = lib.gorio_prep_radius_outlier_mask(int(device), C.c_void_p(xyz.__array_interface__["data"][0]), n, 12, C.c_double(radius), int(min_neighbors),
                                            C.c_void_p(keep.__array_interface__["data"][0]), C.byref(nk))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return keep.astype(bool)


def statistical_outlier_mask(xyz, mean_k=20, stddev_mul=1.0, device=0, return_distances=False):
    """pcl::StatisticalOutlierRemoval (preprocessing_nodelet_ntu.cpp:153-162, the nodelet's default filter): boolean keep mask [n]
    (and, on request, the per-point mean neighbour distances)."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    xyz = np.ascontiguousarray(xyz, np.float32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [n, 3]")
    n = xyz.shape[0]
    keep = np.zeros(n, np.uint8)
    dist = np.zeros(n, np.float32)
    nk = C.c_int(0)
    rc = lib.gorio_prep_statistical_outlier_mask(int(device), C.c_void_p(xyz.__array_interface__["data"][0]), n, 12, int(mean_k), C.c_double(stddev_mul),
                                                 C.c_void_p(keep.__array_interface__["data"][0]), C.byref(nk), C.c_void_p(dist.__array_interface__["data"][0]))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return (keep.astype(bool), dist) if return_distances else keep.astype(bool)


class ReveConfig(C.Structure):
    """gorio_reve_config (include/gorio_prep.h) == RadarEgoVelocityEstimatorConfig (radar_ego_velocity_estimator.h:30-60)."""
    _fields_ = [(k, C.c_float) for k in (
        "min_dist", "max_dist", "min_db", "elevation_thresh_deg", "azimuth_thresh_deg", "doppler_velocity_correction_factor", "thresh_zero_velocity",
        "allowed_outlier_percentage", "sigma_zero_velocity_x", "sigma_zero_velocity_y", "sigma_zero_velocity_z", "sigma_offset_radar_x", "sigma_offset_radar_y",
        "sigma_offset_radar_z", "max_sigma_x", "max_sigma_y", "max_sigma_z", "inlier_thresh")] + [("use_ransac", C.c_int), ("n_ransac_points", C.c_int),
                                                                                                   ("outlier_prob", C.c_float), ("success_prob", C.c_float)]


def reve_default_config(**kw):
    c = ReveConfig()
    load_library().gorio_prep_reve_default_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def reve_ransac_iterations(cfg=None):
    return load_library().gorio_prep_reve_ransac_iterations(C.byref(cfg or reve_default_config()))


def ego_velocity(targets, samples, cfg=None, device=0):
    """RadarEgoVelocityEstimator::estimate on the GPU.  targets [n,5] float32 = x y z intensity doppler; samples [n_iter, N] uint32."""
    lib = load_library()
    lib.gorio_prep_last_error.restype = C.c_char_p
    cfg = cfg or reve_default_config()
    t = np.ascontiguousarray(targets, np.float32)
    s = np.ascontiguousarray(samples, np.uint32).reshape(-1, cfg.n_ransac_points) if len(samples) else np.zeros((0, cfg.n_ransac_points), np.uint32)
    n = t.shape[0]
    base = t.__array_interface__["data"][0]
    v, sg = np.zeros(3), np.zeros(3)
    inl, outl = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    nv, zv, ok = C.c_int(0), C.c_int(0), C.c_int(0)
    rc = lib.gorio_prep_ego_velocity(int(device), C.c_void_p(base), C.c_void_p(base + 12), C.c_void_p(base + 16), n, 20, C.byref(cfg),
                                     C.c_void_p(s.__array_interface__["data"][0]) if s.shape[0] else None, s.shape[0], C.c_void_p(v.__array_interface__["data"][0]),
                                     C.c_void_p(sg.__array_interface__["data"][0]), C.c_void_p(inl.__array_interface__["data"][0]), C.c_void_p(outl.__array_interface__["data"][0]),
                                     C.byref(nv), C.byref(zv), C.byref(ok))
    if rc < 0:
        msg = lib.gorio_prep_last_error()
        raise GorioError(rc, msg.decode() if msg else "")
    return dict(success=bool(ok.value), v_r=v, sigma_v_r=sg, inlier=inl.astype(bool), outlier=outl.astype(bool), n_valid=nv.value, zero_velocity=bool(zv.value))


# ------------------------------------------------------------------------------------------------ include/gorio_scan.h
SCAN_SYMBOLS = ["gorio_scan_default_params", "gorio_scan_create", "gorio_scan_destroy", "gorio_scan_load", "gorio_scan_run", "gorio_scan_get_output", "gorio_scan_get_stage",
                "gorio_scan_get_stage_points", "gorio_scan_get_counters", "gorio_scan_last_error", "gorio_apd_set_source_from_scan", "gorio_apd_set_target_from_scan"]
SCAN_BATCH_SYMBOLS = ["gorio_scan_load_batch", "gorio_scan_run_batch", "gorio_scan_handle_error", "gorio_scan_batch_diag"]  # include/gorio_scan_batch.h
SCAN_BATCH_MAX = 1024
OUTLIER_NONE, OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1, 2
SCAN_OK, SCAN_ZERO_VELOCITY, SCAN_EMPTY, SCAN_REFUSED = 0, 1, 2, 3
SCAN_STATUS = {0: "ok", 1: "zero_velocity", 2: "empty", 3: "refused"}
STAGES = {"gate": 0, "dynamic": 1, "deskew": 2, "distance": 3, "outlier": 4, "ground": 5}
SCAN_STAGE_DBSCAN = 6  # only a value of a result's "stage": the label stage puts out no cloud of its own


def _scan_params_type():
    from .ground import GroundParams

    class ScanParams(C.Structure):
        """gorio_scan_params (include/gorio_scan.h)."""
        _fields_ = [("power_threshold", C.c_float), ("rotation", C.c_double * 9), ("enable_dynamic_object_removal", C.c_int), ("deskew", C.c_int), ("scan_period", C.c_double),
                    ("distance_near", C.c_double), ("distance_far", C.c_double), ("z_low", C.c_double), ("z_high", C.c_double), ("outlier_method", C.c_int), ("mean_k", C.c_int),
                    ("stddev_mul", C.c_double), ("radius", C.c_double), ("min_neighbors", C.c_int), ("ground", C.c_int), ("ground_params", GroundParams),
                    ("dbscan_core_min_pts", C.c_int), ("dbscan_eps", C.c_double), ("dbscan_min_cluster_size", C.c_int), ("dbscan_max_cluster_size", C.c_int), ("reve", ReveConfig)]

    return ScanParams


ScanParams = _scan_params_type()


class ScanResult(C.Structure):
    _fields_ = [("status", C.c_int), ("stage", C.c_int), ("reve_success", C.c_int), ("v_r", C.c_double * 3), ("sigma_v_r", C.c_double * 3), ("n_out", C.c_int),
                ("n_ground", C.c_int), ("n_clusters", C.c_int)]


def scan_default_params(**kw):
    p = ScanParams()
    load_library().gorio_scan_default_params(C.byref(p))
    for k, v in kw.items():
        if k == "rotation":
            p.rotation[:] = [float(x) for x in np.asarray(v, np.float64).reshape(9)]
        else:
            setattr(p, k, v)
    return p


def _ptr(a):
    return C.c_void_p(a.__array_interface__["data"][0])


class ScanPipeline:
    """gorio_scan_t: the preprocessing nodelet's cloud_callback (preprocessing_nodelet_ntu.cpp:370-581) with the scan resident on the GPU.
    One frame is load(raw) -> (n_gated, n_valid), then run(samples, ang_vel) -> dict; output() / stage() read results back."""

    def __init__(self, params=None, device=0, **overrides):
        self.lib = load_library()
        self.lib.gorio_scan_last_error.restype = C.c_char_p
        self.params = params if params is not None else scan_default_params(**overrides)
        self.h = C.c_void_p()
        self._check(self.lib.gorio_scan_create(C.byref(self.h), int(device), C.byref(self.params)))

    def _check(self, rc):
        if rc < 0:
            msg = self.lib.gorio_scan_last_error()
            raise GorioError(rc, msg.decode() if msg else "")

    def close(self):
        if self.h:
            self.lib.gorio_scan_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, raw):
        """raw [n, 5] float32 = x y z power doppler (the message's points, channels[2] and channels[0])."""
        t = np.ascontiguousarray(raw, np.float32).reshape(-1, 5)
        base = t.__array_interface__["data"][0]
        ng, nv = C.c_int(0), C.c_int(0)
        n = t.shape[0]
        self._check(self.lib.gorio_scan_load(self.h, C.c_void_p(base) if n else None, C.c_void_p(base + 12) if n else None, C.c_void_p(base + 16) if n else None, n, 20,
                                             C.byref(ng), C.byref(nv)))
        return ng.value, nv.value

    def run(self, samples=(), ang_vel=None):
        """samples [n_iter, n_ransac_points] uint32 into the valid targets; ang_vel: 3 numbers or None.  A refusal raises GorioError."""
        k = self.params.reve.n_ransac_points
        s = np.ascontiguousarray(samples, np.uint32).reshape(-1, k) if len(samples) else np.zeros((0, k), np.uint32)
        w = None if ang_vel is None else (C.c_double * 3)(*[float(x) for x in ang_vel])
        r = ScanResult()
        rc = self.lib.gorio_scan_run(self.h, _ptr(s) if s.shape[0] else None, s.shape[0], w, C.byref(r))
        self.last_result = dict(status=SCAN_STATUS.get(r.status, r.status), stage=r.stage, reve_success=bool(r.reve_success), v_r=np.array(r.v_r[:]), sigma_v_r=np.array(r.sigma_v_r[:]),
                                n_out=r.n_out, n_ground=r.n_ground, n_clusters=r.n_clusters)
        self._check(rc)
        return self.last_result

    def output(self):
        """(xyz [n,3], intensity [n], doppler [n], label [n]) of the last OK run: what the nodelet publishes."""
        n = self.last_result["n_out"]
        buf = np.zeros((max(n, 1), 6), np.float32)
        base = buf.__array_interface__["data"][0]
        self._check(self.lib.gorio_scan_get_output(self.h, C.c_void_p(base), C.c_void_p(base + 12), C.c_void_p(base + 16), C.c_void_p(base + 20), 24, buf.shape[0]))
        buf = buf[:n]
        return buf[:, :3].copy(), buf[:, 3].copy(), buf[:, 4].copy(), buf[:, 5].copy()

    def stage(self, stage, points=False):
        """Indices (into the gated cloud; for "gate": into the raw message) of the points that survive `stage`, in order; with points=True
        also their coordinates after that stage."""
        st = STAGES[stage] if isinstance(stage, str) else int(stage)
        cnt = C.c_int(0)
        self._check(self.lib.gorio_scan_get_stage(self.h, st, None, 0, C.byref(cnt)))
        idx = np.zeros(max(cnt.value, 1), np.int32)
        self._check(self.lib.gorio_scan_get_stage(self.h, st, _ptr(idx), idx.shape[0], C.byref(cnt)))
        idx = idx[:cnt.value]
        if not points:
            return idx
        xyz = np.zeros((max(cnt.value, 1), 3), np.float32)
        self._check(self.lib.gorio_scan_get_stage_points(self.h, st, _ptr(xyz), xyz.shape[0], C.byref(cnt)))
        return idx, xyz[:cnt.value]

    def counters(self):
        u, b, d = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        self._check(self.lib.gorio_scan_get_counters(self.h, C.byref(u), C.byref(b), C.byref(d)))
        return dict(point_uploads=u.value, index_builds=b.value, point_downloads=d.value)


# ------------------------------------------------------------------------------------------------ include/gorio_scan_batch.h
def _result_dict(r, code=0, error=""):
    return dict(status=SCAN_STATUS.get(r.status, r.status), stage=r.stage, reve_success=bool(r.reve_success), v_r=np.array(r.v_r[:]), sigma_v_r=np.array(r.sigma_v_r[:]),
                n_out=r.n_out, n_ground=r.n_ground, n_clusters=r.n_clusters, code=code, error=error)


def _batch_check(lib, rc):
    if rc < 0:
        lib.gorio_scan_last_error.restype = C.c_char_p
        msg = lib.gorio_scan_last_error()
        raise GorioError(rc, msg.decode() if msg else "")


def scan_load_batch(pipes, raws):
    """gorio_scan_load_batch: pipes[i].load(raws[i]) for every member in two rounds.  Returns (n_gated [count], n_valid [count])."""
    if len(pipes) != len(raws):
        raise ValueError("one raw scan per pipeline")
    count = len(pipes)
    if count == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    lib = pipes[0].lib
    ts = [np.ascontiguousarray(r, np.float32).reshape(-1, 5) for r in raws]
    base = [t.__array_interface__["data"][0] for t in ts]
    hs = (C.c_void_p * count)(*[p.h for p in pipes])
    xyz = (C.c_void_p * count)(*[b if len(t) else None for b, t in zip(base, ts)])
    pw = (C.c_void_p * count)(*[b + 12 if len(t) else None for b, t in zip(base, ts)])
    dop = (C.c_void_p * count)(*[b + 16 if len(t) else None for b, t in zip(base, ts)])
    n = (C.c_int * count)(*[len(t) for t in ts])
    st = (C.c_int * count)(*([20] * count))
    ng, nv = (C.c_int * count)(), (C.c_int * count)()
    _batch_check(lib, lib.gorio_scan_load_batch(hs, count, xyz, pw, dop, n, st, ng, nv))
    return np.array(ng[:], np.int32), np.array(nv[:], np.int32)


def scan_run_batch(pipes, samples, ang_vels):
    """gorio_scan_run_batch: pipes[i].run(samples[i], ang_vels[i]) for every member in lock-step rounds.  A member's refusal does not raise:
    its dict carries `code` (what the single run would have returned) and `error` (its text).  Sets every pipe.last_result."""
    if len(pipes) != len(samples) or len(pipes) != len(ang_vels):
        raise ValueError("one sample set and one angular velocity (or None) per pipeline")
    count = len(pipes)
    if count == 0:
        return []
    lib = pipes[0].lib
    lib.gorio_scan_handle_error.restype = C.c_char_p
    ss = []
    for p, s in zip(pipes, samples):
        k = p.params.reve.n_ransac_points
        ss.append(np.ascontiguousarray(s, np.uint32).reshape(-1, k) if len(s) else np.zeros((0, k), np.uint32))
    ws = [None if w is None else (C.c_double * 3)(*[float(x) for x in w]) for w in ang_vels]
    hs = (C.c_void_p * count)(*[p.h for p in pipes])
    sp = (C.c_void_p * count)(*[s.__array_interface__["data"][0] if s.shape[0] else None for s in ss])
    ni = (C.c_int * count)(*[s.shape[0] for s in ss])
    wp = (C.c_void_p * count)(*[None if w is None else C.addressof(w) for w in ws])
    res = (ScanResult * count)()
    codes = (C.c_int * count)()
    _batch_check(lib, lib.gorio_scan_run_batch(hs, count, sp, ni, wp, res, codes))
    out = []
    for i, p in enumerate(pipes):
        msg = lib.gorio_scan_handle_error(p.h)
        p.last_result = _result_dict(res[i], codes[i], msg.decode() if msg else "")
        out.append(p.last_result)
    return out


def scan_batch_diag(lead):
    """Shape of the last batch call whose first pipeline was `lead`: dict(rounds, launches, synchronisations)."""
    r, l, s = C.c_int(0), C.c_int(0), C.c_int(0)
    _batch_check(lead.lib, lead.lib.gorio_scan_batch_diag(lead.h, C.byref(r), C.byref(l), C.byref(s)))
    return dict(rounds=r.value, launches=l.value, synchronisations=s.value)
