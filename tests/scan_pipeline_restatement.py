"""NumPy restatement of the preprocessing nodelet's cloud_callback (apps/preprocessing_nodelet_ntu.cpp:370-581, "PREP"): the four stages that
have no other restatement -- gate and rotate, dynamic-object selection, deskew, distance filter -- written here operation by operation,
and the whole callback chained from them and the existing oracle / restatement stages (REVE, the outlier masks and the DBSCAN labels of
oracle.apd, Patchwork++ of patchwork_restatement).

Every float32 operation below is ONE correctly rounded NumPy operation in the order include/gorio_scan.h and go-rio_amd/csrc/apd_scan.hip
document, so the GPU stages can be compared bit for bit."""
import types

import numpy as np

F = np.float32

OUTLIER_NONE, OUTLIER_STATISTICAL, OUTLIER_RADIUS = 0, 1, 2
STAGES = ("gate", "dynamic", "deskew", "distance", "outlier", "ground")


def default_params(**kw):
    """The nodelet's own defaults (the second argument of each private_nh.param, PREP:97-181, 526-529, 705)."""
    p = types.SimpleNamespace(power_threshold=0.0, rotation=np.eye(3), enable_dynamic_object_removal=False, deskew=True, scan_period=0.1, distance_near=1.0,
                              distance_far=100.0, z_low=-5.0, z_high=20.0, outlier_method=OUTLIER_STATISTICAL, mean_k=20, stddev_mul=1.0, radius=2.0, min_neighbors=2,
                              ground=True, dbscan_core_min_pts=10, dbscan_eps=0.9, dbscan_min_cluster_size=20, dbscan_max_cluster_size=25000, reve={})
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


def gate_rotate(raw, power_threshold=0.0, rotation=np.eye(3)):
    """PREP:381-412.  raw [n, 5] float32 = x y z power doppler.  Returns (indices into raw of the points kept, in order; their cloud [m, 5]
    = rotated x y z, power, doppler).  Kept: power > threshold (float compare) and all three coordinates finite -- the reference's == NAN
    tests drop nothing, dropping NaN and +-Inf is the pipeline's documented deviation.  Rotation in double, (r0 x + r1 y) + r2 z, one rounding."""
    raw = np.asarray(raw, F).reshape(-1, 5)
    R = np.asarray(rotation, np.float64).reshape(3, 3)
    keep = (raw[:, 3] > F(power_threshold)) & np.isfinite(raw[:, 0]) & np.isfinite(raw[:, 1]) & np.isfinite(raw[:, 2])
    idx = np.nonzero(keep)[0]
    x, y, z = (raw[idx, k].astype(np.float64) for k in range(3))
    out = raw[idx].copy()
    for r in range(3):
        out[:, r] = ((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z).astype(F)
    return idx.astype(np.int64), out


def dynamic_select(inlier_mask, success=True):
    """PREP:453-478: the cloud continues with the inlier cloud of the estimate, which is empty when the estimate failed."""
    m = np.asarray(inlier_mask, bool)
    return np.nonzero(m)[0] if success else np.zeros(0, np.int64)


def deskew(xyz, ang_vel, scan_period=0.1):
    """PREP:695-716.  ang_v = Vector3f(imu angular velocity) * -1; per point i of a cloud of `size` points:
         delta_t = (scan_period * double(i)) / size                          double
         q = Quaternionf(1, float(delta_t / 2 * ang_v))                      unnormalised
         q^-1 = conjugate / squaredNorm, squaredNorm = ((x x + y y) + z z) + w w
         out = v + w 2(q x v) + q x 2(q x v)  as Eigen's _transformVector: uv = q x v; uv += uv; (v + w uv) + q x uv
       everything float except delta_t and the products that make q."""
    v = np.asarray(xyz, F).reshape(-1, 3)
    n = v.shape[0]
    w = -(np.asarray(ang_vel, np.float64).astype(F))
    i = np.arange(n, dtype=np.float64)
    delta_t = scan_period * i / np.float64(n) if n else i
    half = delta_t / 2.0
    qx, qy, qz = ((half * np.float64(w[k])).astype(F) for k in range(3))
    qw = np.ones(n, F)
    n2 = ((qx * qx + qy * qy) + qz * qz) + qw * qw
    ix, iy, iz, iw = -qx / n2, -qy / n2, -qz / n2, qw / n2
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    ux, uy, uz = iy * vz - iz * vy, iz * vx - ix * vz, ix * vy - iy * vx
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    cx, cy, cz = iy * uz - iz * uy, iz * ux - ix * uz, ix * uy - iy * ux
    out = np.stack([(vx + iw * ux) + cx, (vy + iw * uy) + cy, (vz + iw * uz) + cz], 1)
    assert out.dtype == F
    return out


def distance_mask(xyz, near=1.0, far=100.0, z_low=-5.0, z_high=20.0):
    """PREP:643-647: d = double(float norm sqrtf((x x + y y) + z z)), z widened to double; d > near && d < far && z < z_high && z > z_low."""
    v = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    d = np.sqrt((x * x + y * y) + z * z).astype(np.float64)
    zd = z.astype(np.float64)
    return (d > near) & (d < far) & (zd < z_high) & (zd > z_low)


def callback(raw, p, samples, ang_vel, oracle_apd, patchwork=None):
    """The whole callback in PREP order.  `patchwork` is a patchwork_restatement.Patchworkpp that carries the segmenter's state across frames
    (needed when p.ground).  Returns a dict: status ("ok" / "zero_velocity" / "empty" / "refused"), stage (the one an empty / refused run ended
    in), stages {name: (indices into the gated cloud -- for "gate": into raw --, xyz after the stage)}, and for "ok": xyz, intensity, doppler,
    label, n_ground, n_clusters, margin (Patchwork++'s distance from its nearest decision threshold); v_r, sigma_v_r, reve_success always."""
    res = dict(status="ok", stage=-1, stages={}, v_r=np.zeros(3), sigma_v_r=np.zeros(3), reve_success=False, margin=np.inf)
    idx, cloud = gate_rotate(raw, p.power_threshold, p.rotation)
    res["stages"]["gate"] = (idx, cloud[:, :3].copy())
    res["n_gated"] = len(cloud)

    def end(status, stage):
        res["status"], res["stage"] = status, STAGES.index(stage)
        return res

    if len(cloud) == 0:
        return end("empty", "gate")
    cfg = oracle_apd.reve_default_config(**p.reve)
    est = oracle_apd.reve_estimate(cloud, np.asarray(samples, np.uint32).reshape(-1, cfg.n_ransac_points), cfg)
    res["n_valid"] = est["n_valid"]
    res["reve_success"] = ok = bool(est["success"])
    if ok:
        res["v_r"], res["sigma_v_r"] = est["v_r"], est["sigma_v_r"]
        if np.sqrt(np.sum(est["v_r"] * est["v_r"])) < 0.05:  # PREP:427-430
            res["status"] = "zero_velocity"
            return res
    cur = np.arange(len(cloud))
    if p.enable_dynamic_object_removal:
        cur = dynamic_select(est["inlier"], ok)
    pts = cloud[cur]
    res["stages"]["dynamic"] = (cur, pts[:, :3].copy())
    if len(cur) == 0:
        return end("empty", "dynamic")
    if p.deskew and ang_vel is not None:
        pts = pts.copy()
        pts[:, :3] = deskew(pts[:, :3], ang_vel, p.scan_period)
    res["stages"]["deskew"] = (cur, pts[:, :3].copy())
    k = distance_mask(pts[:, :3], p.distance_near, p.distance_far, p.z_low, p.z_high)
    cur, pts = cur[k], pts[k]
    res["stages"]["distance"] = (cur, pts[:, :3].copy())
    if len(cur) == 0:
        return end("empty", "distance")
    if p.outlier_method != OUTLIER_NONE:
        xyz = np.ascontiguousarray(pts[:, :3])
        if p.outlier_method == OUTLIER_STATISTICAL:
            if len(xyz) < p.mean_k + 1:
                return end("refused", "outlier")
            k, _ = oracle_apd.statistical_outlier_mask(xyz, p.mean_k, p.stddev_mul)
        else:
            k = oracle_apd.radius_outlier_mask(xyz, p.radius, p.min_neighbors)
        cur, pts = cur[k], pts[k]
    res["stages"]["outlier"] = (cur, pts[:, :3].copy())
    if len(cur) == 0:
        return end("empty", "outlier")
    n_ground = 0
    if p.ground:
        out = patchwork.estimate_ground(np.ascontiguousarray(pts[:, :3]), np.ascontiguousarray(pts[:, 3]), id=1)
        res["margin"] = out["margin"]
        n_ground = len(out["ground"])
        order = np.concatenate([np.asarray(out["ground"], np.int64), np.asarray(out["nonground"], np.int64)])  # PREP:518
        cur, pts = cur[order], pts[order]
    res["stages"]["ground"] = (cur, pts[:, :3].copy())
    if len(cur) == 0:
        return end("empty", "ground")
    xyz = np.ascontiguousarray(pts[:, :3])
    lab, nc = oracle_apd.dbscan_labels(xyz, p.dbscan_eps, p.dbscan_core_min_pts, p.dbscan_min_cluster_size, p.dbscan_max_cluster_size)
    res.update(xyz=xyz, intensity=pts[:, 3].copy(), doppler=pts[:, 4].copy(), label=lab, n_ground=n_ground, n_clusters=nc, n_out=len(xyz))
    return res


# ------------------------------------------------------------------------------------------------ scenes for the pipeline's tests
def raw_scan(seed, n_ground=9000, v_true=(5.2, -0.3, 0.1), noise=0.05, movers=300, rotation=np.eye(3), junk=40):
    """A raw radar message [n, 5]: the points of ground_scenes.scan carried into the radar frame (so that `rotation` brings them back), power =
    the scene's intensity, Doppler consistent with the ego velocity v_true in the body frame plus `movers` moving objects (as _radar_targets of
    tests/test_prep_gpu.py makes them), and `junk` points the gate must drop: power at or below 0, NaN and +-Inf coordinates."""
    import ground_scenes as gs

    rng = np.random.default_rng(10_000 + seed)
    xyz, inten = gs.scan(seed, n_ground=n_ground)
    n = len(xyz)
    xyz = xyz.astype(np.float64)
    r = np.linalg.norm(xyz, axis=1, keepdims=True)
    dop = -(xyz / r) @ np.asarray(v_true, np.float64) + rng.normal(0, noise, n)  # the estimator negates the measured Doppler (REVE:87)
    dop[:movers] += rng.uniform(-4, 4, movers)
    R = np.asarray(rotation, np.float64)
    raw = np.concatenate([xyz @ R, inten[:, None], dop[:, None]], 1).astype(F)  # row-vector form of R^T p
    if junk:
        at = rng.choice(n, junk, replace=False)
        q = junk // 4
        raw[at[:q], 3] = np.where(np.arange(q) % 2 == 0, 0.0, -1.5)
        raw[at[q:2 * q], rng.integers(0, 3, q)] = np.nan
        raw[at[2 * q:3 * q], rng.integers(0, 3, q)] = np.inf
        raw[at[3 * q:], rng.integers(0, 3, junk - 3 * q)] = -np.inf
    return raw


def tilt(yaw=0.3, pitch=0.02):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])


# (seed, dynamic-object removal, outlier method) of the whole-callback comparison, and the seeds of the five-scan sequence (n_ground 2500);
# tests/test_scan_restatement.py checks on the CPU that the restatement keeps its Patchwork++ margin on every one of them
CHAIN_CASES = ((22, False, OUTLIER_STATISTICAL), (22, False, OUTLIER_RADIUS), (21, True, OUTLIER_STATISTICAL), (21, True, OUTLIER_RADIUS))
CHAIN_ANG_VEL = (0.01, -0.02, 0.15)
SEQUENCE_SEEDS = (120, 121, 122, 123, 124)
SEQUENCE_N_GROUND = 2500


def chain_inputs(seed, dor, method, oracle_apd, n_ground=9000):
    """(raw, params, samples) of one comparison case; the samples are drawn as the REVE tests draw them, from the count of valid targets."""
    raw = raw_scan(seed, n_ground=n_ground, rotation=tilt())
    p = default_params(rotation=tilt(), enable_dynamic_object_removal=dor, outlier_method=method)
    nv = callback(raw, default_params(rotation=tilt(), ground=False, outlier_method=OUTLIER_NONE), np.zeros((0, 5), np.uint32), None, oracle_apd)["n_valid"]
    samples = np.random.default_rng(seed).integers(0, nv, (3, 5)).astype(np.uint32)
    return raw, p, samples
