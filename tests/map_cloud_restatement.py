"""NumPy restatement of include/gorio_map.h (MapCloudGenerator::generate, src/radar_graph_slam/map_cloud_generator.cpp:13-89 of the Go-RIO
sources, "MCG"): exactly the operations the header fixes, in the order it fixes them, so that the GPU result can be compared bit for bit.
NumPy rounds every float32 / float64 operation by itself (nothing is fused), which is what the header asks of the kernels.

Beside it, pcl_voxel_centres emulates what PCL 1.10's OctreePointCloud does to its bounding box while points are added.  PCL's sources
were not at hand: that function is written from recollection of octree_pointcloud.hpp and is the ASSUMPTION the header states.

No GPU, no library: this module is test infrastructure only."""
import numpy as np

F = np.float32
D = np.float64
GATE = 50.0  # MCG:26


def gate(xyz):
    """MCG:25-26.  True where the point is kept: NaN passes (`d > 50` is false), an infinity does not."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        s = (x * x + y * y) + z * z  # float32, left to right
        d = np.sqrt(s.astype(D)).astype(F)  # the correctly rounded float root
        return ~(d.astype(D) > GATE)


def transform_float(xyz, pose):
    """MCG:23, 28: M = pose.matrix().cast<float>(); q_r = ((M_r0 x + M_r1 y) + M_r2 z) + M_r3 in float32."""
    with np.errstate(all="ignore"):
        M = np.asarray(pose, D).reshape(4, 4)[:3].astype(F)
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1).astype(F)


def transform_double(xyz, pose):
    """NOT what the map does: the double transform of the submap assembly (four products summed left to right in double, rounded to float
    once).  Here so that a test can show its input tells the two apart."""
    with np.errstate(all="ignore"):
        T = np.asarray(pose, D).reshape(4, 4)[:3]
        x, y, z = (xyz[:, c].astype(D) for c in range(3))
        return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(F) for r in range(3)], axis=1)


def stage_a(frames, poses, transform=transform_float):
    """frames: list of (xyz [n, 3], intensity [n] or None).  Returns (q [m, 3] float32, intensity [m] float32) in the order listed."""
    qs, its = [np.zeros((0, 3), F)], [np.zeros(0, F)]
    for (xyz, inten), pose in zip(frames, poses):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        keep = gate(xyz)
        qs.append(transform(xyz[keep], pose))
        its.append(np.zeros(int(keep.sum()), F) if inten is None else np.asarray(inten, F).reshape(-1)[keep])
    return np.concatenate(qs), np.concatenate(its)


def lattice(q, resolution):
    """(anchor a [3] float64, cells k [n_finite, 3] int64) of the finite points of q, or (None, empty) without one."""
    fin = np.isfinite(q).all(axis=1)
    if not fin.any():
        return None, np.zeros((0, 3), np.int64)
    qf = q[fin].astype(D)
    a = qf[0] - D(resolution) / 2
    kd = np.floor((qf - a) / D(resolution))
    if not (np.abs(kd) < 2.0 ** 30).all():
        raise OverflowError("a cell coordinate reaches 2^30")
    k = kd.astype(np.int64)
    if ((k.max(axis=0) - k.min(axis=0) + 1) >= 2 ** 21).any():
        raise OverflowError("the occupied voxels span 2^21 cells or more on an axis")
    return a, k


def voxel_centres(q, resolution):
    """MCG:41-50 as the header defines it: one centre per occupied voxel in ascending (kx, ky, kz) order.  Returns (centres [v, 3] float32,
    info dict with the fields of gorio_map_info_t that stage B fills)."""
    a, k = lattice(q, resolution)
    if a is None:
        return np.zeros((0, 3), F), dict(n_finite=0, n_voxels=0, anchor=[0.0] * 3, min_k=[0] * 3, max_k=[0] * 3)
    u = np.unique(k, axis=0)  # rows in ascending lexicographic order
    c = ((u.astype(D) + 0.5) * D(resolution) + a).astype(F)
    return c, dict(n_finite=int(len(k)), n_voxels=int(len(u)), anchor=[float(v) for v in a], min_k=[int(v) for v in k.min(axis=0)], max_k=[int(v) for v in k.max(axis=0)])


def generate(frames, poses, resolution, transform=transform_float):
    """The whole call: (xyz [n, 3], intensity [n], info)."""
    q, inten = stage_a(frames, poses, transform)
    info = dict(n_listed=int(sum(len(np.asarray(x).reshape(-1, 3)) for x, _ in frames)), n_kept=int(len(q)), n_finite=0, n_voxels=0, anchor=[0.0] * 3, min_k=[0] * 3, max_k=[0] * 3)
    if not resolution > 0:
        return q, inten, info
    c, vi = voxel_centres(q, resolution)
    info.update(vi)
    return c, np.zeros(len(c), F), info


def pcl_voxel_centres(q, resolution):
    """ASSUMED (PCL 1.10, octree_pointcloud.hpp, from recollection): addPointsFromInputCloud skips non-finite points; adoptBoundingBoxToPoint
    sets the box to q0 -+ resolution / 2 for the first point and then, while a point lies outside, adds one tree level: the side doubles,
    and on every axis WITHOUT an upper violation the lower corner moves down by the old side.  genOctreeKeyforPoint is
    (unsigned)((q - min) / resolution), genLeafNodeCenterFromOctreeKey is (float)((key + 0.5) * resolution + min), both against the FINAL
    lower corner (the tree re-keys when it grows; keys only shift by whole cells).  Returns the centres sorted by key, lexicographically."""
    res = D(resolution)
    eps = D(np.finfo(F).eps)  # PCL's minValue, taken off the side so that the upper face lies outside
    qf = q[np.isfinite(q).all(axis=1)].astype(D)
    if not len(qf):
        return np.zeros((0, 3), F)
    lo = qf[0] - res / 2
    side = res  # depth 0: one voxel
    hi = qf[0] + res / 2
    for p in qf:
        while ((p < lo) | (p >= hi)).any():
            upper = p >= hi
            lo = np.where(upper, lo, lo - side)
            side = side * 2
            hi = lo + (side - eps)
    key = np.floor((qf - lo) / res).astype(np.int64)
    u = np.unique(key, axis=0)
    return ((u.astype(D) + 0.5) * res + lo).astype(F)


def face_ties(q, resolution, tol=1e-9):
    """Mask over q: finite points that lie ON a cell face of the lattice in real arithmetic, on any axis.  Float coordinates make that
    common, not rare: with a = q0 - res / 2 and res = 0.05, every point whose coordinate differs from the anchor's by an odd multiple of
    1 / 8 sits exactly on a face ((1 / 8 + 1 / 40) / (1 / 20) = 3).  Which side such a point falls to is decided by the rounding of the
    double quotient, here as in PCL, so the two lattices may disagree about it.  tol is far above what the roundings can move a quotient
    (a few thousand cells times 2.2e-16) and far below what separates any other point from a face."""
    fin = np.isfinite(q).all(axis=1)
    out = np.zeros(len(q), bool)
    if fin.any():
        qf = q[fin].astype(D)
        t = (qf - (qf[0] - D(resolution) / 2)) / D(resolution)
        out[fin] = (np.abs(t - np.round(t)) < tol).any(axis=1)
    return out


def ulp_distance(a, b):
    """Per element: how many float32 values lie between a and b (0 = same bits; +0 and -0 count as equal)."""
    def ordered(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


# ------------------------------------------------------------------------------------------------------------------------- scenes
def radar_like_frame(n, seed, snap=0.5, noise=0.05):
    """n points in a forward fan up to 60 m (so the gate has something to drop), snapped to `snap` metres plus `noise` of jitter so that
    voxels are shared between points and between keyframes; intensities 0..40."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.0, 60.0, n)
    az = rng.uniform(-1.0, 1.0, n)
    el = rng.uniform(-0.25, 0.25, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)
    if snap > 0:
        xyz = np.round(xyz / snap) * snap
    xyz = xyz + rng.normal(0.0, noise, (n, 3))
    return xyz.astype(F), rng.uniform(0.0, 40.0, n).astype(F)


def curve_pose(k, step=1.3, turn=0.11):
    """Pose k on a curving, slightly climbing trajectory: entries like 0.1 * k that change under the cast to float."""
    yaw, pitch = turn * k, 0.02 * k
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
    T[:3, 3] = [step * k * np.cos(0.5 * yaw) + 0.1, step * k * np.sin(0.5 * yaw) - 0.1 * k, 0.03 * k + 0.1]
    return T


def scene(sizes, seed=0, snap=0.5):
    """Keyframes of the given sizes along curve_pose: (frames, poses)."""
    return [radar_like_frame(n, seed + 17 * k, snap=snap) for k, n in enumerate(sizes)], [curve_pose(k) for k in range(len(sizes))]
