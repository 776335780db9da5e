"""Seeded scenes for the three voxel structures that share one device pipeline (keys = cell id << 31 | input index, the tiled
key sort, voxel starts counted per 256-key block, one scan of the block counts 1024 at a time, one lane per cell start):
pcl::VoxelGrid (setInputTargetSubmap, prep.voxel_downsample), the FastVGICP Gaussian voxel map and the NDT covariance grid.
NumPy only; tests/test_voxel_scenes.py pins the scenes and the CPU restatements on them, tests/test_voxel_edges_gpu.py runs them
on the device.

A cell of edge `cell` and `phase` p holds the coordinates [(k + p) cell, (k + 1 + p) cell): p = 0 is floor(x / leaf) of VoxelGrid and
the NDT grid, p = 0.5 is floor(x / resolution - 0.5) of the FastVGICP map (fast_vgicp_voxel.hpp:158-160).

Occupancy regimes (float32 xyz [m, 3] in SHUFFLED input order: the order inside a cell is not the sorted one)
  one_cell   every point inside one cell: one voxel start, at key 0, and a single run over the whole cloud
  own_cell   one point per cell of a cubic lattice: m voxel starts, every 64-lane ballot full
  mixed      lattice cells with multiplicities between 1 and MIXED_MAX, a few of them long: runs that start in one wave or 256-key
             block and end in a later one, and (from 4095 points on) 256-key blocks with no voxel start at all
SIZES are the smallest that cross each structure of the pipeline: the 64-lane ballot, the 256-key count block, the sort's padding
(4096 -> 8192 keys at 4097) and the second pass of the block-count scan (1025 blocks at 262 145 keys).

Geometry scenes (at most 2 000 points) and limit scenes (8 - 32 points that fix a bounding box) are described at their generators.
"""
import numpy as np

f32 = np.float32
INT_MAX = 2147483647
GRID_CELL = 0.1  # leaf of the VoxelGrid regime scenes: the launch files' leaf, whose float inverse is not exact

SIZES_SMALL = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
SIZES_LARGE = (262143, 262144, 262145)  # nblocks = ceil(m / 256): 1024, 1024, 1025
MIXED_MAX = 700
MIXED_LONG = (700, 513, 300)  # the first multiplicities of every mixed scene that has room for them
REGIMES = ("one_cell", "own_cell", "mixed")


def regime_cases():
    """(regime, size) for every pair the tests run: one_cell stops at 4097 (its only start is key 0 at every size)."""
    out = [(r, m) for r in REGIMES for m in SIZES_SMALL]
    out += [(r, m) for r in ("own_cell", "mixed") for m in SIZES_LARGE]
    return out


def _lattice_cells(count, rng, spread=1):
    """`count` distinct integer cells of a cube around the origin (negative indices included), `spread` times as many cells as needed
    on every axis when > 1 (then a random subset: gaps in the id range)."""
    side = 1
    while side ** 3 < count:
        side += 1
    side *= spread
    pick = np.arange(count) if spread == 1 else np.sort(rng.choice(side ** 3, count, replace=False))
    cells = np.stack([pick % side, (pick // side) % side, pick // (side * side)], axis=1).astype(np.int64)
    return cells - side // 2


def _inside(cells, rng, cell, phase):
    """one point per row of `cells`, uniform in the middle half of the cell: no coordinate is near a face"""
    u = rng.uniform(0.25, 0.75, cells.shape)
    return ((cells + phase + u) * cell).astype(f32)


def one_cell(m, seed=0, cell=1.0, phase=0.0):
    rng = np.random.default_rng(7000 + seed)
    return np.ascontiguousarray(_inside(np.tile(np.array([[3, -2, 1]], np.int64), (m, 1)), rng, cell, phase))


def own_cell(m, seed=0, cell=1.0, phase=0.0):
    rng = np.random.default_rng(7100 + seed)
    cells = _lattice_cells(m, rng)
    return np.ascontiguousarray(_inside(cells[rng.permutation(m)], rng, cell, phase))


def mixed_multiplicities(m, seed=0):
    """multiplicities that sum to m: MIXED_LONG first (as far as m allows), then log-uniform draws in [1, MIXED_MAX]"""
    rng = np.random.default_rng(7200 + seed)
    out, left = [], m
    for k in MIXED_LONG:
        if left >= 2 * k:
            out.append(k)
            left -= k
    while left > 0:
        k = min(left, int(np.exp(rng.uniform(0.0, np.log(MIXED_MAX + 1.0)))))
        out.append(max(k, 1))
        left -= out[-1]
    return np.array(out, np.int64)


def mixed(m, seed=0, cell=1.0, phase=0.0):
    rng = np.random.default_rng(7300 + seed)
    mult = mixed_multiplicities(m, seed)
    cells = _lattice_cells(len(mult), rng, spread=2)
    cells = cells[rng.permutation(len(mult))]  # the long runs do not sit at the lowest ids
    pts = _inside(np.repeat(cells, mult, axis=0), rng, cell, phase)
    return np.ascontiguousarray(pts[rng.permutation(m)])


def regime(name, m, seed=0, cell=1.0, phase=0.0):
    return {"one_cell": one_cell, "own_cell": own_cell, "mixed": mixed}[name](m, seed, cell, phase)


def labels(m, seed=0):
    """cluster ids 0 .. 9 as the preprocessing writes them into normal_x"""
    return np.random.default_rng(7400 + seed).integers(0, 10, m).astype(f32)


def covariances(m, seed=0):
    """seeded SPD 4 x 4 covariances (row / column 3 zero) with eigenvalues in [1e-3, 1]: R diag(w) R^T from a random rotation"""
    rng = np.random.default_rng(7500 + seed)
    q, _ = np.linalg.qr(rng.normal(size=(m, 3, 3)))
    w = np.exp(rng.uniform(np.log(1e-3), 0.0, (m, 3)))
    c = np.einsum("nij,nj,nkj->nik", q, w, q)
    out = np.zeros((m, 4, 4))
    out[:, :3, :3] = 0.5 * (c + c.transpose(0, 2, 1))
    return out


def run_structure(sorted_ids):
    """From the cell ids in sorted key order: (number of voxels, runs that cross a 64-key boundary, runs that cross a 256-key boundary,
    256-key blocks without a voxel start)."""
    ids = np.asarray(sorted_ids)
    m = ids.shape[0]
    start = np.ones(m, bool)
    start[1:] = ids[1:] != ids[:-1]
    first = np.nonzero(start)[0]
    last = np.append(first[1:], m) - 1
    blocks = (m + 255) // 256
    return int(first.size), int((first // 64 != last // 64).sum()), int((first // 256 != last // 256).sum()), int(blocks - np.unique(first // 256).size)


# ------------------------------------------------------------------------------------------------ VoxelGrid geometry scenes
# every scene: (frames, rel_poses, leaf) with frames = [(xyz float32 [n, 3], label float32 [n])], as setInputTargetSubmap takes them

EYE = np.eye(4)


def _pose(t, rpy_deg):
    r, p, y = np.deg2rad(rpy_deg)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])
    T[:3, 3] = t
    return T


def _one(xyz, lab, leaf):
    return [(np.ascontiguousarray(xyz, f32), np.ascontiguousarray(lab, f32))], [EYE], leaf


def _cloud(n, rng, span=6.0):
    return rng.uniform(-span, span, (n, 3)).astype(f32)


def g_straddle_zero(rng):
    """coordinates in (-leaf, leaf) around the origin, with -0.0 and +0.0 among them: floor(-0.0) is cell 0, a tiny negative cell -1"""
    leaf = 0.5
    xyz = rng.uniform(-leaf, leaf, (600, 3)).astype(f32)
    xyz[np.abs(xyz) >= leaf] = f32(0.25)
    zeros = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0], [-1e-30, 1e-30, -0.0], [1e-30, -1e-30, 0.0]], f32)
    xyz = np.concatenate([xyz, zeros])[rng.permutation(606)]
    return _one(xyz, labels(606, 1), leaf)


def g_faces_half(rng):
    """every coordinate is k * 0.5 at leaf 0.5: all points lie exactly on cell faces (and corners); the products x * inv are exact"""
    xyz = (rng.integers(-12, 13, (1500, 3)).astype(f32) * f32(0.5)).astype(f32)
    return _one(xyz, labels(1500, 2), 0.5)


def g_faces_tenth(rng):
    """float32(k) * float32(0.1) at leaf 0.1: the product with the float inverse leaf rounds to k or just beside it"""
    xyz = (rng.integers(-40, 41, (1500, 3)).astype(f32) * f32(0.1)).astype(f32)
    return _one(xyz, labels(1500, 3), 0.1)


def g_offset_1e5(rng):
    """a cloud 1e5 m from the origin on every axis, where floats are 1/128 m apart: half of it spread over metres, half within
    centimetres, so that many points coincide; every x * inv is a large float"""
    xyz = (rng.normal(0.0, 1.0, (2000, 3)) * np.repeat([[1.5], [0.02]], 1000, axis=0) + np.array([1.0e5, -1.0e5, 1.0e5])).astype(f32)
    xyz = xyz[rng.permutation(2000)]
    return _one(xyz, labels(2000, 4), 0.1)


def g_duplicates(rng):
    """100 exact copies of one point stacked on a background cloud"""
    xyz = np.concatenate([_cloud(400, rng), np.tile(np.array([[1.3, -0.7, 0.2]], f32), (100, 1))])[rng.permutation(500)]
    return _one(xyz, labels(500, 5), 0.5)


def g_line(rng):
    """y = z = 0: div_b = 1 on two axes"""
    xyz = np.zeros((700, 3), f32)
    xyz[:, 0] = rng.uniform(-30.0, 30.0, 700)
    return _one(xyz, labels(700, 6), 0.5)


def g_plane(rng):
    """z constant: div_b = 1 on one axis"""
    xyz = _cloud(1200, rng, 12.0)
    xyz[:, 2] = f32(-1.5)
    return _one(xyz, labels(1200, 7), 0.5)


def g_labels_cancel(rng):
    """labels +1 and -1: in the voxels of the first 40 lattice cells they cancel to zero (two of each), elsewhere they do not"""
    cells = _lattice_cells(64, rng)
    pts = _inside(np.repeat(cells, 4, axis=0), rng, 0.5, 0.0)
    lab = np.tile(np.array([1.0, -1.0, 1.0, -1.0], f32), 64)
    lab[160:] = rng.choice(np.array([-1.0, 1.0], f32), 96)
    lab[160::4] = lab[161::4] = lab[162::4] = 1.0  # at most one -1 in these voxels: the sum is 2 or 4
    perm = rng.permutation(256)
    return _one(pts[perm], lab[perm], 0.5)


def g_labels_zero(rng):
    return _one(_cloud(900, rng), np.zeros(900, f32), 0.5)


def _bad_point(k):
    return np.array([[np.nan, 1.0, 2.0], [1.0, np.inf, 2.0], [1.0, 2.0, -np.inf]], f32)[k % 3]


def g_nonfinite_first(rng):
    xyz = _cloud(513, rng)
    xyz[0] = _bad_point(0)
    return _one(xyz, labels(513, 8), 0.5)


def g_nonfinite_last(rng):
    xyz = _cloud(513, rng)
    xyz[-1] = _bad_point(1)
    return _one(xyz, labels(513, 9), 0.5)


def _frames(sizes, rng, seed):
    frames = [(_cloud(n, rng), labels(n, seed + i)) for i, n in enumerate(sizes)]
    rel = [_pose([0.4 * i, -0.3 * i, 0.05 * i], [0.5 * i, -0.7 * i, 11.0 * i]) for i in range(len(sizes))]
    return frames, rel


def g_frame_all_nonfinite(rng):
    """three keyframes, the middle one without a single finite point"""
    frames, rel = _frames((300, 130, 257), rng, 20)
    bad = np.stack([_bad_point(i) for i in range(130)])
    frames[1] = (bad, frames[1][1])
    return frames, rel, 0.5


def g_empty_frame(rng):
    """three keyframes, the middle one empty"""
    frames, rel = _frames((300, 0, 257), rng, 30)
    return frames, rel, 0.5


def g_frame_sizes(rng):
    """keyframes of 1, 255, 256 and 257 points under different poses: submap_transform_kernel's grid is sized by the largest frame"""
    frames, rel = _frames((1, 255, 256, 257), rng, 40)
    return frames, rel, 0.5


GEOMETRY = dict(straddle_zero=g_straddle_zero, faces_half=g_faces_half, faces_tenth=g_faces_tenth, offset_1e5=g_offset_1e5, duplicates=g_duplicates,
                line=g_line, plane=g_plane, labels_cancel=g_labels_cancel, labels_zero=g_labels_zero, nonfinite_first=g_nonfinite_first,
                nonfinite_last=g_nonfinite_last, frame_all_nonfinite=g_frame_all_nonfinite, empty_frame=g_empty_frame, frame_sizes=g_frame_sizes)


def geometry(name):
    return GEOMETRY[name](np.random.default_rng(7600 + sorted(GEOMETRY).index(name)))


# ------------------------------------------------------------------------------------------------ VoxelGrid limit scenes

def _box_points(lo, hi, extra):
    """the 8 corners of [lo, hi] and `extra` [k, 3] further points inside, in a fixed interleaved order"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)])
    pts = np.concatenate([corners, np.asarray(extra, np.float64).reshape(-1, 3)])
    order = np.random.default_rng(7700).permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(f32))


def grid_limit(name):
    """(frames, rel, leaf, expect_voxel_branch).  d = (int64)((max - min) inv) + 1 is PCL's overflow test, div_b = floor(max inv) -
    floor(min inv) + 1 the grid the indices use.
      fits          d = div_b = (46340, 46340, 1): 2 147 395 600 cells, the voxel branch; the top corner cell holds four points, its
                    id 2 147 395 599 sets bit 61 of the key
      overflow      d = (46341, 46341, 1): 2 147 488 281 > INT_MAX, the input is returned unchanged
      divb_leaf1    d = (46340, 46340, 1) passes, div_b = (46341, 46341, 2) does not: PCL overflows a signed int there; defined here as
                    the pass-through
      divb_leaf01   the same corner at leaf 0.1, every coordinate / 10"""
    if name == "fits":
        lo, hi, leaf = (0.25, 0.25, 0.25), (46339.75, 46339.75, 0.75), 1.0
        extra = [[46339.5, 46339.25, 0.5], [46339.25, 46339.5, 0.3], [0.5, 0.5, 0.5], [0.7, 46339.5, 0.5], [23000.5, 23000.5, 0.5], [23000.25, 23000.75, 0.6]]
        voxel = True
    elif name == "overflow":
        lo, hi, leaf = (0.25, 0.25, 0.25), (46340.75, 46340.75, 0.75), 1.0
        extra = [[46340.5, 46340.25, 0.5], [0.5, 0.5, 0.5], [23000.5, 23000.5, 0.5], [23000.25, 23000.75, 0.6]]
        voxel = False
    elif name == "divb_leaf1":
        lo, hi, leaf = (0.5, 0.5, 0.95), (46340.4, 46340.4, 1.05), 1.0
        extra = [[46340.2, 46340.3, 1.01], [0.75, 0.6, 0.97], [23000.5, 23000.5, 0.99], [23000.25, 23000.75, 1.02]]
        voxel = False
    elif name == "divb_leaf01":
        lo, hi, leaf = (0.05, 0.05, 0.095), (4634.04, 4634.04, 0.105), 0.1
        extra = [[4634.02, 4634.03, 0.101], [0.075, 0.06, 0.097], [2300.05, 2300.05, 0.099], [2300.025, 2300.075, 0.102]]
        voxel = False
    else:
        raise KeyError(name)
    xyz = _box_points(lo, hi, extra)
    frames, rel, leaf = _one(xyz, labels(len(xyz), 50), leaf)
    return frames, rel, leaf, voxel


GRID_LIMITS = ("fits", "overflow", "divb_leaf1", "divb_leaf01")


def grid_dims(xyz, leaf):
    """(d, div_b, min_b) of pcl::VoxelGrid for finite float32 points, in the float arithmetic of voxel_grid.hpp, as int64"""
    inv = f32(1.0) / f32(leaf)
    mn, mx = xyz.min(axis=0), xyz.max(axis=0)
    d = ((mx - mn) * inv).astype(np.int64) + 1
    min_b = np.floor(mn * inv).astype(np.int64)
    div_b = np.floor(mx * inv).astype(np.int64) - min_b + 1
    return d, div_b, min_b


# ------------------------------------------------------------------------------------------------ FastVGICP scenes (resolution 1.0)

def vgicp_geometry(name):
    """float32 targets for the Gaussian voxel map: `faces` puts every coordinate on (k + 0.5) res, the face of floor(x / res - 0.5)"""
    rng = np.random.default_rng(7800 + sorted(VGICP_GEOMETRY).index(name))
    if name == "faces":
        return np.ascontiguousarray((rng.integers(-12, 13, (1500, 3)) + 0.5).astype(f32))
    return np.concatenate([f[0] for f in geometry(name)[0]])


VGICP_GEOMETRY = ("duplicates", "faces", "line", "offset_1e5", "plane", "straddle_zero")
VG_HALF = 1024  # the box of the limit scenes spans the voxel coordinates -1024 .. 1023: |coordinate| <= 2048 m


def vgicp_limit(name):
    """(target, accepted).  Voxel coordinate c holds x in [c + 0.5, c + 1.5), its centre is c + 1.
      box_2047     2048 x 2048 x 2047 occupied box: 2^33 - 2^22 cells, accepted; the top corner voxel (1023, 1023, 1022) is occupied
                   and carries the largest id, 2^33 - 2^22 - 1, whose key has bit 63 set
      box_2048     2048^3 = 2^33 cells: refused (the id is packed into 33 bits)
      coord_2pow30 one coordinate whose voxel coordinate reaches 2^30: refused"""
    lo = -VG_HALF + 1.0  # centre of voxel -1024
    hi = VG_HALF + 0.0   # centre of voxel 1023
    if name == "box_2047":
        top = (hi, hi, hi - 1.0)
        extra = [[hi + 0.25, hi - 0.25, hi - 1.25], [hi, hi, lo], [lo + 0.25, lo, lo - 0.25], [0.0, 0.0, 0.0], [0.25, -0.25, 0.1], [hi, lo, 0.0], [lo, hi, hi - 1.0], [hi - 1.0, hi, hi - 1.0]]
        return _box_points((lo, lo, lo), top, extra), True
    if name == "box_2048":
        extra = [[hi + 0.25, hi - 0.25, hi - 0.25], [0.0, 0.0, 0.0], [0.25, -0.25, 0.1], [hi, lo, 0.0]]
        return _box_points((lo, lo, lo), (hi, hi, hi), extra), False
    if name == "coord_2pow30":
        pts = _cloud(16, np.random.default_rng(7900))
        pts[5, 1] = f32(2.0 ** 30 + 128.0)
        return pts, False
    raise KeyError(name)


VGICP_LIMITS = ("box_2047", "box_2048", "coord_2pow30")


def vgicp_probe_source(coords):
    """a few dozen float32 source points (resolution 1.0) in and just outside the lowest-id voxel, the highest-id voxel and the eight
    corners of the box of the occupied voxel coordinates `coords` [nv, 3] (ascending id order): voxel centres and points 0.75 away"""
    coords = np.asarray(coords, np.float64)
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    pts = []
    for c in range(8):
        corner = np.array([(lo, hi)[(c >> a) & 1][a] for a in range(3)])
        out = np.array([1.0 if (c >> a) & 1 else -1.0 for a in range(3)])
        centre = corner + 1.0
        pts += [centre, centre + 0.75 * out, centre - 0.75 * out]
        for a in range(3):
            e = np.zeros(3)
            e[a] = out[a]
            pts.append(centre + 0.75 * e)
    for v in (coords[0], coords[-1]):
        pts += [v + 1.0, v + 1.0 + [0.75, 0.0, 0.0], v + 1.0 - [0.75, 0.0, 0.0], v + 1.0 + [0.0, 0.0, 0.75], v + 1.0 - [0.0, 0.75, 0.0]]
    return np.ascontiguousarray(np.array(pts).astype(f32))


def vgicp_target(key):
    """the target of a FastVGICP case: (regime, m), a name of VGICP_GEOMETRY or a name of VGICP_LIMITS"""
    if isinstance(key, tuple):
        return regime(key[0], key[1], cell=1.0, phase=0.5)
    return vgicp_limit(key)[0] if key in VGICP_LIMITS else vgicp_geometry(key)


# ------------------------------------------------------------------------------------------------ NDT limit scenes (resolution 1.0)

def ndt_limit(name):
    """(target, accepted).  box_1290: div_b = 1290^3 = 2 146 689 000 <= INT_MAX, the top corner leaf (id 1290^3 - 1) holds 8 points;
    box_1291: 1291^3 = 2 151 685 171, refused."""
    side = {"box_1290": 1290, "box_1291": 1291}[name]
    lo, hi = 0.25, side - 0.25
    rng = np.random.default_rng(8000)
    top = side - 1 + rng.uniform(0.3, 0.7, (7, 3))
    low = rng.uniform(0.3, 0.7, (6, 3))
    return _box_points((lo, lo, lo), (hi, hi, hi), np.concatenate([top, low, [[600.5, 600.5, 600.5]]])), side == 1290


NDT_LIMITS = ("box_1290", "box_1291")
NDT_CASES = [(r, m) for r in ("own_cell", "mixed") for m in (255, 256, 257) + SIZES_LARGE] + [("one_cell", 4097)]
