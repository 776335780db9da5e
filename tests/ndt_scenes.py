"""Target / source scenes shared by tests/test_ndt_restatement.py (CPU) and tests/test_ndt_gpu.py: small, seeded, and built so that
every rule of the voxel map (VGC:60-370) meets at least one leaf."""
import importlib
import os

import numpy as np

synth = importlib.import_module("go-rio_amd.synth")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_lidar_pair.npz")
f32 = np.float32


def clusters(n, seed, offset=0.0, span=15.0):
    """n points in flat Gaussian clusters (about 16 per cluster) over [-span, span]^3 + offset: negative coordinates included."""
    rng = np.random.default_rng(seed)
    k = n // 16 + 1
    centres = rng.uniform(-span, span, (k, 3))
    pts = centres[rng.integers(0, k, n)] + rng.normal(0.0, 1.0, (n, 3)) * np.array([0.3, 0.3, 0.06])
    return (pts + offset).astype(f32)


def real_pair():
    """(source, target, T): two disjoint samples of one real LiDAR scan, the target moved by a known 0.3 m / 2 degree transform."""
    g = np.load(GOLD)
    a0, a1 = g["a_0"][:, :3].copy(), g["a_1"][:, :3].copy()
    T = synth.gt_transform([0.30, -0.20, 0.05], [0.5, -0.4, 2.0])
    moved = (a1.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32)
    return a0, moved, T


def with_nonfinite(pts, seed):
    """Every 7th point replaced by one with a NaN, +Inf or -Inf coordinate."""
    rng = np.random.default_rng(seed)
    out = pts.copy()
    bad = np.arange(3, out.shape[0], 7)
    vals = np.array([np.nan, np.inf, -np.inf], f32)
    out[bad, rng.integers(0, 3, bad.size)] = vals[rng.integers(0, 3, bad.size)]
    return out


def rule_scene():
    """Leaves that meet one rule each (resolution 1.0), coordinates are short binary fractions so the sums are exact:
    cell (0,0,0) five points, (2,0,0) six points, (4,0,0) eight collinear points along x, (6,0,0) six coincident points,
    (0,3,0) a generic 12-point leaf, (-3,-2,-1) a generic leaf at negative coordinates.  Returns (points, dict name -> cell)."""
    rng = np.random.default_rng(5)
    gen = lambda cell, n: (np.array(cell) + 0.5 + rng.uniform(-0.4, 0.4, (n, 3)))
    five, six = gen((0, 0, 0), 5), gen((2, 0, 0), 6)
    line = np.stack([4.0 + 0.125 * np.arange(8), np.full(8, 0.5), np.full(8, 0.25)], axis=1)
    same = np.tile(np.array([[6.5, 0.5, 0.25]]), (6, 1))
    pts = np.concatenate([five, six, line, same, gen((0, 3, 0), 12), gen((-3, -2, -1), 12)])
    perm = rng.permutation(pts.shape[0])  # leaves interleaved in the input
    cells = {"five": (0, 0, 0), "six": (2, 0, 0), "line": (4, 0, 0), "same": (6, 0, 0), "generic": (0, 3, 0), "negative": (-3, -2, -1)}
    return pts[perm].astype(f32), cells


def leaf_of(vm_min_b, vm_div_b, cell):
    """Linear leaf index of an integer cell (VGC:223)."""
    r = np.array(cell) - np.asarray(vm_min_b)
    return int(r[0] + r[1] * vm_div_b[0] + r[2] * vm_div_b[0] * vm_div_b[1])


def smooth_scene():
    """A target of eight compact blobs, each well inside one cell, and a source near the blob centres: under DIRECT1 and the small
    poses of the tests no source point changes its cell, so the score is a smooth function of the pose."""
    rng = np.random.default_rng(11)
    cells = np.array([(i, j, k) for i in (-2, 1) for j in (-2, 1) for k in (-1, 0)], float)
    tgt = np.concatenate([c + 0.5 + np.clip(rng.normal(0, 0.12, (200, 3)) * np.array([1.0, 0.6, 0.3]), -0.4, 0.4) for c in cells])
    src = np.concatenate([c + 0.5 + rng.uniform(-0.15, 0.15, (40, 3)) for c in cells])
    return src.astype(f32), tgt.astype(f32)


def radar_pair(n=4096, seed=3):
    """A synthetic radar pair of go-rio_amd/synth.py: (source, target, T)."""
    sx, _, tx, _, T = synth.scan_pair(n, n, seed=seed)
    return sx, tx, T


def poses(src, vm_leaf_extent):
    """Named pose vectors for the derivative tests; vm_leaf_extent = (lo, hi) corners of the grid in metres."""
    lo, hi = np.asarray(vm_leaf_extent[0], float), np.asarray(vm_leaf_extent[1], float)
    far = float(np.abs(np.concatenate([lo, hi])).max() + np.abs(src).max() + 10.0)
    mid = np.median(src.astype(np.float64), axis=0)
    third = np.sort(src[:, 0].astype(np.float64))[(2 * src.shape[0]) // 3]  # a shift in x that carries the upper third beyond hi[0]
    return {
        "identity": np.zeros(6),
        "below_switch": np.array([0.01, -0.02, 0.005, 0.9e-4, -0.99e-4, 0.5e-4]),
        "above_switch": np.array([0.01, -0.02, 0.005, 1.01e-4, -1.1e-4, 1.5e-4]),
        "third_outside": np.array([hi[0] + 1.0 - third, 0.0, 0.0, 0.0, 0.0, 0.01]),
        "all_outside": np.array([far, far, 0.0, 0.0, 0.0, 0.0]) + 0 * mid[0],
        "typical": np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03]),
    }
