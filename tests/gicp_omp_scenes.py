"""Scenes of the GICP_OMP tests (tests/test_gicp_omp_restatement.py, tests/test_gicp_omp_gpu.py): small clouds at the sizes where the
covariance rule, the gate, the pair count and the two iteration caps take another path.  Every scene is a dict of source, target, guess
and the parameters that differ from the reference constructor's (gicp_omp.h:117-127).  Reference runs are computed once per process."""
import functools
import importlib
import os

import numpy as np

import gicp_omp_restatement as R

f32 = np.float32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_lidar_pair.npz")


def pose(t, rpy_deg):
    """float 4x4 of a translation and roll / pitch / yaw in degrees."""
    T = R.apply_state(np.concatenate([np.asarray(t, np.float64), np.deg2rad(np.asarray(rpy_deg, np.float64))]))
    return T.astype(f32)


def room(n, seed):
    """n points on a floor and two walls of a 10 m room with 1 cm noise: covariances with three distinct singular values almost everywhere."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 3, n)
    u, v = rng.uniform(-5, 5, n), rng.uniform(-5, 5, n)
    w = rng.normal(0, 0.01, n)
    pts = np.where((which == 0)[:, None], np.stack([u, v, w - 1.0], 1), np.where((which == 1)[:, None], np.stack([u, w + 5.0, 0.3 * v + 0.5], 1), np.stack([w - 5.0, u, 0.3 * v + 0.5], 1)))
    return pts.astype(f32)


def moved(pts, T, seed, noise=0.005):
    rng = np.random.default_rng(seed)
    q = pts.astype(np.float64) @ np.asarray(T, np.float64)[:3, :3].T + np.asarray(T, np.float64)[:3, 3]
    return (q + rng.normal(0, noise, q.shape)).astype(f32)


def lattice():
    """5 x 5 x 5 unit lattice: every k-NN list is full of equal distances."""
    g = np.arange(5, dtype=f32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).copy()


def few_pairs(n_near):
    """A 64-point target; a source of 20 points 100 m away (they find nothing inside max_correspondence_distance) and n_near points next to
    target points: exactly n_near pairs."""
    tgt = room(64, 11)
    far = room(20, 12) + f32(100.0)
    near = tgt[:n_near] + np.array([0.02, -0.01, 0.015], f32)
    return np.concatenate([far, near]).astype(f32), tgt


@functools.lru_cache(maxsize=None)
def scenes():
    T_small = pose([0.10, -0.06, 0.03], [0.4, -0.3, 1.0])
    a600 = room(600, 1)
    a300 = room(300, 2)
    s4, t4 = few_pairs(4)
    s3, t3 = few_pairs(3)
    n20 = room(20, 3)
    return {
        "general": dict(source=a600, target=moved(a600, T_small, 21), guess=pose([0.02, 0.01, -0.01], [0.0, 0.1, -0.3]), params={}),
        "k_equals_n": dict(source=n20, target=moved(n20, pose([0.01, 0.0, 0.0], [0, 0, 0.2]), 22), guess=np.eye(4, dtype=f32), params={}),
        "four_pairs": dict(source=s4, target=t4, guess=np.eye(4, dtype=f32), params=dict(max_correspondence_distance=0.5)),
        "three_pairs": dict(source=s3, target=t3, guess=pose([0.001, 0, 0], [0, 0, 0]), params=dict(max_correspondence_distance=0.5)),
        "no_pairs": dict(source=a300, target=moved(a300, T_small, 23), guess=pose([0.002, 0, 0], [0, 0, 0]), params=dict(max_correspondence_distance=1e-4)),
        "outer_cap": dict(source=a300, target=moved(a300, T_small, 24), guess=np.eye(4, dtype=f32), params=dict(max_iterations=1)),
        "inner_cap": dict(source=a300, target=moved(a300, T_small, 25), guess=np.eye(4, dtype=f32), params=dict(max_optimizer_iterations=1, max_iterations=6)),
        "identical": dict(source=a300, target=a300.copy(), guess=np.eye(4, dtype=f32), params={}),
    }


def make(scene, scale=1.0):
    g = R.GicpOmp(scale=scale, **scene["params"])
    g.set_target(scene["target"])
    g.set_source(scene["source"])
    return g


@functools.lru_cache(maxsize=None)
def reference(name):
    """(restatement object after its align, result) of a scene, computed once."""
    sc = scenes()[name]
    g = make(sc)
    return g, g.align(sc["guess"])


@functools.lru_cache(maxsize=None)
def is_stable(name):
    """The stability condition of the pose gate: every reduction scaled by (1 +- 1e-9) leaves the outer and inner counts as they are."""
    _, r0 = reference(name)
    for s in (1.0 + 1e-9, 1.0 - 1e-9):
        r = make(scenes()[name], s).align(scenes()[name]["guess"])
        if (r["nr_iterations"], r["inner_total"], r["converged"]) != (r0["nr_iterations"], r0["inner_total"], r0["converged"]):
            return False
    return True


def real_pair(n=1500):
    """Two disjoint samples of one real LiDAR scan thinned to n points each, the target moved by a known 0.3 m / 2 degree transform."""
    synth = importlib.import_module("go-rio_amd").synth
    g = np.load(GOLD)
    a0, a1 = g["a_0"][:, :3], g["a_1"][:, :3]
    a0 = a0[:: max(1, a0.shape[0] // n)][:n].copy()
    a1 = a1[:: max(1, a1.shape[0] // n)][:n].copy()
    T = synth.gt_transform([0.30, -0.20, 0.05], [0.5, -0.4, 2.0])
    return a0, (a1.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(f32), T


def pose_error(Ta, Tb):
    """(metres, radians) between two 4x4 poses."""
    d = np.linalg.inv(np.asarray(Ta, np.float64)) @ np.asarray(Tb, np.float64)
    c = min(1.0, max(-1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))
    return float(np.linalg.norm(d[:3, 3])), float(np.arccos(c))
