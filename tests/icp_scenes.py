"""Deterministic scenes of the ICP tests.  Sizes: sources of 3, 4, 255, 256, 257 and 513 points (below, at and above one 256-point block,
more than two blocks) against targets of about 300 and about 2 000 points.  Every align scene is admitted only if the restatement alone
decides each floating-point criterion with a relative margin above MARGIN (tests/test_icp_restatement.py checks all of them on the CPU;
the GPU tests run every scene, none is skipped).  Reference runs are computed once per process."""
import functools

import numpy as np

import icp_restatement as R

f32 = np.float32
MARGIN = 1e-6
SOURCE_SIZES = [3, 4, 255, 256, 257, 513]
TARGET_SIZES = [300, 2000]


def pose(t, rpy_deg):
    """float32 4x4 of a translation and roll / pitch / yaw in degrees (R = Rz Ry Rx)."""
    a, b, c = np.deg2rad(np.asarray(rpy_deg, np.float64))
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(f32)


def room(n, seed):
    """n points on a floor and two walls of a 10 m room with 1 cm noise."""
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


T_TRUE = pose([0.10, -0.06, 0.03], [0.4, -0.3, 1.0])  # target = T_TRUE * source


@functools.lru_cache(maxsize=None)
def target(m):
    return room(m, 100 + m)


@functools.lru_cache(maxsize=None)
def source(n, m):
    """n points that T_TRUE takes next to points of target(m) (drawn with repetition when n > m, each with its own 5 mm noise)."""
    tgt = target(m)
    pick = np.random.default_rng(7 * n + m).integers(0, tgt.shape[0], n)
    return moved(tgt[pick], np.linalg.inv(T_TRUE.astype(np.float64)), 1000 + n + m)


def step_cases():
    """(name, source, target, T, max_correspondence_distance, reciprocal) of the one-pass checks: a gate that drops some of the pairs (all
    of them pass it for the sources of 3 and 4 points, so that an estimate exists)."""
    out = []
    for m in TARGET_SIZES:
        for n in SOURCE_SIZES:
            for recip in (False, True):
                out.append(("step_%d_%d_%s" % (n, m, "recip" if recip else "plain"), source(n, m), target(m), pose([0.02, 0.01, -0.01], [0.0, 0.1, -0.3]), 1.0 if n <= 4 else 0.12, recip))
    return out


def two_pairs():
    """A 300-point target; a source of 20 points 100 m away and 2 next to target points: a gate of 0.5 m leaves exactly 2 pairs."""
    tgt = target(300)
    far = room(20, 12) + f32(100.0)
    near = tgt[:2] + np.array([0.02, -0.01, 0.015], f32)
    return np.concatenate([far, near]).astype(f32), tgt


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(source, target, guess, params): params are keyword arguments of icp_restatement.align."""
    I = np.eye(4, dtype=f32)
    g1 = pose([0.02, 0.01, -0.01], [0.0, 0.1, -0.3])
    s2, t2 = two_pairs()
    common = dict(max_iterations=60, transformation_epsilon=1e-5, max_correspondence_distance=1.0)  # gorio_apd_params are one per batch
    return {
        # PCL's constructor defaults but for the gate: ends by the iteration cap (state 1)
        "defaults_257": dict(source=source(257, 300), target=target(300), guess=I, params=dict(max_correspondence_distance=1.0)),
        "cap3_513_guess": dict(source=source(513, 2000), target=target(2000), guess=g1, params=dict(max_iterations=3, max_correspondence_distance=1.0)),
        # the transformation criterion (state 2): a step below 3.2 mm and 0.26 degrees
        "transform_256": dict(source=source(256, 2000), target=target(2000), guess=I, params=dict(max_iterations=60, transformation_epsilon=1e-5, max_correspondence_distance=1.0)),
        "transform_255_recip": dict(source=source(255, 300), target=target(300), guess=g1,
                                    params=dict(max_iterations=60, transformation_epsilon=1e-5, max_correspondence_distance=1.0, use_reciprocal=True)),
        # the relative MSE criterion (state 4)
        "relmse_513": dict(source=source(513, 300), target=target(300), guess=I, params=dict(max_iterations=60, euclidean_fitness_epsilon=1e-2, max_correspondence_distance=1.0)),
        "relmse_4_recip": dict(source=source(4, 300), target=target(300), guess=g1,
                               params=dict(max_iterations=40, euclidean_fitness_epsilon=1e-3, max_correspondence_distance=1.0, use_reciprocal=True)),
        # a rotation threshold of its own next to a loose translation one
        "roteps_257": dict(source=source(257, 2000), target=target(2000), guess=g1,
                           params=dict(max_iterations=60, transformation_epsilon=1e-4, transformation_rotation_epsilon=1.0 - 2e-5, max_correspondence_distance=0.5)),
        # three points: every other method refuses a cloud smaller than k_correspondences; ends by the absolute MSE criterion (state 3)
        "three_points": dict(source=source(3, 300), target=target(300), guess=I, params=dict(max_iterations=5, max_correspondence_distance=1.0)),
        # fewer than 3 pairs (state 5), at the first pass
        "two_pairs": dict(source=s2, target=t2, guess=I, params=dict(max_iterations=10, max_correspondence_distance=0.5)),
        # the members of the batch test: one set of gorio_apd_params, ICP parameters of their own
        "batch_257": dict(source=source(257, 300), target=target(300), guess=g1, params=dict(common)),
        "batch_two_pairs": dict(source=s2, target=t2, guess=I, params=dict(common)),
        "batch_256_relmse": dict(source=source(256, 2000), target=target(2000), guess=I, params=dict(common, euclidean_fitness_epsilon=0.9)),
        "batch_513_recip": dict(source=source(513, 300), target=target(300), guess=I, params=dict(common, use_reciprocal=True)),
        "batch_3": dict(source=source(3, 300), target=target(300), guess=I, params=dict(common)),
        "batch_513_roteps": dict(source=source(513, 2000), target=target(2000), guess=pose([0.3, -0.2, 0.1], [2.0, -1.0, 4.0]),
                                 params=dict(common, transformation_rotation_epsilon=1.0 - 5e-6)),
    }


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = scenes()[name]
    return R.align(sc["source"], sc["target"], sc["guess"], **sc["params"])


def batch():
    """The six members of the batch test: mixed sizes and ICP parameters, ending at different iterations, one in state 5; batch_257 and
    batch_513_recip register against one target."""
    return ["batch_257", "batch_two_pairs", "batch_256_relmse", "batch_513_recip", "batch_3", "batch_513_roteps"]


def pose_error(Ta, Tb):
    """(metres, radians) between two 4x4 poses."""
    d = np.linalg.inv(np.asarray(Ta, np.float64)) @ np.asarray(Tb, np.float64)
    Rm = d[:3, :3]
    v = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    return float(np.linalg.norm(d[:3, 3])), float(np.arctan2(np.linalg.norm(v), (np.trace(Rm) - 1.0) / 2.0))
