"""Seeded scenes for the spatial index and its searches (the CPU tests that pin the oracle on them and the GPU boundary tests
use the same ones).

Every generator takes the point count `n` and a seed and returns float32 xyz [n, 3] with FINITE coordinates, in a shuffled order:
the position of a point in the array says nothing about where it lies.  Non-finite coordinates are out of scope -- the
reference's callers filter them before registration and the oracle defines nothing for them.

What each scene is for (the index is a Morton sort with ONE cubic cell size from the widest axis and 11 bits per axis, refined by
median splits along the widest axis of every chunk; ties go to the lowest original index):

  line              y = z = 0 exactly: zero extent on two axes, every box is a segment
  plane             z constant: zero extent on one axis
  lattice3d         integer lattice: equal distances everywhere (an interior point has 27 points within its 20th distance),
                    equal minima in different tiles for a query half a cell off
  lattice3d_dup     the same with exact duplicates appended, so that the duplicates carry the higher indices
  cluster_outliers  n - 8 points with sigma = 1 cm and 8 points uniform in +-1 km: thousands of points share a Morton code
  two_clusters      two dense blobs 500 m apart: the same, twice, with an empty code range in between
  offset            a radar scan shifted by about 1e5 m on x and y, where the float spacing is 1/128 m
  radar             synth.radar_scan unchanged: the control
"""
import importlib

import numpy as np

synth = importlib.import_module("go-rio_amd.synth")

K = 20  # k_correspondences of the shipped launch files
TIE_BUFFER = K + 4  # knn_collect_kernel buffers this many candidates up to the k-th distance; more send the wave to the insertion kernel


def _shuffled(xyz, rng):
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))], dtype=np.float32)


def line(n, seed):
    rng = np.random.default_rng(seed)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, 0] = rng.uniform(0.0, 100.0, n)
    return _shuffled(xyz, rng)


def plane(n, seed):
    rng = np.random.default_rng(seed)
    xyz = np.empty((n, 3), np.float32)
    xyz[:, 0] = rng.uniform(0.0, 80.0, n)
    xyz[:, 1] = rng.uniform(-40.0, 40.0, n)
    xyz[:, 2] = np.float32(-1.5)
    return _shuffled(xyz, rng)


def _lattice_points(n):
    """the first n points (x fastest) of the smallest integer cube that holds n: the cut leaves a partial layer on top"""
    side = 1
    while side ** 3 < n:
        side += 1
    i = np.arange(n)
    return np.stack([i % side, (i // side) % side, i // (side * side)], axis=1).astype(np.float32)


def lattice3d(n, seed):
    return _shuffled(_lattice_points(n), np.random.default_rng(seed))


DUP_SHARE, DUP_STACK = 0.2, 8


def lattice3d_dup(n, seed):
    """lattice of n - n_dup points, shuffled, then n_dup exact copies behind them (so that a copy always has a higher index than its
    original), DUP_STACK copies of each chosen lattice point, in shuffled order.  Stacks rather than single copies: one or two copies
    near a query only pull its 20th distance in (19 lattice points lie within d^2 = 2), a stack of eight puts every lattice point
    within d^2 = 2 of it over TIE_BUFFER."""
    rng = np.random.default_rng(seed)
    n_dup = int(n * DUP_SHARE)
    base = _shuffled(_lattice_points(n - n_dup), rng)
    picks = np.repeat(rng.choice(len(base), -(-n_dup // DUP_STACK), replace=False), DUP_STACK)[:n_dup]
    return np.ascontiguousarray(np.concatenate([base, base[rng.permutation(picks)]]), dtype=np.float32)


N_OUTLIERS = 8


def cluster_outliers(n, seed):
    rng = np.random.default_rng(seed)
    blob = rng.normal(0.0, 0.01, (n - N_OUTLIERS, 3)) + np.array([3.0, -2.0, 0.5])
    far = rng.uniform(-1000.0, 1000.0, (N_OUTLIERS, 3))
    return _shuffled(np.concatenate([blob, far]).astype(np.float32), rng)


def two_clusters(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, 0.5, (n // 2, 3)) + np.array([10.0, 0.0, 0.0])
    b = rng.normal(0.0, 0.5, (n - n // 2, 3)) + np.array([510.0, 0.0, 0.0])
    return _shuffled(np.concatenate([a, b]).astype(np.float32), rng)


OFFSET = np.array([1.0e5, -1.0e5, 0.0], np.float32)


def offset(n, seed):
    xyz, _ = synth.radar_scan(n, seed=seed)
    return np.ascontiguousarray(xyz + OFFSET, dtype=np.float32)  # float32 addition: x and y land on the 1/128 m grid


def radar(n, seed):
    return synth.radar_scan(n, seed=seed)[0]


SCENES = dict(line=line, plane=plane, lattice3d=lattice3d, lattice3d_dup=lattice3d_dup, cluster_outliers=cluster_outliers,
              two_clusters=two_clusters, offset=offset, radar=radar)
KNN_TIE_SCENES = ("lattice3d", "lattice3d_dup")  # a stated share of queries has more than TIE_BUFFER points within the k-th distance
KNN_SELECT_SCENES = ("radar", "plane", "line", "offset")  # no query has: these prove the selection path, not the fallback
NN_TIE_SCENES = ("lattice3d", "lattice3d_dup")  # a query half a cell off is equidistant from eight lattice points
RANK_DEFICIENT = ("line", "plane", "lattice3d", "lattice3d_dup")  # neighbourhoods without a unique plane: compare the lists, not the covariances

HALF_UNIT = np.array([0.5, 0.5, 0.5], np.float32)


def make(name, n, seed=0):
    return SCENES[name](n, 1000 + seed)


def shifted(xyz):
    """the scene moved by half a unit on every axis: the queries of the 1-NN tests (rounded to float32, as every cloud is)"""
    return np.ascontiguousarray(xyz + HALF_UNIT, dtype=np.float32)


def within_kth(sqd_wide, k=K):
    """per query, how many points lie within its k-th distance, from an oracle k-NN run with more than k columns (the count saturates
    at the number of columns, which is all a comparison with TIE_BUFFER needs)"""
    return (sqd_wide <= sqd_wide[:, k - 1 : k]).sum(axis=1)


def natural_qpw(cloud_sizes):
    """queries per wave that the selection kernels use for one covariance call over these clouds (the rule of run_covariances:
    halved while the call has fewer waves than the chip has SIMDs)"""
    w64 = sum((n + 63) // 64 for n in cloud_sizes)
    qpw = 64
    while qpw > 8 and w64 * (64 // qpw) < 1024:
        qpw //= 2
    return qpw
