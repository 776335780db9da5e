"""Scenes shared by the FastGICP / FastVGICP tests (CPU restatement tests and GPU parity tests use the same ones)."""
import importlib

import numpy as np

synth = importlib.import_module("go-rio_amd.synth")

C1_SEED = 20250704  # BASELINE config C1, the pair tests/test_apd_gpu.py uses


def c1_pair(n=5000, m=5000):
    """Independently sampled source / target of one scene (synth.scan_pair): the parity scene."""
    return synth.scan_pair(n, m, seed=C1_SEED)


def moved_copy_pair(n=5000):
    """The target is the source moved EXACTLY by T_gt (no resampling, no second noise draw): the known-transform recovery scene."""
    sx, sl, _, _, T = synth.scan_pair(n, 64, seed=C1_SEED)
    tx = (sx.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return sx, sl, tx, sl.copy(), T


def c3_pair(n=16384, m=100000):
    """BASELINE config C3 shape: one scan against a 100 k-point local map."""
    sx, sl = synth.radar_scan(n, seed=31)
    tx, tl = synth.local_map(m, seed=32)
    return sx, sl, tx, tl, synth.gt_transform()


def parity_pose():
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0.1, -0.1, 1.0])
    T[:3, 3] = [0.2, -0.05, 0.01]
    return T


def near_face_pose(src, resolution, point=17, eps=2.0 ** -24):
    """parity_pose() with its translation moved so that source point `point` lands `eps` metres above a voxel face on every axis
    (voxel faces are at (k + 0.5) * resolution, fast_vgicp_voxel.hpp:158-160)."""
    T = parity_pose()
    q = T[:3, :3] @ src[point].astype(np.float64) + T[:3, 3]
    face = (np.floor(q / resolution - 0.5) + 0.5) * resolution
    T[:3, 3] += face + eps - q
    return T


def face_distance(T, src, resolution):
    """distance [m] of every transformed source coordinate to its nearest voxel face"""
    q = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    f = q / resolution - 0.5
    return np.abs(f - np.round(f)) * resolution


def shared_source():
    """second source of the shared-target GPU test (against the C1 target)"""
    return synth.radar_scan(4000, seed=77)


def batch_pairs(count=16):
    """pairs of differing sizes with private targets for the batched FastVGICP test"""
    return [synth.scan_pair(2000 + 137 * q, 2100 + 91 * q, seed=500 + q) for q in range(count)]


def _fused_row(Trow, p):
    """((m0 x + m1 y) + m2 z) + m3 as a compiler that contracts multiply-adds would evaluate it: exact products, one rounding per add"""
    from fractions import Fraction as F

    a = Trow[0] * p[0]
    a = float(F(Trow[1]) * F(p[1]) + F(a))
    a = float(F(Trow[2]) * F(p[2]) + F(a))
    return a + Trow[3]


def straddling_case(src, max_points=400):
    """(pose, resolution, point index, axis): the defined, un-fused transform of that source point and the contracted one differ in the
    last place, and the resolution puts a voxel face between the two values -- a slot table computed with fused multiply-adds (or in
    another order) names another voxel for this point."""
    T = parity_pose()
    p = src.astype(np.float64)
    for i in range(min(max_points, len(p))):
        for ax in range(3):
            u = ((T[ax, 0] * p[i, 0] + T[ax, 1] * p[i, 1]) + T[ax, 2] * p[i, 2]) + T[ax, 3]
            f = _fused_row(T[ax], p[i])
            if u == f:
                continue
            hi = max(u, f)
            for k in range(3, 200):
                res = abs(hi) / (k + 0.5)
                if 0.3 < res < 3.0 and np.floor(u / res - 0.5) != np.floor(f / res - 0.5):
                    return T, float(res), i, ax
    raise AssertionError("no straddling point found")
