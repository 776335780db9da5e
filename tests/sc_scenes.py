"""Keyframe scans for the Scan Context tests: a loop trajectory through the synthetic radar scene (go-rio_amd/synth.py), driven
twice, the second lap revisiting the first lap's places, some with a yaw offset of 1 - 3 sectors.  Intensity is a function of the
object hit plus noise.  Points in the band where the reading of abs() matters (|azimuth| in (56.5, 57) deg, see include/gorio_sc.h)
are dropped, except where a test asks for them."""
import importlib

import numpy as np

synth = importlib.import_module("go-rio_amd.synth")
UNIT_SECTOR_DEG = 113.0 / 20.0  # 2 * 56.5 / 20
CENTER, RADIUS = np.array([55.0, 0.0]), 22.0


def sensor_pose(theta, yaw_offset_deg=0.0, jitter=(0.0, 0.0)):
    """On the circle at angle theta, heading along the tangent (counter-clockwise) plus yaw_offset_deg."""
    p = CENTER + RADIUS * np.array([np.cos(theta), np.sin(theta)]) + np.asarray(jitter)
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0.0, 0.0, np.rad2deg(theta + np.pi / 2) + yaw_offset_deg])
    T[:2, 3] = p
    return T


def intensity_of(label, rng):
    """A per-object intensity (ground and every box differ) plus noise."""
    base = np.where(label == 0, 0.5, 4.0 + 3.0 * label)
    return (base + rng.normal(0.0, 0.4, label.shape)).astype(np.float32)


def drop_abs_band(xyz, inten, azimuth_range=56.5):
    a = np.arctan2(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64))
    az = np.abs(np.rad2deg(a - np.pi / 2))
    keep = ~((az > azimuth_range - 0.05) & (az < np.floor(azimuth_range) + 1.05))
    return xyz[keep], inten[keep]


def keyframe(theta, seed, n_points=2000, yaw_offset_deg=0.0, jitter=(0.0, 0.0)):
    rng = np.random.default_rng(seed + 7919)
    xyz, label = synth.radar_scan(n_points, seed, sensor_pose=sensor_pose(theta, yaw_offset_deg, jitter))
    return drop_abs_band(xyz, intensity_of(label, rng))


def loop_sequence(n_lap=80, seed=11, n_points=2000):
    """[(xyz, intensity)] of 2 n_lap keyframes: lap 1 at theta_k = 2 pi k / n_lap, lap 2 over the same places with a small position
    jitter, every third keyframe yawed by 1 - 3 sectors.  Returns (scans, info) with info[k] = (lap, place, yaw offset in sectors)."""
    rng = np.random.default_rng(seed)
    scans, info = [], []
    for lap in range(2):
        for k in range(n_lap):
            theta = 2 * np.pi * k / n_lap
            m = 0
            jit = (0.0, 0.0)
            if lap == 1:
                jit = tuple(rng.normal(0.0, 0.3, 2))
                if k % 3 == 0:
                    m = int(rng.integers(1, 4)) * (1 if k % 2 else -1)
            scans.append(keyframe(theta, seed * 100003 + lap * 1009 + k, n_points, m * UNIT_SECTOR_DEG, jit))
            info.append((lap, k, m))
    return scans, info


def candidate_lists(n, seed=5, drop=0.25):
    """Per keyframe q, the keyframes before it with about `drop` of them left out, as a distance-based find_candidates would; so the
    lists change between snapshot rebuilds.  Every 7th list is cut short to at most 12 entries."""
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n):
        c = np.arange(q)
        c = c[rng.uniform(size=q) >= drop] if q > 3 else c
        if q % 7 == 3:
            c = c[-12:]
        if c.size == 0:
            c = np.array([max(q - 1, 0)])
        out.append(c.astype(np.int32))
    return out
