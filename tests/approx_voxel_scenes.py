"""Clouds shared by tests/test_approx_voxel_restatement.py (CPU) and tests/test_approx_voxel_gpu.py: small, seeded, each built to meet
one path of pcl::ApproximateVoxelGrid (tests/approx_voxel_restatement.py)."""
import numpy as np

import ndt_scenes

f32 = np.float32


def gaussian(n, seed, span=6.0, fields=4):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, fields)).astype(f32)
    p[:, :3] *= f32(span)
    return p


def buckets_512():
    """512 points in 512 different buckets (leaf 1): cells (k, 0, 0), k = 0 .. 511 -- 7171 is odd, so k * 7171 mod 512 is a
    permutation.  Only the final flush puts points out."""
    p = np.zeros((512, 4), f32)
    p[:, 0] = np.arange(512, dtype=f32) + f32(0.5)
    p[:, 1:3] = f32(0.25)
    p[:, 3] = np.arange(512, dtype=f32)
    rng = np.random.default_rng(11)
    return p[rng.permutation(512)]


def one_cell(n=5000, seed=12):
    """n points inside cell (0, 0, 0) of leaf 1: one run of n points, whose float sum depends on the order of every add."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.01, 0.99, (n, 4)).astype(f32)
    p[:, 3] = rng.standard_normal(n).astype(f32) * f32(100.0)
    return p


def alternating(n=4096):
    """Points alternating between cells (0, 0, 0) and (512, 0, 0) of leaf 1, which share bucket 0: every point but the first evicts."""
    rng = np.random.default_rng(13)
    p = rng.uniform(0.01, 0.99, (n, 4)).astype(f32)
    p[1::2, 0] += f32(512.0)
    return p


def hash_wrap(n=600, seed=14):
    """Cells around +-300000 per axis at leaf 0.5 (300000 * 7171 > 2^31: the bucket needs the 32-bit wrap), a few cells repeated."""
    rng = np.random.default_rng(seed)
    c = rng.integers(-3, 4, (n, 3)) + rng.choice([-300000, 300000], (n, 3))
    p = np.zeros((n, 4), f32)
    p[:, :3] = ((c + 0.5) * 0.5).astype(f32)  # cell centres: exact in float at this magnitude (multiples of 0.25 below 2^18)
    p[:, 3] = rng.standard_normal(n).astype(f32)
    return p


def ring_scan():
    """A ring-ordered synthetic scan: 16 rings x 1800 azimuths, r = 8 + 3 sin 3az, elevations -15 .. 15 degrees, ring after ring."""
    az = np.linspace(0.0, 2.0 * np.pi, 1800, endpoint=False)
    el = np.deg2rad(np.linspace(-15.0, 15.0, 16))
    r = 8.0 + 3.0 * np.sin(3.0 * az)
    x = (r[None, :] * np.cos(az)[None, :] * np.cos(el)[:, None]).reshape(-1)
    y = (r[None, :] * np.sin(az)[None, :] * np.cos(el)[:, None]).reshape(-1)
    z = (r[None, :] * np.sin(el)[:, None]).reshape(-1)
    inten = np.tile(np.cos(az), 16)
    return np.stack([x, y, z, inten], axis=1).astype(f32)


def xyzinormal(n, seed):
    """[n, 12] float32 rows laid out as pcl::PointXYZINormal; the padding floats carry a sentinel the filter must not touch or read."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 12)).astype(f32)
    p[:, :3] *= f32(4.0)
    p[:, [3, 7, 10, 11]] = f32(-77.0)
    return p


XYZINORMAL_OFFSETS = [0, 1, 2, 4, 5, 6, 8, 9]  # x y z | normal_x normal_y normal_z | intensity curvature


def same(a, b):
    """Equal shape and equal bits (NaN payloads and signed zeros included)."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# name -> (cloud, leaf): the cases of both test files
CLOUDS = {
    "n1": lambda: (gaussian(1, 1), 0.5),
    "n255": lambda: (gaussian(255, 2), 0.5),
    "n256": lambda: (gaussian(256, 3), 0.5),
    "n257": lambda: (gaussian(257, 4), 0.5),
    "n513": lambda: (gaussian(513, 5), 0.5),
    "buckets_512": lambda: (buckets_512(), 1.0),
    "one_cell": lambda: (one_cell(), 1.0),
    "alternating": lambda: (alternating(), 1.0),
    "hash_wrap": lambda: (hash_wrap(), 0.5),
    "gauss_3000": lambda: (gaussian(3000, 6, span=3.0), 0.5),
    "gauss_20000": lambda: (gaussian(20000, 7, span=5.0), 0.5),
    "ring_scan": lambda: (ring_scan(), 0.25),
    "real_target": lambda: (ndt_scenes.real_pair()[1], 0.5),
    "anisotropic": lambda: (gaussian(3000, 8, span=3.0), (0.25, 0.5, 1.0)),
    "fields_8": lambda: (gaussian(2000, 9, span=2.0, fields=8), 0.5),
    "fields_3": lambda: (gaussian(2000, 10, span=2.0, fields=3), 0.5),
}
