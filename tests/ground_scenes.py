"""Radar-like scans for the Patchwork++ tests: a sloped, noisy ground near z = -sensor_height, walls, poles and cars, weak returns
below the ground (what RNR removes), points outside the 1 - 50 m range, sparse far patches, and sequences in which the sensor moves
so that the adaptive thresholds and TGR act."""
import numpy as np


def _ground(rng, n, h, slope, r_max=48.0):
    r = np.sqrt(rng.uniform(1.2 ** 2, r_max ** 2, n))
    t = rng.uniform(-np.pi, np.pi, n)
    x, y = r * np.cos(t), r * np.sin(t)
    z = -h + slope[0] * x + slope[1] * y + rng.normal(0, 0.03, n)
    return np.stack([x, y, z], 1), rng.uniform(0.2, 1.0, n)


def _box(rng, n, c, size, h):
    p = rng.uniform(-0.5, 0.5, (n, 3)) * np.array(size) + np.array([c[0], c[1], -h + size[2] / 2])
    return p, rng.uniform(0.3, 1.0, n)


def _wall(rng, n, a, b, height, h):
    s = rng.uniform(0, 1, n)
    p = np.array(a)[None, :] * (1 - s[:, None]) + np.array(b)[None, :] * s[:, None]
    z = -h + rng.uniform(0.0, height, n)
    return np.stack([p[:, 0] + rng.normal(0, 0.02, n), p[:, 1] + rng.normal(0, 0.02, n), z], 1), rng.uniform(0.3, 1.0, n)


def scan(seed, n_ground=3000, h=0.7, slope=(0.004, -0.003), offset=(0.0, 0.0), extras=True):
    """One scan [n, 3] float32 and intensities [n] float32."""
    rng = np.random.default_rng(seed)
    parts = [_ground(rng, n_ground, h, slope)]
    ox, oy = offset
    if extras:
        parts.append(_wall(rng, 500, (6 - ox, -8 - oy), (6 - ox, 9 - oy), 3.0, h))           # a building face
        parts.append(_wall(rng, 300, (-15 - ox, 20 - oy), (12 - ox, 22 - oy), 4.0, h))
        for k in range(6):                                                            # poles
            c = rng.uniform(-30, 30, 2)
            parts.append(_box(rng, 40, c, (0.2, 0.2, 3.0), h))
        for k in range(4):                                                            # cars
            c = rng.uniform(-20, 20, 2)
            parts.append(_box(rng, 150, c, (4.0, 1.8, 1.5), h))
        m = 60                                                                        # weak returns under the ground, steep and close
        r = rng.uniform(2.0, 4.0, m)
        t = rng.uniform(-np.pi, np.pi, m)
        parts.append((np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-2.4, -1.9, m)], 1), rng.uniform(0.0, 0.09, m)))
        m = 40                                                                        # strong returns 1.2 - 1.8 m under the ground
        r = rng.uniform(5.0, 30.0, m)
        t = rng.uniform(-np.pi, np.pi, m)
        parts.append((np.stack([r * np.cos(t), r * np.sin(t), -h - rng.uniform(1.2, 1.8, m)], 1), rng.uniform(0.3, 1.0, m)))
        m = 80                                                                        # outside (1, 50]
        r = np.concatenate([rng.uniform(0.1, 0.9, m // 2), rng.uniform(51, 80, m // 2)])
        t = rng.uniform(-np.pi, np.pi, m)
        parts.append((np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-1, 1, m)], 1), rng.uniform(0.2, 1.0, m)))
    xyz = np.concatenate([p[0] for p in parts]).astype(np.float32)
    inten = np.concatenate([p[1] for p in parts]).astype(np.float32)
    perm = rng.permutation(len(xyz))
    return xyz[perm], inten[perm]


def sparse_far_scan(seed, h=0.7):
    """Dense near field, a far zone with patches of 3 - 12 points: some patches fall below num_min_pts."""
    rng = np.random.default_rng(seed)
    xyz, inten = scan(seed, n_ground=1500, h=h)
    keep = np.hypot(xyz[:, 0], xyz[:, 1]) < 25.5
    far = []
    for k, cnt in enumerate([3, 7, 12, 9]):
        t = rng.uniform(k * np.pi / 2 + 0.1, (k + 1) * np.pi / 2 - 0.1, cnt)
        r = rng.uniform(26.5, 40, cnt)
        far.append(np.stack([r * np.cos(t), r * np.sin(t), -h + rng.normal(0, 0.03, cnt)], 1))
    far = np.concatenate(far).astype(np.float32)
    return np.concatenate([xyz[keep], far]), np.concatenate([inten[keep], rng.uniform(0.2, 1, len(far)).astype(np.float32)])


def sequence(seed, frames=24, n_ground=3000, h=0.7):
    """A sensor driving forward 0.8 m per frame, with the ground's slope drifting."""
    out = []
    for f in range(frames):
        out.append(scan(seed * 1000 + f, n_ground=n_ground, h=h, slope=(0.004 + 0.0003 * f, -0.003), offset=(0.8 * f, 0.0)))
    return out


def plane_scan(seed, n=2000, normal=(0.0, 0.0, 1.0), d=0.7, r_max=9.0):
    """Noiseless plane n.p + d = 0 in the first rings (for closed-form checks)."""
    rng = np.random.default_rng(seed)
    nrm = np.asarray(normal, np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    r = np.sqrt(rng.uniform(1.5 ** 2, r_max ** 2, n))
    t = rng.uniform(-np.pi, np.pi, n)
    x, y = r * np.cos(t), r * np.sin(t)
    z = -(d + nrm[0] * x + nrm[1] * y) / nrm[2]
    return np.stack([x, y, z], 1).astype(np.float32), np.full(n, 0.5, np.float32)


def large_scan(seed, n=60000, h=0.7):
    """A dense LiDAR-like scan: most of its points in a few near patches, so patches exceed the LDS sort size."""
    rng = np.random.default_rng(seed)
    xyz, inten = scan(seed, n_ground=2000, h=h)
    m = n - len(xyz)
    r = np.sqrt(rng.uniform(1.2 ** 2, 11.0 ** 2, m))
    t = rng.uniform(-np.pi, np.pi, m)
    g = np.stack([r * np.cos(t), r * np.sin(t), -h + rng.normal(0, 0.03, m)], 1).astype(np.float32)
    return np.concatenate([xyz, g]), np.concatenate([inten, rng.uniform(0.2, 1, m).astype(np.float32)])
