"""Two keyframe databases for the cross-database Scan Context tests (include/gorio_sc_cross.h), each of scans of <= 400 points.

A, 29 entries (the database tests/test_sc_exhaustive_gpu.py documents, built here again): the 24 keyframes of
sc_scenes.loop_sequence(n_lap=12, seed=11, n_points=400), an empty scan (24, all-zero descriptor: 1e7 against everything), a scan
confined to 3 sectors (25: most column norms 0 on its side), and keyframes 1, 1 and 14 added again (26, 27, 28).

B, 19 entries (2 x GORIO_SC_TILE_COLS + 3): the 14 keyframes of sc_scenes.loop_sequence(n_lap=7, seed=23, n_points=400), A's keyframes
1, 1 and 14 (14, 15, 16: the two copies tie exactly against every query, and A's own copies of them score their self-distance), an
empty scan (17) and the 3-sector scan (18)."""
import functools

import numpy as np

import sc_cross_restatement as cx
import sc_restatement as sr
import sc_scenes as ss

F = np.float32
N_A, N_B = 29, 19
A_EMPTY, A_NARROW, A_DUPS = 24, 25, {26: 1, 27: 1, 28: 14}
B_TIED, B_A14, B_EMPTY, B_NARROW = (14, 15), 16, 17, 18


def narrow_scan():
    """300 points in sectors 6..8 of 20: azimuth = atan2(x, y) - 90 deg, so x = r cos(az), y = -r sin(az)."""
    rng = np.random.default_rng(5)
    unit = 113.0 / 20.0
    az = np.deg2rad(rng.uniform(-56.5 + 5 * unit + 0.2, -56.5 + 8 * unit - 0.2, 300))
    r = rng.uniform(2.0, 78.0, 300)
    xyz = np.stack([r * np.cos(az), -r * np.sin(az), np.zeros(300)], 1).astype(F)
    return xyz, rng.uniform(1.0, 30.0, 300).astype(F)


def empty_scan():
    return np.zeros((0, 3), F), np.zeros(0, F)


@functools.lru_cache(maxsize=None)
def scans():
    """(scans of A, scans of B)."""
    lap_a, _ = ss.loop_sequence(n_lap=12, seed=11, n_points=400)
    lap_b, _ = ss.loop_sequence(n_lap=7, seed=23, n_points=400)
    a = list(lap_a) + [empty_scan(), narrow_scan()] + [lap_a[k] for k in A_DUPS.values()]
    b = list(lap_b) + [lap_a[1], lap_a[1], lap_a[14], empty_scan(), narrow_scan()]
    assert (len(a), len(b)) == (N_A, N_B)
    return a, b


def _descs(scan_list):
    ref = sr.SCManagerRef()
    for x, i in scan_list:
        ref.add_scan(x, i)
    return ref.descs


@functools.lru_cache(maxsize=None)
def world():
    """dict(scans_a, scans_b, descs_a, descs_b, and the reference matrices (dist, shift) axb [29, 19], axa [29, 29], bxa [19, 29]).
    Computed once per process and read-only."""
    a, b = scans()
    da, db = _descs(a), _descs(b)
    out = dict(scans_a=a, scans_b=b, descs_a=da, descs_b=db)
    for name, (q, d) in dict(axb=(da, db), axa=(da, da), bxa=(db, da)).items():
        dist, shift = cx.cross_matrix(q, d)
        dist.setflags(write=False), shift.setflags(write=False)
        out[name] = (dist, shift)
    return out
