"""Scans at the size, geometry and parameter edges of Patchwork++ ground segmentation (go-rio_amd/csrc/apd_ground.hip).

Every builder is deterministic and returns (xyz float32 [n, 3], intensity float32 [n], parameter overrides) or a dict of such triples;
switches() returns sequences.  Radii, ring sizes and sector sizes come from the constructor of the restatement (PWP:254-272) for the
parameters in use, never from literals here.  tests/test_ground_edge_scenes.py pins, on the CPU, that each scene has the property it
is named for; tests/test_ground_edges_gpu.py runs them on the device.
"""
import math

import numpy as np

import ground_scenes as gs
import patchwork_restatement as pr

F = np.float32
LADDER = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
# patch id -> point count (default grid: ids 0-11 zone 0, 12-15 zone 1, 16-17 zone 2, 18-23 zone 3).  8192 keys still sort in LDS;
# 8193, 16385 and 8194 sort in the global scratch, with a skipped patch (9 < num_min_pts) and an LDS patch (256) between the first two.
EXACT_COUNTS = {0: 255, 1: 8193, 2: 9, 4: 256, 6: 16385, 9: 10, 11: 8191, 13: 257, 16: 8192, 21: 8194}
SELECTED_COUNTS = {1: 255, 5: 256, 14: 257}  # patch id -> size of its ground layer (the R-GPF selection)
SELECTED_ELEVATED = 100


def geometry(**overrides):
    """The restatement's object for these parameters: min_ranges, ring_sizes, sector_sizes, zone_patch_off, p."""
    return pr.Patchworkpp(**overrides)


def patch_bounds(geo, pid):
    """(r_lo, r_hi, theta_lo, theta_hi) of patch pid; theta in (0, 2 pi] as xy2theta gives it."""
    R, S = geo.p["num_rings_each_zone"], geo.p["num_sectors_each_zone"]
    zone = max(z for z in range(4) if geo.zone_patch_off[z] <= pid)
    ring, sector = divmod(pid - int(geo.zone_patch_off[zone]), S[zone])
    assert ring < R[zone]
    r_lo = geo.min_ranges[zone] + ring * geo.ring_sizes[zone]
    return r_lo, r_lo + geo.ring_sizes[zone], sector * geo.sector_sizes[zone], (sector + 1) * geo.sector_sizes[zone]


def _inside(rng, geo, pid, m):
    """m (x, y) strictly inside patch pid: 0.05 m and 0.02 rad inside its borders."""
    r_lo, r_hi, t_lo, t_hi = patch_bounds(geo, pid)
    r = rng.uniform(r_lo + 0.05, r_hi - 0.05, m)
    t = rng.uniform(t_lo + 0.02, t_hi - 0.02, m)
    return r * np.cos(t), r * np.sin(t)


def _ground_z(rng, geo, x, y):
    return -geo.p["sensor_height"] + 0.004 * x - 0.003 * y + rng.normal(0, 0.03, len(x))


def _without_patch(xyz, inten, geo, pid):
    keep = geo.labels(xyz, inten) != pid
    return xyz[keep], inten[keep]


# ------------------------------------------------------------------------------------------------ boundaries
def boundary_radii(geo):
    """min_range, min_range + one ring, the zone starts, max_range and the float neighbours above the two ends, ascending."""
    mn, mx = F(geo.p["min_range"]), F(geo.p["max_range"])
    rs = {float(mn), float(F(geo.min_ranges[0] + geo.ring_sizes[0])), float(mx), float(np.nextafter(mx, F(np.inf))), float(np.nextafter(mn, F(np.inf)))}
    rs |= {float(F(v)) for v in geo.min_ranges}
    return sorted(rs)


def boundary_special(sectors):
    """The boundary points alone, in a fixed order: for every radius of boundary_radii (r, +0), (r, -0), (0, r), (-r, +0), (-r, -0),
    (0, -r); then the origin; then (a, a), (-a, a), (-a, -a), (a, -a) for a in 2, 5, 10, 20."""
    geo = geometry(num_sectors_each_zone=list(sectors))
    h = geo.p["sensor_height"]
    pts, inten = [], []
    for r in boundary_radii(geo):
        for x, y in ((r, 0.0), (r, -0.0), (0.0, r), (-r, 0.0), (-r, -0.0), (0.0, -r)):
            pts.append((x, y, -h))
            inten.append(0.5)
    pts.append((0.0, 0.0, -3.0))
    inten.append(geo.p["RNR_intensity_thr"] / 2)
    for a in (2.0, 5.0, 10.0, 20.0):
        for x, y in ((a, a), (-a, a), (-a, -a), (a, -a)):
            pts.append((x, y, -h))
            inten.append(0.5)
    return np.array(pts, F), np.array(inten, F)


def boundary_points(sectors, seed=101):
    """boundary_special(sectors) appended to an ordinary scan."""
    xyz, inten = gs.scan(seed)
    sp, si = boundary_special(sectors)
    return np.concatenate([xyz, sp]), np.concatenate([inten, si]), dict(num_sectors_each_zone=list(sectors))


def rnr_special():
    """Points one float step around each RNR threshold (PWP:661-665), the other two conditions met:
    [0:3] intensity below / at / above float32(RNR_intensity_thr); [3:6] z below / at / above -sensor_height - 0.8;
    [6:10] z two steps and one step on the noise side of the vertical angle threshold, then one and two steps on the other side."""
    geo = geometry()
    p = geo.p
    it = F(p["RNR_intensity_thr"])
    low = F(p["RNR_intensity_thr"] / 2)
    zt = F(-p["sensor_height"] - 0.8)
    deep = F(-p["sensor_height"] - 1.5)
    pts = [(3.0, 0.5, deep, np.nextafter(it, F(-np.inf))), (3.0, 0.5, deep, it), (3.0, 0.5, deep, np.nextafter(it, F(np.inf)))]
    pts += [(2.0, 1.0, np.nextafter(zt, F(-np.inf)), low), (2.0, 1.0, zt, low), (2.0, 1.0, np.nextafter(zt, F(np.inf)), low)]
    x, y = F(8.0), F(0.5)
    rn = float(np.sqrt(x * x + y * y))
    ver = lambda z: math.atan2(float(z), rn) * 180 / math.pi
    z = F(rn * math.tan(p["RNR_ver_angle_thr"] / 180 * math.pi))
    while ver(z) >= p["RNR_ver_angle_thr"]:
        z = np.nextafter(z, F(-np.inf))
    while ver(np.nextafter(z, F(np.inf))) < p["RNR_ver_angle_thr"]:
        z = np.nextafter(z, F(np.inf))
    up = np.nextafter(z, F(np.inf))  # z is the last float with ver < thr, up the first with ver >= thr
    assert float(up) < float(zt)  # the height condition holds on both sides
    pts += [(x, y, np.nextafter(z, F(-np.inf)), low), (x, y, z, low), (x, y, up, low), (x, y, np.nextafter(up, F(np.inf)), low)]
    a = np.array(pts, F)
    return a[:, :3].copy(), a[:, 3].copy()


def rnr_threshold_points(seed=102):
    xyz, inten = gs.scan(seed)
    sp, si = rnr_special()
    return np.concatenate([xyz, sp]), np.concatenate([inten, si]), {}


# ------------------------------------------------------------------------------------------------ sizes
def size_ladder(seed=103):
    """{"n<k>": the first k points of one scan} for k in LADDER, "outside": every point outside (min_range, max_range],
    "noise": every point RNR noise."""
    geo = geometry()
    p = geo.p
    xyz, inten = gs.scan(seed)
    out = {"n%d" % k: (xyz[:k].copy(), inten[:k].copy(), {}) for k in LADDER}
    rng = np.random.default_rng(seed)
    m = 300
    r = np.concatenate([rng.uniform(0.0, p["min_range"] * 0.95, m // 2), rng.uniform(p["max_range"] * 1.01, p["max_range"] * 2, m // 2)])
    t = rng.uniform(-np.pi, np.pi, m)
    o = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-1, 1, m)], 1)
    o[0, :2] = (p["min_range"], 0.0)  # r == min_range exactly is outside
    o[1, :2] = 0.0
    out["outside"] = (o.astype(F), rng.uniform(0.2, 1.0, m).astype(F), {})
    r = rng.uniform(2.0, 4.0, m)
    t = rng.uniform(-np.pi, np.pi, m)
    z = -p["sensor_height"] - rng.uniform(1.2, 1.7, m)  # steeper than -15 degrees, lower than -sensor_height - 0.8
    out["noise"] = (np.stack([r * np.cos(t), r * np.sin(t), z], 1).astype(F), rng.uniform(0.0, p["RNR_intensity_thr"] * 0.9, m).astype(F), {})
    return out


def exact_patch_counts(seed=104, variant="counts"):
    """variant "counts": the patches of EXACT_COUNTS hold exactly those many ground points, every other patch none; input order
    shuffled.  variant "selected": the patches of SELECTED_COUNTS hold a ground layer of exactly that size plus SELECTED_ELEVATED
    points above -sensor_height + 0.5, so every R-GPF selection has exactly the layer's size (255 / 256 / 257, the staging width of
    the moments and its neighbours)."""
    geo = geometry()
    h = geo.p["sensor_height"]
    rng = np.random.default_rng(seed)
    parts = []
    if variant == "counts":
        for pid, m in EXACT_COUNTS.items():
            x, y = _inside(rng, geo, pid, m)
            parts.append(np.stack([x, y, _ground_z(rng, geo, x, y)], 1))
    else:
        assert variant == "selected"
        for pid, m in SELECTED_COUNTS.items():
            x, y = _inside(rng, geo, pid, m)
            parts.append(np.stack([x, y, _ground_z(rng, geo, x, y)], 1))
            x, y = _inside(rng, geo, pid, SELECTED_ELEVATED)
            parts.append(np.stack([x, y, -h + rng.uniform(0.6, 2.0, SELECTED_ELEVATED)], 1))
    xyz = np.concatenate(parts).astype(F)
    xyz = xyz[rng.permutation(len(xyz))]
    return xyz, np.full(len(xyz), 0.5, F), {}


# ------------------------------------------------------------------------------------------------ ties and degenerate fits
TIE_PATCH = 4          # zone 0, ring 1, sector 1 of the default grid
LINE_PATCH = 3         # zone 0, ring 1, sector 0


def z_ties(seed=305):
    """{"a": z rounded to 1/16 m; "b": TIE_PATCH also holds 40 points with z alternating +0.0 / -0.0 in input order; "c": every z is
    float32(-sensor_height) (covariance zz and the smallest singular value are rounding noise); "d": LINE_PATCH holds 16 collinear
    points only (covariance exactly diag(c, 0, 0)), with the elevation thresholds at -1 so that the patch reaches TGR; "e": LINE_PATCH
    holds 12 coincident points only}."""
    geo = geometry()
    rng = np.random.default_rng(seed)
    xyz, inten = gs.scan(seed)
    out = {}
    a = xyz.copy()
    a[:, 2] = np.round(a[:, 2] * 16) / 16
    out["a"] = (a, inten, {})
    x, y = _inside(rng, geo, TIE_PATCH, 40)
    zz = np.where(np.arange(40) % 2 == 0, 0.0, -0.0)
    b = np.concatenate([xyz, np.stack([x, y, zz], 1).astype(F)])
    bi = np.concatenate([inten, np.full(40, 0.5, F)])
    perm = rng.permutation(len(b))
    out["b"] = (b[perm], bi[perm], {})
    c = xyz.copy()
    c[:, 2] = F(-geo.p["sensor_height"])
    out["c"] = (c, inten, {})
    base, binten = gs.scan(seed + 1, extras=False)
    base, binten = _without_patch(base, binten, geo, LINE_PATCH)
    # x = 2.25 + k / 16, y = 2, z = -0.75, 16 points: every product, sum and division of the moments is exact in float, so
    # cov = diag(c, 0, 0) and sv[1] == 0
    line = np.stack([2.25 + np.arange(16) / 16.0, np.full(16, 2.0), np.full(16, -0.75)], 1).astype(F)
    d = np.concatenate([base[:500], line, base[500:]])
    di = np.concatenate([binten[:500], np.full(16, 0.5, F), binten[500:]])
    out["d"] = (d, di, dict(elevation_thr=[-1.0] * 4))
    same = np.tile(np.array([[3.0, 2.0, -geo.p["sensor_height"]]], F), (12, 1))
    e = np.concatenate([base[:500], same, base[500:]])
    out["e"] = (e, np.concatenate([binten[:500], np.full(12, 0.5, F), binten[500:]]), {})
    for k in ("d", "e"):
        assert np.all(geo.labels(out[k][0][500:512], out[k][1][500:512]) == LINE_PATCH)
    return out


ELEVATED_PATCH = 7     # zone 0, ring 2, sector 1


def elevated_only_patch(seed=306):
    """ELEVATED_PATCH holds 60 points, all with z >= -sensor_height + 0.5: seeds, but no R-GPF selection."""
    geo = geometry()
    rng = np.random.default_rng(seed)
    xyz, inten = gs.scan(seed)
    xyz, inten = _without_patch(xyz, inten, geo, ELEVATED_PATCH)
    x, y = _inside(rng, geo, ELEVATED_PATCH, 60)
    zmax = -geo.p["sensor_height"] + 0.5
    e = np.stack([x, y, zmax + rng.uniform(0.001, 1.5, 60)], 1).astype(F)
    e[0, 2] = F(zmax) if float(F(zmax)) >= zmax else np.nextafter(F(zmax), F(np.inf))  # the lowest float that z < zmax (strict, in double) rejects
    assert np.all(e[:, 2].astype(np.float64) >= zmax)
    xyz, inten = np.concatenate([xyz, e]), np.concatenate([inten, np.full(60, 0.5, F)])
    perm = rng.permutation(len(xyz))
    return xyz[perm], inten[perm], {}


UNDER_RUN = 6


def under_ground_run(seed=107):
    """Input indices 0 .. UNDER_RUN - 1 lie outside max_range at z = -5, index UNDER_RUN outside at z = +1; the scan has no RNR noise,
    so these open cloud_nonground in index order (PWP:872-884 then erases 0, 2, 4 and never tests 1, 3, 5)."""
    geo = geometry()
    xyz, inten = gs.scan(seed, extras=False)
    r = geo.p["max_range"] + 5.0 + np.arange(UNDER_RUN + 1)
    t = 0.3 + 0.7 * np.arange(UNDER_RUN + 1)
    run = np.stack([r * np.cos(t), r * np.sin(t), np.r_[np.full(UNDER_RUN, -5.0), 1.0]], 1).astype(F)
    return np.concatenate([run, xyz]), np.concatenate([np.full(UNDER_RUN + 1, 0.5, F), inten]), {}


# ------------------------------------------------------------------------------------------------ grids and switches
def grid_512(seed=108):
    """512 patches (the most the kernels take), every non-empty one fitted, 1 + 8 fits.  1000 ground points plus extras: about a third of
    the patches are empty and another third hold one or two points (the restatement's time goes with the number of fitted patches)."""
    xyz, inten = gs.scan(seed, n_ground=1000)
    return xyz, inten, dict(num_sectors_each_zone=[32] * 4, num_rings_each_zone=[4] * 4, num_min_pts=1, num_iter=8)


def grid_4(seed=209):
    xyz, inten = gs.scan(seed)
    return xyz, inten, dict(num_sectors_each_zone=[1] * 4, num_rings_each_zone=[1] * 4)


SWITCHES = {"rnr_off": dict(enable_RNR=False), "tgr_off": dict(enable_TGR=False), "iter_1": dict(num_iter=1), "lpr_1": dict(num_lpr=1),
            "storage_3": dict(max_elevation_storage=3, max_flatness_storage=3), "storage_0": dict(max_elevation_storage=0, max_flatness_storage=0)}


SWITCH_SEEDS = {"lpr_1": 5}  # the sequence seed of a switch, 3 unless named here (chosen for the margin, tests/test_ground_edge_scenes.py)


def switches():
    """{name: (8 frames of one sequence, overrides)}."""
    seqs = {s: gs.sequence(s, frames=8) for s in {3} | set(SWITCH_SEEDS.values())}
    return {k: (seqs[SWITCH_SEEDS.get(k, 3)], dict(v)) for k, v in SWITCHES.items()}


# ------------------------------------------------------------------------------------------------ the scenes by name
# Scenes whose LM cost is ~0 (the iteration count then depends on the reduction order), or that fit nothing: id = 0 only on the device.
ID0_ONLY = ("ties_c", "ties_d", "ties_e", "ladder_outside", "ladder_noise", "ladder_n1", "ladder_n2")


def single_scenes():
    """{name: (xyz, intensity, overrides)} of every single-scan scene."""
    S = {"boundary_4444": boundary_points([4, 4, 4, 4]), "boundary_3113": boundary_points([3, 1, 1, 3]), "rnr": rnr_threshold_points()}
    S.update(("ladder_" + k, v) for k, v in size_ladder().items())
    S.update(exact_counts=exact_patch_counts(), exact_counts_b=exact_patch_counts(seed=204), exact_selected=exact_patch_counts(variant="selected"))
    S.update(("ties_" + k, v) for k, v in z_ties().items())
    S.update(elevated=elevated_only_patch(), under_run=under_ground_run(), grid_512=grid_512(), grid_4=grid_4())
    return S
