"""CPU tests that pin the scenes of voxel_scenes.py and the CPU restatements of the three voxel structures on them, before any GPU
comparison depends on either (no GPU).

  * pcl::VoxelGrid: an independent NumPy statement (cell index np.floor(x32 * inv32) in float32, then int64 arithmetic; membership by a
    stable sort; centroids in float64) against the C restatement oracle.apd.submap_assemble, on every regime x size, every geometry
    scene and every limit scene -- no case is left out of the comparison.
  * FastVGICP map: gicp_restatement.VoxelMapVec (no loop over the points; used at 262 k points) equal to gicp_restatement.VoxelMap
    with np.array_equal on every scene of at most 4097 points, both accumulation modes.
  * NDT grid: ndt_restatement.build_voxel_map is vectorised over the leaves already and needs no second form; the limit scenes and
    the 262 k regimes are checked for the structure they claim.
  * Every scene: the structural facts it is named for (voxel count, runs that cross wave and block boundaries, blocks without a
    start, points on faces, signed zeros, cancelling labels, bounding boxes at the packed-id limits).
"""
import numpy as np
import pytest

import gicp_restatement as gr
import ndt_restatement as nr
import voxel_scenes as S

f32 = np.float32
GRID_CELL = S.GRID_CELL


# ------------------------------------------------------------------------------------------------ the NumPy statement of pcl::VoxelGrid

def np_transform(frames, rel):
    """finite points of every frame, (float)(((T0 x + T1 y) + T2 z) + T3) in double, concatenated with their labels"""
    xs, ls = [], []
    for (xyz, lab), T in zip(frames, rel):
        x = np.asarray(xyz, f32).reshape(-1, 3)
        keep = np.isfinite(x).all(axis=1)
        p = x[keep].astype(np.float64)
        T = np.asarray(T, np.float64)
        out = np.empty((p.shape[0], 3), f32)
        for r in range(3):
            out[:, r] = (((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3]).astype(f32)
        xs.append(out)
        ls.append(np.asarray(lab, f32)[keep])
    return np.concatenate(xs), np.concatenate(ls)


def np_voxelgrid(frames, rel, leaf):
    """dict(voxel, ids, order, centroid float64 [nv, 3], count, label_sum float64, maxabs [nv, 3], x, l).  voxel False: the input is
    passed through (PCL's overflow test on d, or the product of div_b beyond int32: DESIGN.md section 2)."""
    x, l = np_transform(frames, rel)
    d, div_b, min_b = S.grid_dims(x, leaf)
    cells_d = int(d[0]) * int(d[1]) * int(d[2])
    cells_b = int(div_b[0]) * int(div_b[1]) * int(div_b[2])
    out = dict(x=x, l=l, d=d, div_b=div_b, voxel=cells_d <= S.INT_MAX and cells_b <= S.INT_MAX)
    if not out["voxel"]:
        return out
    inv = f32(1.0) / f32(leaf)
    ijk = np.floor(x * inv).astype(np.int64) - min_b
    ids = ijk[:, 0] + ijk[:, 1] * div_b[0] + ijk[:, 2] * div_b[0] * div_b[1]
    order = np.argsort(ids, kind="stable")
    sid = ids[order]
    first = np.ones(sid.size, bool)
    first[1:] = sid[1:] != sid[:-1]
    starts = np.nonzero(first)[0]
    count = np.diff(np.append(starts, sid.size))
    xd = x.astype(np.float64)[order]
    out.update(ids=ids, sorted_ids=sid, count=count, centroid=np.add.reduceat(xd, starts, axis=0) / count[:, None],
               maxabs=np.maximum.reduceat(np.abs(xd), starts, axis=0), label_sum=np.add.reduceat(l.astype(np.float64)[order], starts))
    return out


def check_oracle_against_numpy(oracle_apd, frames, rel, leaf):
    ref = np_voxelgrid(frames, rel, leaf)
    xo, lo, co = oracle_apd.submap_assemble(frames, rel, leaf, with_counts=True)
    if not ref["voxel"]:
        assert np.array_equal(xo, ref["x"]) and np.array_equal(lo, ref["l"]) and (co == 1).all()
        return ref
    # the same voxel set in the same order: as many voxels, the same count in every position, and (below) every centroid within a
    # bound that is a small fraction of the leaf
    assert xo.shape[0] == ref["count"].shape[0]
    assert np.array_equal(co, ref["count"])
    # Centroid: the restatement adds the cnt float32 coordinates of a voxel one after the other and divides once.  With u = 2^-24
    # the sequential sum is off by at most gamma_(cnt-1) * sum |x_i| <= gamma_(cnt-1) * cnt * max |x_i| (gamma_k = k u / (1 - k u)),
    # the division by cnt (exact as a float below 2^24) leaves gamma_(cnt-1) * max |x_i| of that and adds one rounding of the
    # quotient, u * (1 + gamma_(cnt-1)) * max |x_i|: together at most gamma_cnt * max |x_i| <= 2 cnt u max |x_i| = cnt 2^-23 max |x_i|
    # while cnt u <= 1/2.  The float64 centroid it is compared with is off by cnt 2^-53 max |x_i| at most, which the slack between
    # gamma_cnt and 2 cnt u (a factor 1 - cnt u of the bound) covers for every cnt here.
    bound = ref["count"][:, None] * 2.0 ** -23 * ref["maxabs"]
    err = np.abs(xo.astype(np.float64) - ref["centroid"])
    assert (err <= bound).all(), float((err - bound).max())
    # label: the sign of the summed labels; the labels are small integers, so the float sum is exact and a zero sum stays zero
    assert np.array_equal(lo.astype(np.float64), np.sign(ref["label_sum"]))
    return ref


# ------------------------------------------------------------------------------------------------ regimes

@pytest.mark.parametrize("phase", [0.0, 0.5])
@pytest.mark.parametrize("regime,m", S.regime_cases())
def test_regime_structure(regime, m, phase):
    """what each regime claims, from the cell ids in sorted key order -- for the floor(x / leaf) cells of VoxelGrid / NDT (phase 0) and
    the floor(x / res - 0.5) cells of FastVGICP (phase 0.5)"""
    cell = GRID_CELL if phase == 0.0 else 1.0
    xyz = S.regime(regime, m, cell=cell, phase=phase)
    assert xyz.dtype == f32 and xyz.shape == (m, 3) and xyz.flags["C_CONTIGUOUS"] and np.isfinite(xyz).all()
    assert np.array_equal(xyz, S.regime(regime, m, cell=cell, phase=phase))
    if phase == 0.0:
        c = np.floor(xyz * (f32(1.0) / f32(cell))).astype(np.int64)
    else:
        c = gr.voxel_coord(xyz.astype(np.float64), cell)
    c -= c.min(axis=0)
    dim = c.max(axis=0) + 1
    ids = c[:, 0] + c[:, 1] * dim[0] + c[:, 2] * dim[0] * dim[1]
    nv, cross64, cross256, empty = S.run_structure(np.sort(ids, kind="stable"))
    if regime == "one_cell":
        assert nv == 1 and cross64 == (m > 64) and cross256 == (m > 256) and empty == (m - 1) // 256
    elif regime == "own_cell":
        assert nv == m and cross64 == 0 and empty == 0
    else:
        mult = S.mixed_multiplicities(m)
        assert nv == len(mult) and mult.sum() == m and mult.max() <= S.MIXED_MAX
        if m >= 4095:
            assert list(mult[:3]) == list(S.MIXED_LONG) and cross64 > 0 and cross256 > 0 and empty > 0
        elif m >= 255:
            assert cross64 > 0
        if m >= 262143:
            assert nv > 1024  # more voxels than one pass of the block scan has lanes
    if nv > 1 and m > 2:
        assert (np.diff(ids) < 0).any()  # shuffled: the input is not in key order
    if regime != "own_cell" and m > 2:
        first_cell = np.nonzero(ids == ids[0])[0]
        assert first_cell.size == 1 or not np.array_equal(xyz[first_cell], xyz[first_cell][np.lexsort(xyz[first_cell].T)])


@pytest.mark.parametrize("regime,m", S.regime_cases())
def test_voxelgrid_oracle_equals_numpy_on_regimes(oracle_apd, regime, m):
    xyz = S.regime(regime, m, cell=GRID_CELL)
    ref = check_oracle_against_numpy(oracle_apd, [(xyz, S.labels(m))], [S.EYE], GRID_CELL)
    assert ref["voxel"] and ref["count"].shape[0] == {"one_cell": 1, "own_cell": m}.get(regime, len(S.mixed_multiplicities(m)))


# ------------------------------------------------------------------------------------------------ geometry and limits of the grid

@pytest.mark.parametrize("name", sorted(S.GEOMETRY))
def test_voxelgrid_oracle_equals_numpy_on_geometry(oracle_apd, name):
    frames, rel, leaf = S.geometry(name)
    assert sum(f[0].shape[0] for f in frames) <= 2000
    ref = check_oracle_against_numpy(oracle_apd, frames, rel, leaf)
    assert ref["voxel"]
    x, inv = ref["x"], f32(1.0) / f32(leaf)
    raw = np.concatenate([f[0] for f in frames])
    on_face = (x * inv == np.floor(x * inv)).sum()
    if name == "straddle_zero":
        assert (np.signbit(raw) & (raw == 0)).sum() >= 6 and (~np.signbit(raw) & (raw == 0)).sum() >= 6
        assert (np.abs(raw) < leaf).all() and (raw < 0).any() and (raw > 0).any()
    if name == "faces_half":
        assert on_face == x.size
    if name == "faces_tenth":
        k = np.round(x.astype(np.float64) * 10.0)
        assert on_face > x.size // 2 and (np.floor(x * inv) != k).sum() > 0  # most products land on k exactly, some just below it
    if name == "offset_1e5":
        assert np.unique(x, axis=0).shape[0] < x.shape[0] - 100 and np.all(x * 128 == np.round(x * 128))
    if name == "duplicates":
        assert ref["count"].max() >= 100
    if name == "line":
        assert list(ref["div_b"][1:]) == [1, 1] and ref["div_b"][0] > 100
    if name == "plane":
        assert ref["div_b"][2] == 1 and ref["div_b"][0] > 10 and ref["div_b"][1] > 10
    if name == "labels_cancel":
        assert (ref["label_sum"] == 0).sum() == 40 and (ref["label_sum"] > 0).sum() == 24 and (ref["l"] != 0).all()
    if name == "labels_zero":
        assert not ref["l"].any()
    if name == "nonfinite_first":
        assert not np.isfinite(raw[0]).all() and x.shape[0] == raw.shape[0] - 1
    if name == "nonfinite_last":
        assert not np.isfinite(raw[-1]).all() and x.shape[0] == raw.shape[0] - 1
    if name == "frame_all_nonfinite":
        assert not np.isfinite(frames[1][0]).all(axis=1).any() and x.shape[0] == 300 + 257
    if name == "empty_frame":
        assert frames[1][0].shape == (0, 3) and x.shape[0] == 300 + 257
    if name == "frame_sizes":
        assert [f[0].shape[0] for f in frames] == [1, 255, 256, 257]
    if name not in ("labels_cancel", "labels_zero"):
        assert set(np.unique(ref["l"])) == set(np.arange(10.0))  # cluster ids 0 .. 9


@pytest.mark.parametrize("name", S.GRID_LIMITS)
def test_voxelgrid_oracle_equals_numpy_on_limits(oracle_apd, name):
    frames, rel, leaf, voxel = S.grid_limit(name)
    assert 8 <= frames[0][0].shape[0] <= 32
    ref = check_oracle_against_numpy(oracle_apd, frames, rel, leaf)
    assert ref["voxel"] == voxel
    d, div_b = [int(v) for v in ref["d"]], [int(v) for v in ref["div_b"]]
    if name == "fits":
        assert d == [46340, 46340, 1] and div_b == d and ref["sorted_ids"][-1] == 46340 * 46340 - 1 and ref["count"][-1] == 4  # two corners of the box and two further points
        assert (int(ref["sorted_ids"][-1]) << 31) >> 61  # the top id reaches the key's high bits
    if name == "overflow":
        assert d == [46341, 46341, 1] and d[0] * d[1] > S.INT_MAX
    if name in ("divb_leaf1", "divb_leaf01"):
        # PCL's test passes, the grid the indices use does not fit: the int product div_b.x * div_b.y is -2 147 479 015 in 32 bits
        assert d == [46340, 46340, 1] and div_b == [46341, 46341, 2]
        assert d[0] * d[1] * d[2] <= S.INT_MAX < div_b[0] * div_b[1]
        assert np.int64(div_b[0] * div_b[1]).astype(np.int32) == -2147479015
        x, inv = ref["x"], f32(1.0) / f32(leaf)
        assert ((np.floor(x[:, 2] * inv) - np.floor(x[:, 2].min() * inv)) == 1).sum() >= 4  # points whose id the parent made negative


# ------------------------------------------------------------------------------------------------ FastVGICP map

def _vgicp_small_scenes():
    out = [("regime-%s-%d" % (r, m), (r, m)) for r, m in S.regime_cases() if m <= 4097]
    out += [("geometry-" + g, g) for g in S.VGICP_GEOMETRY] + [("limit-box_2047", "box_2047")]
    return out


@pytest.mark.parametrize("mode", [gr.ADDITIVE, gr.MULTIPLICATIVE])
@pytest.mark.parametrize("key", [k for _, k in _vgicp_small_scenes()], ids=[i for i, _ in _vgicp_small_scenes()])
def test_vectorised_voxelmap_equals_the_loop(key, mode):
    xyz = S.vgicp_target(key)
    cov = S.covariances(len(xyz))
    a, b = gr.VoxelMap(xyz, cov, 1.0, mode), gr.VoxelMapVec(xyz, cov, 1.0, mode)
    assert np.array_equal(a.coord, b.coord) and np.array_equal(a.num_points, b.num_points)
    assert np.array_equal(a.mean, b.mean) and np.array_equal(a.cov, b.cov)
    probe = S.vgicp_probe_source(a.coord)
    c = gr.voxel_coord(probe.astype(np.float64), 1.0)
    assert np.array_equal(a.lookup(c), b.lookup(c))
    if isinstance(key, tuple):
        assert a.coord.shape[0] == {"one_cell": 1, "own_cell": key[1]}.get(key[0], len(S.mixed_multiplicities(key[1])))


@pytest.mark.parametrize("regime,m", [(r, m) for r, m in S.regime_cases() if m > 4097])
def test_vectorised_voxelmap_at_the_large_sizes(regime, m):
    xyz = S.regime(regime, m, cell=1.0, phase=0.5)
    vm = gr.VoxelMapVec(xyz, S.covariances(m), 1.0, gr.MULTIPLICATIVE)
    assert vm.num_points.sum() == m and vm.coord.shape[0] == (m if regime == "own_cell" else len(S.mixed_multiplicities(m)))
    assert np.isfinite(vm.mean).all() and np.isfinite(vm.cov).all()


def test_vgicp_geometry_and_limit_scenes():
    faces = S.vgicp_geometry("faces")
    assert np.array_equal(faces - 0.5, np.round(faces - 0.5)) and faces.shape[0] <= 2000  # every coordinate is (k + 0.5) res
    z = S.vgicp_geometry("straddle_zero")
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    xyz, ok = S.vgicp_limit("box_2047")
    c = gr.voxel_coord(xyz.astype(np.float64), 1.0)
    dim = c.max(axis=0) - c.min(axis=0) + 1
    assert ok and 8 <= len(xyz) <= 32 and list(dim) == [2048, 2048, 2047] and np.abs(xyz).max() <= 2048
    r = c - c.min(axis=0)
    top = int(((r[:, 0] * dim[1] + r[:, 1]) * dim[2] + r[:, 2]).max())
    assert top == 2 ** 33 - 2 ** 22 - 1 and ((top << 31) >> 63) == 1 and (top << 31) < 2 ** 64  # the largest id is in the map, bit 63 of its key set
    assert (c == c.max(axis=0)).all(axis=1).sum() >= 2 and (c == c.min(axis=0)).all(axis=1).sum() >= 2
    xyz, ok = S.vgicp_limit("box_2048")
    c = gr.voxel_coord(xyz.astype(np.float64), 1.0)
    assert not ok and 8 <= len(xyz) <= 32 and list(c.max(axis=0) - c.min(axis=0) + 1) == [2048] * 3 and np.abs(xyz).max() <= 2048
    xyz, ok = S.vgicp_limit("coord_2pow30")
    assert not ok and 8 <= len(xyz) <= 32 and gr.voxel_coord(xyz.astype(np.float64), 1.0).max() >= 2 ** 30
    box = np.array([[-1024, -1024, -1024], [1023, 1023, 1022]])
    probe = S.vgicp_probe_source(box)
    assert 24 <= len(probe) <= 60
    pc = gr.voxel_coord(probe.astype(np.float64), 1.0)
    inside = ((pc >= box[0]) & (pc <= box[1])).all(axis=1)
    assert inside.sum() >= 16 and (~inside).sum() >= 16  # probes on both sides of every corner of the box
    assert (pc == box[0]).all(axis=1).any() and (pc == box[1]).all(axis=1).any()


# ------------------------------------------------------------------------------------------------ NDT grid

@pytest.mark.parametrize("regime,m", S.NDT_CASES)
def test_ndt_restatement_on_regimes(regime, m):
    vm = nr.build_voxel_map(S.regime(regime, m), 1.0)
    assert vm.n_leaves == {"one_cell": 1, "own_cell": m}.get(regime, len(S.mixed_multiplicities(m)))
    assert np.abs(vm.count).sum() == m and np.all(np.diff(vm.idx) > 0)
    if regime == "own_cell":
        assert (vm.count == 1).all() and not vm.icov.any()
    else:
        assert (vm.count >= 6).any()


def test_ndt_limit_scenes():
    xyz, ok = S.ndt_limit("box_1290")
    vm = nr.build_voxel_map(xyz, 1.0)
    assert ok and 8 <= len(xyz) <= 32 and list(vm.div_b) == [1290] * 3 and 1290 ** 3 <= S.INT_MAX
    assert vm.idx[-1] == 1290 ** 3 - 1 and vm.count[-1] >= 6 and vm.idx[0] == 0 and vm.count[0] >= 6  # the top corner leaf is enabled
    xyz, ok = S.ndt_limit("box_1291")
    assert not ok and 8 <= len(xyz) <= 32 and 1291 ** 3 > S.INT_MAX
    assert list(np.floor(xyz.max(axis=0)) - np.floor(xyz.min(axis=0)) + 1) == [1291] * 3
    with pytest.raises(nr.Unsupported):
        nr.build_voxel_map(xyz, 1.0)
