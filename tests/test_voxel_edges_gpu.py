"""The device voxel structures at the size and geometry edges of tests/voxel_scenes.py, against the CPU restatements that
tests/test_voxel_scenes.py pins on the same scenes.

All of them go through one pipeline (keys = cell id << 31 | input index, the tiled key sort, cell_count_kernel per 256-key block,
block_scan_kernel over the block counts 1024 at a time, one lane per cell start), so every regime x size runs on the first three:
  pcl::VoxelGrid     setInputTargetSubmap + getTargetPoints and prep.voxel_downsample against oracle.apd.submap_assemble: np.array_equal
                     on points and labels, equal counts
  FastVGICP map      getVoxelMap() against gicp_restatement.VoxelMap (VoxelMapVec at 262 k points) with the gates of
                     map_checks.check_map; voxel slots of linearize() equal to the restatement's table
  NDT grid           Ndt.voxels() against ndt_restatement.build_voxel_map with the gates of map_checks.check_ndt_map
The 262 k inputs and their references are built once per module.
The two float maps run the sizes on the wave and 256-key block boundaries of the shared preamble (the 1024 / 1025-block scan edge is
the same scan kernel's, exercised above):
  NDTCuda map        ndt_cuda_voxels(1) against ndt_cuda_restatement.build_map with the table comparison of tests/test_ndt_cuda_gpu.py
  FastVGICPCuda map  vgicp_cuda_voxels() against vgicp_cuda_restatement.build_map fed the device's own per-point covariances, with the
                     comparison of tests/test_vgicp_cuda_gpu.py (bit-exact)
"""
import importlib

import numpy as np
import pytest

import gicp_restatement as gr
import ndt_cuda_restatement as ncr
import ndt_restatement as nr
import test_ndt_cuda_gpu as ndtc
import test_vgicp_cuda_gpu as vgc
import vgicp_cuda_restatement as vr
import voxel_scenes as S
from map_checks import check_map, check_ndt_map

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu
UNSUPPORTED = -5  # GORIO_ERR_UNSUPPORTED

REGIME_IDS = ["%s-%d" % c for c in S.regime_cases()]


# ------------------------------------------------------------------------------------------------ pcl::VoxelGrid

def _grid_scene(key):
    """(frames, rel, leaf) of ("regime", name, m) / ("geometry", name) / ("limit", name)"""
    if key[0] == "regime":
        return [(S.regime(key[1], key[2], cell=S.GRID_CELL), S.labels(key[2]))], [S.EYE], S.GRID_CELL
    if key[0] == "geometry":
        return S.geometry(key[1])
    return S.grid_limit(key[1])[:3]


GRID_KEYS = [("regime",) + c for c in S.regime_cases()] + [("geometry", g) for g in sorted(S.GEOMETRY)] + [("limit", g) for g in S.GRID_LIMITS]
GRID_IDS = ["-".join(str(p) for p in k) for k in GRID_KEYS]


@pytest.fixture(scope="module")
def grid_case(oracle_apd):
    cache = {}

    def get(key):
        if key not in cache:
            frames, rel, leaf = _grid_scene(key)
            cache[key] = (frames, rel, leaf) + oracle_apd.submap_assemble(frames, rel, leaf)
        return cache[key]

    return get


def _assemble_equals(g, case):
    frames, rel, leaf, xo, lo = case
    n = g.setInputTargetSubmap(frames, rel, voxel_leaf=leaf)
    assert n == xo.shape[0]
    xg, lg = g.getTargetPoints()
    assert np.array_equal(xg, xo) and np.array_equal(lg, lo)


@pytest.mark.parametrize("key", GRID_KEYS, ids=GRID_IDS)
def test_voxelgrid_submap(gpu, gorio, grid_case, key):
    case = grid_case(key)
    if key[0] == "limit":
        n_in = case[0][0][0].shape[0]
        assert (case[3].shape[0] < n_in) == S.grid_limit(key[1])[3]  # the voxel branch merges the points of the corner cells
    _assemble_equals(gorio.ApdGicp(), case)


@pytest.mark.parametrize("key", GRID_KEYS, ids=GRID_IDS)
def test_voxelgrid_downsample(gpu, gorio, oracle_apd, grid_case, key):
    """the same clouds through prep.voxel_downsample: one frame as it is (non-finite points included), several frames as the cloud
    their poses assemble (the identity leaves every float coordinate unchanged)"""
    frames, rel, leaf, xo, _ = grid_case(key)
    xyz = frames[0][0] if len(frames) == 1 else oracle_apd.submap_assemble(frames, rel, 0.0)[0]
    out = gorio.prep.voxel_downsample(xyz, leaf)
    assert out.shape == xo.shape and np.array_equal(out, xo)


def test_voxelgrid_handle_reuse(gpu, gorio, grid_case):
    """one handle: 262 145 points (1025 count blocks), then 64, then 4097 -- buffers and block counts of the larger call are still there"""
    g = gorio.ApdGicp()
    for m in (262145, 64, 4097):
        _assemble_equals(g, grid_case(("regime", "mixed", m)))


# ------------------------------------------------------------------------------------------------ FastVGICP Gaussian voxel map

VG_KEYS = [c for c in S.regime_cases()] + list(S.VGICP_GEOMETRY) + ["box_2047"]
VG_IDS = REGIME_IDS + ["geometry-" + g for g in S.VGICP_GEOMETRY] + ["limit-box_2047"]
MODES = [gr.ADDITIVE, gr.MULTIPLICATIVE]


@pytest.fixture(scope="module")
def vg_case():
    clouds, maps = {}, {}

    def get(key, mode):
        if key not in clouds:
            xyz = S.vgicp_target(key)
            clouds[key] = (xyz, S.covariances(len(xyz)))
        if (key, mode) not in maps:
            xyz, cov = clouds[key]
            maps[(key, mode)] = (gr.VoxelMap if len(xyz) <= 4097 else gr.VoxelMapVec)(xyz, cov, 1.0, mode)
        return clouds[key] + (maps[(key, mode)],)

    return get


def _vgicp(gorio, xyz, cov, mode, search=gr.DIRECT1):
    g = gorio.ApdGicp()
    g.set_method(apd.METHOD_VGICP, 1.0, search, mode)
    g.setInputTarget(xyz)
    g.setTargetCovariances(cov)
    return g


@pytest.mark.parametrize("mode", MODES, ids=["additive", "multiplicative"])
@pytest.mark.parametrize("key", VG_KEYS, ids=VG_IDS)
def test_vgicp_map(gpu, gorio, vg_case, key, mode):
    xyz, cov, ref = vg_case(key, mode)
    check_map(_vgicp(gorio, xyz, cov, mode).getVoxelMap(), ref)


@pytest.mark.parametrize("key", ["box_2047", ("mixed", 4097), "faces"], ids=["limit-box_2047", "mixed-4097", "geometry-faces"])
def test_vgicp_lookups(gpu, gorio, vg_case, key):
    """a few dozen source points in and just outside the lowest-id voxel, the highest-id voxel and the other corners of the box of
    occupied voxels: the slot table of linearize() for DIRECT1 / 7 / 27 against the restatement's"""
    xyz, cov, ref = vg_case(key, gr.ADDITIVE)
    src = S.vgicp_probe_source(ref.coord)
    src_cov = S.covariances(len(src), seed=1)
    g = _vgicp(gorio, xyz, cov, gr.ADDITIVE)
    g.setInputSource(src)
    g.setSourceCovariances(src_cov)
    check_map(g.getVoxelMap(), ref)
    for search in (gr.DIRECT1, gr.DIRECT7, gr.DIRECT27):
        g.set_method(apd.METHOD_VGICP, 1.0, search, gr.ADDITIVE)
        g.linearize(np.eye(4))
        want = gr.Vgicp(src, xyz, src_cov, cov, 1.0, search, gr.ADDITIVE, voxelmap=ref).slot_table(np.eye(4))
        assert np.array_equal(g.getVoxelCorrespondences(), want)
        assert (want >= 0).any() and (want < 0).any()
        if search == gr.DIRECT1:  # the probes reach the first and the last voxel of the ascending order
            assert 0 in want and len(ref.coord) - 1 in want


@pytest.mark.parametrize("name", ["box_2048", "coord_2pow30"])
def test_vgicp_refusals_leave_the_handle_usable(gpu, gorio, vg_case, name):
    xyz, ok = S.vgicp_limit(name)
    assert not ok
    g = _vgicp(gorio, xyz, S.covariances(len(xyz)), gr.ADDITIVE)
    with pytest.raises(gorio.GorioError) as e:
        g.getVoxelMap()
    assert e.value.code == UNSUPPORTED
    good, cov, ref = vg_case(("mixed", 257), gr.ADDITIVE)
    g.setInputTarget(good)
    g.setTargetCovariances(cov)
    check_map(g.getVoxelMap(), ref)


# ------------------------------------------------------------------------------------------------ NDT covariance grid

@pytest.fixture(scope="module")
def ndt_case():
    cache = {}

    def get(regime, m):
        if (regime, m) not in cache:
            xyz = S.regime(regime, m)
            cache[(regime, m)] = (xyz, nr.build_voxel_map(xyz, 1.0))
        return cache[(regime, m)]

    return get


@pytest.mark.parametrize("regime,m", S.NDT_CASES)
def test_ndt_map(gpu, gorio, ndt_case, regime, m):
    xyz, ref = ndt_case(regime, m)
    check_ndt_map(gorio, gpu, xyz, ref=ref)


def test_ndt_limits(gpu, gorio, ndt_case):
    """div_b = 1290^3 fits int32 and builds (the top corner leaf, id 1290^3 - 1, is enabled); 1291^3 is refused and the handle goes on"""
    xyz, ok = S.ndt_limit("box_1290")
    ref, v = check_ndt_map(gorio, gpu, xyz)
    assert ok and v["leaf_index"][-1] == 1290 ** 3 - 1 and v["nr_points"][-1] >= 6 and v["icov"][-1].any()
    bad, ok = S.ndt_limit("box_1291")
    assert not ok
    n = gorio.Ndt(device=gpu)
    with pytest.raises(gorio.GorioError) as e:
        n.set_target(bad)
        n.voxels()
    assert e.value.code == UNSUPPORTED
    good, ref = ndt_case("mixed", 257)
    n.set_target(good)
    v = n.voxels()
    n.close()
    assert np.array_equal(v["leaf_index"], ref.idx) and np.array_equal(v["mean"], ref.mean)


# ------------------------------------------------------------------------------------------------ the float maps: NDTCuda, FastVGICPCuda

FLOAT_CASES = [(r, m) for r in ("own_cell", "mixed") for m in (1, 63, 64, 65, 255, 256, 257, 4097)] + [("one_cell", 4097)]
FLOAT_IDS = ["%s-%d" % c for c in FLOAT_CASES]


@pytest.mark.parametrize("regime,m", FLOAT_CASES, ids=FLOAT_IDS)
def test_ndt_cuda_map(gpu, gorio, regime, m):
    xyz = S.vgicp_target((regime, m))  # points in the middle half of their voxels: the float and the double rule agree
    g = ndtc.make(gorio, gpu, mode=ncr.P2D)
    g.setInputTarget(xyz)
    ref = ncr.build_map(xyz, 1.0)
    assert ref["num_points"].sum() == m
    ndtc.check_table(g.ndt_cuda_voxels(1), ref)


@pytest.mark.parametrize("regime,m", FLOAT_CASES, ids=FLOAT_IDS)
def test_vgicp_cuda_map(gpu, gorio, regime, m):
    """covariances by the RBF kernel (no k-NN list, so one point is a cloud) and no regularisation: every point is kept, the map is
    built from exactly m keys"""
    xyz = S.vgicp_target((regime, m))
    g = vgc.make(gorio, gpu, nn=vr.GPU_RBF_KERNEL, regularization=vr.NONE)
    g.setInputTarget(xyz)
    pts, tab = g.vgicp_cuda_points(1), g.vgicp_cuda_voxels()
    assert np.array_equal(pts["kept_index"], np.arange(m)) and np.isfinite(pts["cov"]).all()
    ref = vr.build_map(xyz, pts["cov"], 1.0)
    assert np.array_equal(tab["coord"], ref["coord"]) and np.array_equal(tab["num_points"], ref["num_points"])
    assert vgc.same_bits(tab["mean"], ref["mean"]) and vgc.same_bits(tab["cov"], ref["cov6"])
    assert ref["num_points"].sum() == m
