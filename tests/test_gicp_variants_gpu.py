"""GPU parity tests of the FastGICP and FastVGICP methods of the registration ABI (gorio_apd_set_method) against the NumPy
restatement tests/gicp_restatement.py, on identical inputs and identical (oracle) covariances.

Gates (README): indices and voxel slots bit-exact; H, b, error relative 1e-9; voxel means / covariances 1e-12 (the same
double sums in the same order, only the final division differs); poses within 1e-4 m / 1e-4 rad; iteration and linearisation counts equal.
"""
import importlib

import numpy as np
import pytest

import gicp_restatement as gr
import gicp_scenes as gs
from map_checks import MAP_RTOL, check_map, rel  # noqa: F401 -- shared with tests/test_voxel_edges_gpu.py

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu

H_RTOL = 1e-9
SHIPPED = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1)  # launch/ntu_loop3.launch:85-96


@pytest.fixture(scope="module")
def covs(oracle_apd):
    cache = {}

    def get(name, xyz):
        if name not in cache:
            cache[name] = oracle_apd.calculate_covariances(xyz, oracle_apd.launch_params())
        return cache[name]

    return get


@pytest.fixture(scope="module")
def c1(covs):
    sx, sl, tx, tl, T = gs.c1_pair()
    return sx, sl, tx, tl, T, covs("c1s", sx), covs("c1t", tx)


@pytest.fixture(scope="module")
def c16k(covs):
    sx, sl, tx, tl, T = gs.c1_pair(16384, 16384)
    return sx, sl, tx, tl, T, covs("16s", sx), covs("16t", tx)


@pytest.fixture(scope="module")
def nn_oracle(oracle_apd):
    """exact float 1-NN of the transformed source through the oracle's kd-tree search (pinned to the exhaustive one by
    tests/test_oracle_apd.py::test_kdtree_search_equals_exhaustive): the stand-in for GICP:142-144 on 16 k clouds"""
    p = oracle_apd.default_params(corr_dist_threshold=1e18, search=1)

    def f(T, src, tgt):
        eye_s = np.broadcast_to(np.eye(4), (src.shape[0], 4, 4)).copy()
        eye_t = np.broadcast_to(np.eye(4), (tgt.shape[0], 4, 4)).copy()
        c, d, _ = oracle_apd.update_correspondences(T, src, tgt, eye_s, eye_t, p)
        return c, d

    return f


def make(gorio, scene, method, res=1.0, search=gr.DIRECT1, mode=gr.ADDITIVE, **params):
    sx, sl, tx, tl, _, cs, ct = scene
    g = gorio.ApdGicp(**params)
    g.set_method(method, res, search, mode)
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    g.setSourceCovariances(cs)
    g.setTargetCovariances(ct)
    return g


def check_align(r, ro, pose_err):
    dt, dr = pose_err(ro["T"], r["T"])
    print("align: dt %.3e dr %.3e, n_linearize %d / %d, nr_iterations %d / %d" % (dt, dr, r["n_linearize"], ro["n_linearize"], r["nr_iterations"], ro["nr_iterations"]))
    assert dt < 1e-4 and dr < 1e-4
    assert r["converged"] == ro["converged"]
    assert r["nr_iterations"] == ro["nr_iterations"]
    assert r["n_linearize"] == ro["n_linearize"]


OPT = {"LM": dict(optimizer=1, **SHIPPED), "GN": dict(optimizer=0, **SHIPPED)}
OPT_R = {"LM": dict(optimizer="LM", transformation_epsilon=0.1), "GN": dict(optimizer="GN", transformation_epsilon=0.1)}


# ------------------------------------------------------------------------------------------------ FastGICP

@pytest.mark.parametrize("scene_name", ["c1", "c16k"])
def test_gicp_linearize(gpu, gorio, request, nn_oracle, scene_name):
    scene = request.getfixturevalue(scene_name)
    sx, sl, tx, tl, Tgt, cs, ct = scene
    g = make(gorio, scene, apd.METHOD_GICP, **SHIPPED)
    ref = gr.Gicp(sx, tx, cs, ct, corr_dist_threshold=2.0, nn=nn_oracle)
    for T in (np.eye(4), Tgt):
        err, H, b = g.linearize(T)
        err_o, H_o, b_o = ref.linearize(T)
        corr, sqd = g.getCorrespondences()
        assert np.array_equal(corr, ref.corr) and np.array_equal(sqd, ref.sqd)
        print("GICP linearize %s: H %.2e b %.2e err %.2e" % (scene_name, rel(H, H_o), rel(b, b_o), abs(err - err_o) / err_o))
        assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * err_o
        assert rel(g.getMahalanobis(), ref.maha) < H_RTOL
        Tx = gs.parity_pose()
        assert g.compute_error(Tx) == pytest.approx(ref.compute_error(Tx), rel=H_RTOL)


@pytest.mark.parametrize("opt", ["LM", "GN"])
def test_gicp_align(gpu, gorio, c1, nn_oracle, pose_err, opt):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    g = make(gorio, c1, apd.METHOD_GICP, **OPT[opt])
    r = g.align()
    ro = gr.align(gr.Gicp(sx, tx, cs, ct, corr_dist_threshold=2.0, nn=nn_oracle), **OPT_R[opt])
    check_align(r, ro, pose_err)


def test_gicp_batch_equals_singles_and_mixed_batch_refused(gpu, gorio, covs):
    scenes = []
    for q in range(8):
        sx, sl, tx, tl, T = gs.synth.scan_pair(3000 + 100 * q, 3100, seed=400 + q)
        scenes.append((sx, sl, tx, tl, T, covs("bs%d" % q, sx), covs("bt%d" % q, tx)))
    singles = [make(gorio, s, apd.METHOD_GICP, **SHIPPED).align() for s in scenes]
    objs = [make(gorio, s, apd.METHOD_GICP, **SHIPPED) for s in scenes]
    batch = gorio.align_batch(objs)
    for a, b in zip(singles, batch):
        assert np.array_equal(a["T"], b["T"]) and np.array_equal(a["H"], b["H"])
        assert (a["converged"], a["nr_iterations"], a["n_linearize"]) == (b["converged"], b["nr_iterations"], b["n_linearize"])
    objs[3].set_method(apd.METHOD_APDGICP)
    with pytest.raises(gorio.GorioError) as e:
        gorio.align_batch(objs)
    assert e.value.code == -1  # GORIO_ERR_INVALID
    objs[3].set_method(apd.METHOD_VGICP)
    with pytest.raises(gorio.GorioError) as e:
        gorio.align_batch(objs)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ FastVGICP

VG_CONFIGS = [(gr.DIRECT1, gr.ADDITIVE, 1.0), (gr.DIRECT7, gr.ADDITIVE, 1.0), (gr.DIRECT27, gr.ADDITIVE, 1.0), (gr.DIRECT1, gr.ADDITIVE, 0.5),
              (gr.DIRECT7, gr.ADDITIVE, 0.5), (gr.DIRECT27, gr.ADDITIVE, 0.5), (gr.DIRECT7, gr.MULTIPLICATIVE, 1.0), (gr.DIRECT7, gr.MULTIPLICATIVE, 0.5)]


@pytest.mark.parametrize("search,mode,res", VG_CONFIGS)
def test_vgicp_map_slots_linearize(gpu, gorio, c1, search, mode, res):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    g = make(gorio, c1, apd.METHOD_VGICP, res, search, mode, **SHIPPED)
    ref = gr.Vgicp(sx, tx, cs, ct, res, search, mode)
    check_map(g.getVoxelMap(), ref.map)
    Tface = gs.near_face_pose(sx, res)
    assert (gs.face_distance(Tface, sx, res) < 1e-6).any()  # some transformed coordinates sit within a micrometre of a voxel face
    for T in (np.eye(4), Tface, Tgt):
        err, H, b = g.linearize(T)
        err_o, H_o, b_o = ref.linearize(T)
        assert np.array_equal(g.getVoxelCorrespondences(), ref.slots)
        print("VGICP linearize: pairs %d, H %.2e b %.2e err %.2e" % ((ref.slots >= 0).sum(), rel(H, H_o), rel(b, b_o), abs(err - err_o) / err_o))
        assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * err_o
        Tx = gs.parity_pose()
        assert g.compute_error(Tx) == pytest.approx(ref.compute_error(Tx), rel=H_RTOL)


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("search,mode,res", VG_CONFIGS)
def test_vgicp_align(gpu, gorio, c1, pose_err, search, mode, res, opt):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    g = make(gorio, c1, apd.METHOD_VGICP, res, search, mode, **OPT[opt])
    r = g.align()
    ro = gr.align(gr.Vgicp(sx, tx, cs, ct, res, search, mode), **OPT_R[opt])
    check_align(r, ro, pose_err)


def test_vgicp_c3_shape_first_linearisation(gpu, gorio, covs):
    sx, sl, tx, tl, T = gs.c3_pair()
    scene = (sx, sl, tx, tl, T, covs("c3s", sx), covs("c3t", tx))
    g = make(gorio, scene, apd.METHOD_VGICP, 1.0, gr.DIRECT7, gr.ADDITIVE, **SHIPPED)
    ref = gr.Vgicp(sx, tx, scene[5], scene[6], 1.0, gr.DIRECT7, gr.ADDITIVE)
    check_map(g.getVoxelMap(), ref.map)
    err, H, b = g.linearize(np.eye(4))
    err_o, H_o, b_o = ref.linearize(np.eye(4))
    assert np.array_equal(g.getVoxelCorrespondences(), ref.slots)
    assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * err_o
    r = g.align()
    assert r["n_linearize"] >= 1


# ------------------------------------------------------------------------------------------------ reuse of the voxel map

def _same(a, b):
    return np.array_equal(a["T"], b["T"]) and np.array_equal(a["H"], b["H"]) and (a["converged"], a["nr_iterations"], a["n_linearize"]) == (b["converged"], b["nr_iterations"], b["n_linearize"])


def test_vgicp_map_reuse_equals_rebuild(gpu, gorio, c1):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    g = make(gorio, c1, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **SHIPPED)
    first, second = g.align(), g.align()  # the second align reuses the map
    fresh = make(gorio, c1, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **SHIPPED).align()
    assert _same(first, second) and _same(first, fresh)
    # a rebuilt target in between: same cloud set again (setInputTarget invalidates covariances and map)
    g.setInputTarget(tx, tl)
    g.setTargetCovariances(ct)
    assert _same(g.align(), fresh)
    # changed resolution / mode / target give what a fresh handle gives
    g.set_method(apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.ADDITIVE)
    assert _same(g.align(), make(gorio, c1, apd.METHOD_VGICP, 0.5, gr.DIRECT7, **SHIPPED).align())
    g.set_method(apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.MULTIPLICATIVE)
    assert _same(g.align(), make(gorio, c1, apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.MULTIPLICATIVE, **SHIPPED).align())
    other = (sx, sl, tx[:4000], tl[:4000], Tgt, cs, ct[:4000])
    g.setInputTarget(tx[:4000], tl[:4000])
    g.setTargetCovariances(ct[:4000])
    assert _same(g.align(), make(gorio, other, apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.MULTIPLICATIVE, **SHIPPED).align())


def test_vgicp_shared_target_equals_private_copies(gpu, gorio, c1, covs):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    sx2, sl2 = gs.shared_source()
    scene2 = (sx2, sl2, tx, tl, Tgt, covs("sh2", sx2), ct)
    private = [make(gorio, c1, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **SHIPPED).align(), make(gorio, scene2, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **SHIPPED).align()]
    owner = make(gorio, c1, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **SHIPPED)
    sharer = gorio.ApdGicp(**SHIPPED)
    sharer.set_method(apd.METHOD_VGICP, 1.0, gr.DIRECT7, gr.ADDITIVE)
    sharer.setInputTargetShared(owner)
    sharer.setInputSource(sx2, sl2)
    sharer.setSourceCovariances(scene2[5])
    shared = gorio.align_batch([owner, sharer])
    assert _same(shared[0], private[0]) and _same(shared[1], private[1])
    # a sharer with other voxel settings must not get the owner's map
    sharer.set_method(apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.ADDITIVE)
    with pytest.raises(gorio.GorioError) as e:
        sharer.align()
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ what has no meaning in VGICP mode

def test_vgicp_refuses_per_point_getters_and_sharding(gpu, gorio, c1):
    g = make(gorio, c1, apd.METHOD_VGICP, 1.0, gr.DIRECT1, **SHIPPED)
    g.linearize(np.eye(4))
    for call in (g.getCorrespondences, g.getMahalanobis):
        with pytest.raises(gorio.GorioError) as e:
            call()
        assert e.value.code == -3  # GORIO_ERR_STATE
    g.debugSetShard(2, 0)
    with pytest.raises(gorio.GorioError) as e:
        g.linearize(np.eye(4))
    assert e.value.code == -3
    g.debugSetShard(1, 0)
    score, inl = g.getFitnessScore(np.eye(4, dtype=np.float32))  # depends on clouds and pose only
    a = make(gorio, c1, apd.METHOD_APDGICP, **SHIPPED)
    assert (score, inl) == a.getFitnessScore(np.eye(4, dtype=np.float32))
    assert g.transformSource(np.eye(4, dtype=np.float32)).shape == (5000, 3)


# ------------------------------------------------------------------------------------------------ APD-GICP untouched

def test_apd_bit_equal_after_switching_method_and_back(gpu, gorio, c1):
    never = make(gorio, c1, apd.METHOD_APDGICP, **SHIPPED)
    g = make(gorio, c1, apd.METHOD_APDGICP, **SHIPPED)
    g.set_method(apd.METHOD_GICP)
    g.linearize(np.eye(4))
    g.align()
    g.set_method(apd.METHOD_VGICP, 1.0, gr.DIRECT7)
    g.align()
    g.set_method(apd.METHOD_APDGICP)
    e0, H0, b0 = never.linearize(gs.parity_pose())
    e1, H1, b1 = g.linearize(gs.parity_pose())
    assert e0 == e1 and np.array_equal(H0, H1) and np.array_equal(b0, b1)
    assert _same(never.align(), g.align())


# ------------------------------------------------------------------------------------------------ known-transform recovery on the device

@pytest.mark.parametrize("method", ["gicp", "vgicp1", "vgicp7"])
def test_known_transform_recovery_on_gpu(gpu, gorio, pose_err, method):
    """The acceptance shape of the reference's gicp_test.cpp:148-149 (translation < 0.05 m, rotation < 1 deg) on the scene that
    tests/test_gicp_restatement.py::test_known_transform_recovery found to meet it on the CPU (gicp_scenes.moved_copy_pair), with the
    classes' default tolerances, an identity guess and the library's own covariances."""
    sx, sl, tx, tl, Tgt = gs.moved_copy_pair()
    g = gorio.ApdGicp()
    g.set_method(apd.METHOD_GICP if method == "gicp" else apd.METHOD_VGICP, 1.0, gr.DIRECT1 if method != "vgicp7" else gr.DIRECT7, gr.ADDITIVE)
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    r = g.align()
    dt, dr = pose_err(Tgt, r["T"])
    print("recovery %s: %.4f m, %.4f deg, %d linearisations" % (method, dt, np.rad2deg(dr), r["n_linearize"]))
    assert r["converged"] and dt < 0.05 and np.rad2deg(dr) < 1.0


# ------------------------------------------------------------------------------------------------ batches of FastVGICP handles

@pytest.mark.parametrize("opt", ["LM", "GN"])
def test_vgicp_batch_of_16_private_targets_equals_singles(gpu, gorio, covs, opt):
    """16 handles (the XCD renumbering of the launch grid applies from 16 pairs on) with private targets and differing sizes"""
    scenes = [(sx, sl, tx, tl, T, covs("vb%ds" % q, sx), covs("vb%dt" % q, tx)) for q, (sx, sl, tx, tl, T) in enumerate(gs.batch_pairs(16))]
    singles = [make(gorio, s, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **OPT[opt]).align() for s in scenes]
    objs = [make(gorio, s, apd.METHOD_VGICP, 1.0, gr.DIRECT7, **OPT[opt]) for s in scenes]
    for a, b in zip(singles, gorio.align_batch(objs)):
        assert _same(a, b)
    objs[5].set_method(apd.METHOD_VGICP, 0.5, gr.DIRECT7, gr.ADDITIVE)  # differing voxel settings inside one batch
    with pytest.raises(gorio.GorioError) as e:
        gorio.align_batch(objs)
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ the bit-defined transform

def test_vgicp_slot_of_a_point_whose_fused_transform_crosses_a_face(gpu, gorio, c1):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    T, res, i, ax = gs.straddling_case(sx)
    ref = gr.Vgicp(sx, tx, cs, ct, res, gr.DIRECT27)
    slots = ref.slot_table(T)
    q = gr.transform_points(T, sx[i:i + 1])
    fused = q.copy()
    fused[0, ax] = gs._fused_row(T[ax], sx[i].astype(np.float64))
    assert gr.voxel_coord(q, res)[0, ax] != gr.voxel_coord(fused, res)[0, ax]  # the property the scene is built for
    g = make(gorio, c1, apd.METHOD_VGICP, res, gr.DIRECT27, gr.ADDITIVE, **SHIPPED)
    g.linearize(T)
    got = g.getVoxelCorrespondences()
    assert np.array_equal(got, slots)
    # and the row of that point is not the one a contracted transform would give (so the comparison above can tell the two apart)
    shifted = gr.Vgicp(sx[i:i + 1], tx, cs[i:i + 1], ct, res, gr.DIRECT27, voxelmap=ref.map)
    alt = np.stack([ref.map.lookup(gr.voxel_coord(fused, res) + off[None, :]) for off in shifted.offsets], axis=1)
    assert not np.array_equal(alt[0], slots[i])


# ------------------------------------------------------------------------------------------------ FastGICP with a sharded source

def test_gicp_shard_partials_add_up(gpu, gorio, c1):
    whole = make(gorio, c1, apd.METHOD_GICP, **SHIPPED)
    T = gs.parity_pose()
    e, H, b = whole.linearize(T)
    ee = whole.compute_error(gs.c1_pair()[4])
    parts = []
    for rank in range(2):
        g = make(gorio, c1, apd.METHOD_GICP, **SHIPPED)
        g.debugSetShard(2, rank)
        parts.append(g.linearize(T) + (g.compute_error(gs.c1_pair()[4]),))
    assert rel(parts[0][1] + parts[1][1], H) < H_RTOL and rel(parts[0][2] + parts[1][2], b) < H_RTOL
    assert parts[0][0] + parts[1][0] == pytest.approx(e, rel=H_RTOL) and parts[0][3] + parts[1][3] == pytest.approx(ee, rel=H_RTOL)


# ------------------------------------------------------------------------------------------------ the map needs a target only

def test_voxelmap_getter_needs_only_a_target(gpu, gorio, c1):
    sx, sl, tx, tl, Tgt, cs, ct = c1
    g = gorio.ApdGicp(**SHIPPED)
    g.set_method(apd.METHOD_VGICP, 1.0, gr.DIRECT1, gr.ADDITIVE)
    g.setInputTarget(tx, tl)
    g.setTargetCovariances(ct)
    check_map(g.getVoxelMap(), gr.VoxelMap(tx, ct, 1.0))
