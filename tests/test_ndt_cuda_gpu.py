"""GPU parity tests of GORIO_METHOD_NDT_CUDA (fast_gicp::NDTCuda, P2D and D2D) against the NumPy restatement tests/ndt_cuda_restatement.py.

Gates: voxel coordinates, counts, means and raw covariances bit-exact; regularised covariances within one float ulp of the matrix's largest
entry (both sides round a double result that agrees far below half an ulp); pair lists bit-exact; H, b, error relative 1e-9 against the
restatement's pair arithmetic fed with the GPU's own voxel tables; poses within 1e-4 m / 1e-4 rad with equal iteration counts.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import ndt_cuda_restatement as nr
from map_checks import rel

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu

F = np.float32
H_RTOL = 1e-9  # the project's gate, as tests/test_gicp_variants_gpu.py applies it
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SEARCH = {nr.DIRECT1: apd.VOXEL_DIRECT1, nr.DIRECT7: apd.VOXEL_DIRECT7, nr.DIRECT27: apd.VOXEL_DIRECT27, nr.DIRECT_RADIUS: apd.VOXEL_DIRECT_RADIUS}


def make(gorio, gpu, mode=nr.D2D, search=nr.DIRECT7, resolution=1.0, radius=-1.0, **params):
    g = gorio.ApdGicp(device=gpu, **params)
    g.set_ndt_cuda_params(mode, radius)
    g.set_method(apd.METHOD_NDT_CUDA, resolution, SEARCH[search])
    return g


def ref_of(g, src, tgt, mode, search=nr.DIRECT7, resolution=1.0, radius=-1.0, gpu_tables=True):
    """the restatement object; with gpu_tables its maps are the GPU's own (parity hook), so only the pair arithmetic is compared"""
    r = nr.NdtCuda(distance_mode=mode, search=search, resolution=resolution, radius=radius)
    r.setInputSource(src)
    r.setInputTarget(tgt)
    if gpu_tables:
        r.target_map = nr.map_from_tables(g.ndt_cuda_voxels(1), resolution)
        if mode == nr.D2D:
            r.source_map = nr.map_from_tables(g.ndt_cuda_voxels(0), resolution)
    return r


def check_table(tab, ref):
    assert np.array_equal(tab["coord"], ref["coord"])
    assert np.array_equal(tab["num_points"], ref["num_points"])
    assert np.array_equal(tab["mean"].view(np.uint32), ref["mean"].view(np.uint32))
    assert np.array_equal(tab["cov_raw"].view(np.uint32), ref["cov_raw"].view(np.uint32))
    ulp = np.spacing(np.abs(ref["cov"]).max(axis=(1, 2)))
    d = np.abs(tab["cov"].astype(np.float64) - ref["cov"].astype(np.float64)).max(axis=(1, 2))
    print("voxels %d, cov: worst difference %.3g ulp of the largest entry" % (len(ulp), (d / ulp).max()))
    assert np.all(d <= ulp)


def edge_cloud():
    """voxels of 1, 6, 7 and 300 points, points exactly on voxel faces, in a shuffled order"""
    rng = np.random.default_rng(11)
    parts = [rng.uniform(0.6, 1.4, (300, 3)), np.array([[4.0, 1.0, 1.0]]), rng.uniform(0.6, 1.4, (6, 3)) + [0, 3, 0], rng.uniform(0.6, 1.4, (7, 3)) + [0, 0, 3]]
    faces = np.array([[0.5, 5.2, 5.1], [1.5, 5.2, 5.1], [-0.5, 5.2, 5.1], [2.5, 5.5, 5.1], [5.2, 0.5, 1.5], [5.2, -1.5, -0.5], [-2.5, -2.5, -2.5]])
    pts = np.concatenate(parts + [faces]).astype(F)
    return pts[rng.permutation(len(pts))]


VOXEL_CASES = {
    "one_point": (lambda: np.array([[0.3, -2.7, 9.1]], F), 1.0),
    "one_voxel": (lambda: np.random.default_rng(5).uniform(2.6, 3.4, (50, 3)).astype(F), 1.0),
    "edges": (edge_cloud, 1.0),
    "float_rule": (lambda: np.concatenate([np.full((1, 3), nr.FLOAT_RULE_POINT), np.random.default_rng(6).uniform(-3, 3, (700, 3))]).astype(F), nr.FLOAT_RULE_RESOLUTION),
    "scene": (lambda: nr.structured_scene(4096), 1.0),
}


@pytest.mark.parametrize("case", sorted(VOXEL_CASES))
def test_voxel_table(gorio, gpu, case):
    fn, res = VOXEL_CASES[case]
    pts = fn()
    g = make(gorio, gpu, resolution=res)
    g.setInputTarget(pts)
    g.setInputSource(pts[::-1].copy())
    ref = nr.build_map(pts, res)
    check_table(g.ndt_cuda_voxels(1), ref)
    check_table(g.ndt_cuda_voxels(0), nr.build_map(pts[::-1], res))  # D2D: the source has a map too, summed in ITS input order
    if case == "edges":
        assert {1, 6, 7, 300} <= set(ref["num_points"].tolist())
    if case == "float_rule":
        c = nr.voxel_coord(pts[:1], res)[0]
        assert c.tolist() == [6, 6, 6] and nr.voxel_coord_double(pts[:1], res)[0].tolist() == [7, 7, 7]
        assert np.any(np.all(g.ndt_cuda_voxels(1)["coord"] == c, axis=1))


POSE = nr.known_transform(0.2, -0.1, 0.05, 0.02, -0.01)


@pytest.mark.parametrize("search,radius", [(nr.DIRECT1, -1.0), (nr.DIRECT7, -1.0), (nr.DIRECT27, -1.0), (nr.DIRECT_RADIUS, 1.5)])
def test_pair_list_per_offset_mode(gorio, gpu, search, radius):
    src, tgt, _ = nr.scene_pair(2048)
    for mode in (nr.P2D, nr.D2D):
        g = make(gorio, gpu, mode, search, 1.0, radius)
        g.setInputSource(src)
        g.setInputTarget(tgt)
        g.linearize(POSE)
        r = ref_of(g, src, tgt, mode, search, 1.0, radius)
        r.linearize(POSE)
        got = g.ndt_cuda_pairs()
        assert len(r.pairs) > 0 and np.array_equal(got, r.pairs)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_pair_list_p2d_sizes(gorio, gpu, n):
    src, tgt, _ = nr.scene_pair(2048)
    g = make(gorio, gpu, nr.P2D, nr.DIRECT7)
    g.setInputSource(src[:n])
    g.setInputTarget(tgt)
    err, H, b = g.linearize(POSE)
    r = ref_of(g, src[:n], tgt, nr.P2D)
    err_o, H_o, b_o = r.linearize(POSE)
    assert np.array_equal(g.ndt_cuda_pairs(), r.pairs)
    assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * abs(err_o)


def test_pair_list_d2d_one_source_voxel(gorio, gpu):
    _, tgt, _ = nr.scene_pair(2048)
    src = (np.random.default_rng(9).uniform(-0.3, 0.3, (40, 3)) + [1.0, 1.0, 0.0]).astype(F)
    g = make(gorio, gpu, nr.D2D, nr.DIRECT27)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    err, H, b = g.linearize(np.eye(4))
    assert len(g.ndt_cuda_voxels(0)["num_points"]) == 1
    r = ref_of(g, src, tgt, nr.D2D, nr.DIRECT27)
    err_o, H_o, b_o = r.linearize(np.eye(4))
    assert len(r.pairs) > 0 and np.array_equal(g.ndt_cuda_pairs(), r.pairs)
    assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * abs(err_o)


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_linearize_and_compute_error(gorio, gpu, mode):
    src, tgt, _ = nr.scene_pair(4096)
    g = make(gorio, gpu, mode)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    err, H, b = g.linearize(POSE)
    r = ref_of(g, src, tgt, mode)
    err_o, H_o, b_o = r.linearize(POSE)
    assert np.array_equal(g.ndt_cuda_pairs(), r.pairs)
    print("NDTCuda mode %d linearize: pairs %d, H %.2e b %.2e err %.2e" % (mode, len(r.pairs), rel(H, H_o), rel(b, b_o), abs(err - err_o) / err_o))
    assert err_o > 0 and rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * err_o
    assert np.array_equal(H, H.T)
    err2, H2, b2 = g.linearize(POSE)  # no floating-point atomics: the same bits
    assert err2 == err and np.array_equal(H2, H) and np.array_equal(b2, b)
    Tx = nr.known_transform(0.23, -0.12, 0.04, 0.035, 0.0)  # a second pose, stale pairs, R_lin of POSE
    assert g.compute_error(Tx) == pytest.approx(r.compute_error(Tx), rel=H_RTOL)
    assert g.compute_error(POSE) == pytest.approx(err_o, rel=H_RTOL)


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_whole_align(gorio, gpu, pose_err, mode, opt):
    src, tgt, T = nr.scene_pair(4096)
    r = ref_of(None, src, tgt, mode, gpu_tables=False)
    ro = r.align(optimizer=opt)
    # the scene was picked on the CPU so that a one-ulp map difference cannot flip a decision of the shell
    assert all(abs(x) >= 1e-3 for x in ro["rhos"]) and all(abs(m - 1.0) >= 0.01 for m in ro["measures"])
    g = make(gorio, gpu, mode, optimizer=apd.OPT_LEVENBERG_MARQUARDT if opt == "LM" else apd.OPT_GAUSS_NEWTON)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    out = g.align()
    te, re_ = pose_err(ro["T"], out["T"])
    print("NDTCuda mode %d %s: %d linearisations, pose difference %.2e m %.2e rad" % (mode, opt, out["n_linearize"], te, re_))
    assert te < 1e-4 and re_ < 1e-4
    assert (out["converged"], out["nr_iterations"], out["n_linearize"]) == (ro["converged"], ro["nr_iterations"], ro["n_linearize"])
    te, re_ = pose_err(T, out["T"])
    assert te < 0.05 and np.degrees(re_) < 1.0  # gicp_test.cpp:148-149
    assert g.align()["T"].tobytes() == out["T"].tobytes()


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_disjoint_clouds(gorio, gpu, mode, opt):
    src, tgt, _ = nr.scene_pair(600)
    far = src + F(500.0)
    r = ref_of(None, far, tgt, mode, gpu_tables=False)
    ro = r.align(optimizer=opt)
    g = make(gorio, gpu, mode, optimizer=apd.OPT_LEVENBERG_MARQUARDT if opt == "LM" else apd.OPT_GAUSS_NEWTON)
    g.setInputSource(far)
    g.setInputTarget(tgt)
    out = g.align()
    assert len(g.ndt_cuda_pairs()) == 0 and len(r.pairs) == 0
    assert (out["converged"], out["nr_iterations"], out["n_linearize"]) == (ro["converged"], ro["nr_iterations"], ro["n_linearize"])
    assert np.array_equal(out["T"], ro["T"]) and np.all(np.isfinite(out["T"])) and np.all(np.isfinite(out["H"]))
    err, H, b = g.linearize(np.eye(4))
    assert err == 0.0 and not H.any() and not b.any()


def test_lifecycle_swap_resolution_and_p2d_source_map(gorio, gpu, pose_err):
    src, tgt, T = nr.scene_pair(4096)
    g = make(gorio, gpu, nr.P2D)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    out = g.align()
    assert len(g.ndt_cuda_voxels(0)["num_points"]) == 0  # P2D builds no source map (ndt_cuda.cu:122)
    nt = len(g.ndt_cuda_voxels(1)["num_points"])
    assert nt == len(nr.build_map(tgt, 1.0)["num_points"])
    g.swapSourceAndTarget()  # clouds and maps change sides (ndt_cuda.cu:90-93): the old target's map is now the source's
    assert len(g.ndt_cuda_voxels(0)["num_points"]) == nt
    back = g.align()
    te, re_ = pose_err(np.linalg.inv(T), back["T"])
    assert te < 0.05 and np.degrees(re_) < 1.0
    r = ref_of(None, tgt, src, nr.P2D, gpu_tables=False)
    te, re_ = pose_err(r.align()["T"], back["T"])
    assert te < 1e-4 and re_ < 1e-4
    # a changed resolution rebuilds the map (documented deviation from ndt_cuda.cu:120-140)
    g.set_method(apd.METHOD_NDT_CUDA, 2.0, apd.VOXEL_DIRECT7)
    check_table(g.ndt_cuda_voxels(1), nr.build_map(src, 2.0))
    assert len(g.ndt_cuda_voxels(0)["num_points"]) == 0  # the map held has another resolution, and P2D builds none
    g.set_ndt_cuda_params(nr.D2D)
    check_table(g.ndt_cuda_voxels(0), nr.build_map(tgt, 2.0))
    assert out["converged"]


def test_shared_target_and_refusals(gorio, gpu):
    src, tgt, _ = nr.scene_pair(2048)
    a = make(gorio, gpu, nr.D2D)
    a.setInputSource(src)
    a.setInputTarget(tgt)
    ra = a.align()
    b = make(gorio, gpu, nr.D2D)
    b.setInputSource(src)
    b.setInputTargetShared(a)
    assert b.align()["T"].tobytes() == ra["T"].tobytes()  # the sharers share the map
    c = make(gorio, gpu, nr.D2D, resolution=2.0)
    with pytest.raises(gorio.GorioError) as e:
        c.setInputTargetShared(a)
    assert e.value.code == INVALID
    lib, h = a._lib, a._h
    n = a._n_src
    buf = np.zeros((n, 16))
    assert lib.gorio_apd_get_correspondences(h, None, None, n) == STATE
    assert lib.gorio_apd_get_mahalanobis(h, buf.ctypes.data_as(C.POINTER(C.c_double)), n) == STATE
    assert lib.gorio_apd_get_source_covariances(h, None, 0) == STATE and lib.gorio_apd_get_target_covariances(h, None, 0) == STATE
    assert lib.gorio_apd_set_source_covariances(h, buf.ctypes.data_as(C.POINTER(C.c_double)), n) == STATE
    assert lib.gorio_apd_calculate_covariances(h) == STATE
    assert lib.gorio_apd_debug_set_shard(h, 2, 0) == STATE
    assert lib.gorio_apd_icp_diag(h, None, None, None, None) == STATE
    # the rest of the surface keeps working in this mode
    moved = a.transformSource(ra["T"])
    assert moved.shape == (n, 3) and np.all(np.isfinite(moved))
    score, inl = a.getFitnessScore(ra["T"])
    assert np.isfinite(score) and 0.0 <= inl <= 1.0
    with pytest.raises(gorio.GorioError) as e:  # no pairs held after new points
        a.setInputSource(src[:100])
        a.ndt_cuda_pairs()
    assert e.value.code == STATE


def _scan_params(gorio, p):
    kw = {k: getattr(p, k) for k in ("power_threshold", "rotation", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul",
                                     "radius", "min_neighbors", "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size")}
    kw.update(enable_dynamic_object_removal=int(p.enable_dynamic_object_removal), deskew=int(p.deskew), ground=int(p.ground))
    sp = gorio.prep.scan_default_params(**kw)
    for k, v in p.reve.items():
        setattr(sp.reve, k, v)
    return sp


@pytest.mark.parametrize("mode", [nr.P2D, nr.D2D])
def test_keyframe_and_scan_hand_offs_equal_host_arrays(gorio, gpu, oracle_apd, mode):
    """A keyframe resident in the store and the output of the scan pipeline serve this method like host copies of the same clouds: same
    maps, same pairs, same pose bits; two handles holding one keyframe share its map."""
    import scan_pipeline_restatement as sr

    src, tgt, _ = nr.scene_pair(2048)
    store = gorio.KeyframeStore()
    kt, ks = store.add(tgt), store.add(src)
    a, b, c = make(gorio, gpu, mode), make(gorio, gpu, mode), make(gorio, gpu, mode)
    a.setInputTarget(tgt)
    a.setInputSource(src)
    for g in (b, c):
        g.setInputTargetKeyframe(store, kt)
        g.setInputSourceKeyframe(store, ks)
    ra, rb, rc = a.align(), b.align(), c.align()
    assert ra["T"].tobytes() == rb["T"].tobytes() == rc["T"].tobytes() and ra["n_linearize"] == rb["n_linearize"] >= 1
    assert np.array_equal(a.ndt_cuda_pairs(), b.ndt_cuda_pairs())
    ta, tb = a.ndt_cuda_voxels(1), b.ndt_cuda_voxels(1)
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    d = make(gorio, gpu, mode, resolution=2.0)  # the keyframe's map has another resolution: refused at the align, like a shared target's
    d.setInputTargetKeyframe(store, kt)
    d.setInputSource(src)
    with pytest.raises(gorio.GorioError) as e:
        d.align()
    assert e.value.code == INVALID
    # the scan pipeline's output as the source
    raw, p, samples = sr.chain_inputs(*sr.CHAIN_CASES[0], oracle_apd)
    pipe = gorio.prep.ScanPipeline(_scan_params(gorio, p))
    pipe.load(raw)
    assert pipe.run(samples, sr.CHAIN_ANG_VEL)["status"] == "ok"
    xyz = pipe.output()[0]
    g, h = make(gorio, gpu, mode, resolution=2.0), make(gorio, gpu, mode, resolution=2.0)
    g.setInputSourceFromScan(pipe)
    g.setInputTargetFromScan(pipe)
    h.setInputSource(xyz)
    h.setInputTarget(xyz)
    guess = nr.known_transform(0.1, 0.05, 0.0, 0.01, 0.0)
    rg, rh = g.align(guess), h.align(guess)
    assert rg["T"].tobytes() == rh["T"].tobytes() and rg["n_linearize"] == rh["n_linearize"] >= 1
    assert len(g.ndt_cuda_pairs()) > 0 and np.array_equal(g.ndt_cuda_pairs(), h.ndt_cuda_pairs())
    pipe.close()
    store.close()
