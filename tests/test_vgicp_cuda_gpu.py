"""GPU parity tests of GORIO_METHOD_VGICP_CUDA (fast_gicp::FastVGICPCuda) against the NumPy restatement tests/vgicp_cuda_restatement.py.

Gates: k-NN raw covariances bit-exact; RBF raw covariances measured against a float64 evaluation next to the float32 restatement (expf on
the device and NumPy's float32 exp need not agree in the last bit); keep masks equal; regularised covariances within one float ulp of the
matrix's largest entry (both sides round a double result that agrees far below half an ulp); voxel tables and pair lists bit-exact; H, b,
error relative 1e-9 against the restatement's pair arithmetic fed with the GPU's own tables; poses within 1e-4 m / 1e-4 rad with equal
iteration counts.
"""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import ndt_cuda_restatement as nr
import vgicp_cuda_restatement as vr
from map_checks import rel

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu

F = np.float32
H_RTOL = 1e-9  # the project's gate, as tests/test_gicp_variants_gpu.py applies it
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SEARCH = {nr.DIRECT1: apd.VOXEL_DIRECT1, nr.DIRECT7: apd.VOXEL_DIRECT7, nr.DIRECT27: apd.VOXEL_DIRECT27, nr.DIRECT_RADIUS: apd.VOXEL_DIRECT_RADIUS}
POSE = nr.known_transform(0.2, -0.1, 0.05, 0.02, -0.01)


def make(gorio, gpu, nn=vr.CPU_PARALLEL_KDTREE, search=nr.DIRECT1, resolution=1.0, radius=-1.0, width=0.5, maxd=3.0, **params):
    g = gorio.ApdGicp(device=gpu, **params)
    g.set_vgicp_cuda_params(nn, width, maxd)
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, radius)
    g.set_method(apd.METHOD_VGICP_CUDA, resolution, SEARCH[search])
    return g


def ref_of(g, src, tgt, gpu_tables=True, **kw):
    """the restatement object; with gpu_tables its kept points, covariances and map are the GPU's own (parity hooks), so only the pair
    arithmetic is compared"""
    r = vr.VgicpCuda(**kw)
    r.setInputSource(src)
    r.setInputTarget(tgt)
    if gpu_tables:
        r.adopt(r.source, g.vgicp_cuda_points(0))
        r.adopt(r.target, g.vgicp_cuda_points(1), g.vgicp_cuda_voxels())
    return r


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


# ------------------------------------------------------------------------------------------------ raw covariances

@pytest.mark.parametrize("k", [5, 20])
@pytest.mark.parametrize("n", ["k", "k+1", 255, 256, 257, 700])
def test_knn_raw_covariances_bit_exact(gorio, gpu, n, k):
    n = {"k": k, "k+1": k + 1}.get(n, n)
    cloud = vr.rail_scene(700)[:n]
    g = make(gorio, gpu, k_correspondences=k)
    g.setInputTarget(cloud)
    got = g.vgicp_cuda_points(1)["cov_raw"]
    assert same_bits(got, vr.cov_knn(cloud, vr.knn(cloud, k)))
    g.set_vgicp_cuda_params(vr.GPU_BRUTEFORCE)  # the same path: nothing is made again, nothing changes
    assert same_bits(g.vgicp_cuda_points(1)["cov_raw"], got)


def test_knn_fewer_points_than_k_is_invalid(gorio, gpu):
    g = make(gorio, gpu)
    g.setInputTarget(vr.rail_scene(700)[:19])
    with pytest.raises(gorio.GorioError) as e:
        g.vgicp_cuda_points(1)
    assert e.value.code == INVALID
    g.set_vgicp_cuda_params(vr.GPU_RBF_KERNEL)  # no list, no k
    assert g.vgicp_cuda_points(1)["cov_raw"].shape == (19, 6)


def rbf_cloud(n):
    """the first n points of the 3000-point scene, a point within max_dist of the origin first (so that n = 1 sees the padding)"""
    c = vr.rail_scene(3000)
    i = int(np.argmin((c.astype(np.float64) ** 2).sum(axis=1)))
    c[[0, i]] = c[[i, 0]]
    return c[:n].copy()


@functools.lru_cache(maxsize=None)
def rbf_refs(n):
    c = rbf_cloud(n)
    return c, vr.cov_rbf(c, 0.5, 3.0), vr.cov_rbf(c, 0.5, 3.0, np.float64)


@pytest.mark.parametrize("n", [1, 511, 512, 513, 700, 3000])
def test_rbf_raw_covariances_against_float64(gorio, gpu, n):
    """GPU and float32 restatement each against the float64 evaluation, per point, in ulps of the largest |p|^2 in range.  Both are float
    accumulations of the same length in the same order and differ only in expf's last bits: the GPU's worst error must stay within 4 x the
    restatement's own worst error on the same cloud."""
    c, r32, r64 = rbf_refs(n)
    assert ((c.astype(np.float64) ** 2).sum(axis=1) <= 9.0).sum() >= 1  # the padding matters
    g = make(gorio, gpu, nn=vr.GPU_RBF_KERNEL)
    g.setInputTarget(c)
    got = g.vgicp_cuda_points(1)["cov_raw"]
    ext = np.zeros(((n + 511) // 512 * 512, 3), F)
    ext[:n] = c
    inr = ~(vr.sqdist(c, ext) > F(9.0))
    scale = np.spacing(np.where(inr, (ext.astype(np.float64) ** 2).sum(axis=1)[None, :], 0.0).max(axis=1).astype(F)).astype(np.float64)
    scale = np.maximum(scale, np.spacing(F(1e-3)))
    e_gpu = (np.abs(got.astype(np.float64) - r64).max(axis=1) / scale).max()
    e_ref = (np.abs(r32.astype(np.float64) - r64).max(axis=1) / scale).max()
    print("RBF n %d: worst error GPU %.3f ulp, float32 restatement %.3f ulp, equal bits on %.1f %% of the points"
          % (n, e_gpu, e_ref, 100.0 * np.mean(np.all(got.view(np.uint32) == r32.view(np.uint32), axis=1))))
    assert np.all(np.isfinite(got)) and e_gpu <= 4.0 * e_ref
    assert same_bits(g.vgicp_cuda_points(1)["cov_raw"], got)


def test_rbf_kernel_parameters(gorio, gpu):
    """kernel_max_dist <= 0 means 5 kernel_width (fast_vgicp_cuda_impl.hpp:46-50); a changed width makes the covariances again"""
    c = rbf_cloud(700)
    g = make(gorio, gpu, nn=vr.GPU_RBF_KERNEL, width=0.4, maxd=-1.0)
    g.setInputTarget(c)
    a = g.vgicp_cuda_points(1)["cov_raw"]
    g.set_vgicp_cuda_params(vr.GPU_RBF_KERNEL, 0.4, 2.0)
    assert same_bits(g.vgicp_cuda_points(1)["cov_raw"], a)
    g.set_vgicp_cuda_params(vr.GPU_RBF_KERNEL, 0.4, 3.0)
    b = g.vgicp_cuda_points(1)["cov_raw"]
    assert not same_bits(a, b)
    r64 = vr.cov_rbf(c, 0.4, 3.0, np.float64)
    assert np.abs(b - r64).max() < 1e-4


# ------------------------------------------------------------------------------------------------ regularisation and compaction

def line_cloud():
    t = np.linspace(0.0, 4.0, 300)
    return np.c_[1.0 + t, 2.0 + 0.5 * t, 0.25 * t].astype(F)


REG_CASES = {"scene_knn": (lambda: vr.scene_pair(3000)[1], vr.CPU_PARALLEL_KDTREE), "scene_rbf": (lambda: vr.scene_pair(3000)[1], vr.GPU_RBF_KERNEL),
             "small": (lambda: vr.scene_pair(700)[0][:300], vr.CPU_PARALLEL_KDTREE), "line": (line_cloud, vr.CPU_PARALLEL_KDTREE)}


@pytest.mark.parametrize("reg", [vr.PLANE, vr.MIN_EIG, vr.FROBENIUS, vr.NONE])
@pytest.mark.parametrize("case", sorted(REG_CASES))
def test_keep_mask_and_regularised_covariances(gorio, gpu, case, reg):
    fn, nn = REG_CASES[case]
    cloud = fn()
    g = make(gorio, gpu, nn=nn, regularization=reg)
    g.setInputSource(cloud)
    got = g.vgicp_cuda_points(0)
    keep, cov = vr.regularize(got["cov_raw"], reg)  # the restatement is fed the GPU's own raw covariances
    idx = np.flatnonzero(keep)
    assert np.array_equal(got["kept_index"], idx)  # an order-preserving compaction
    if reg != vr.PLANE:
        assert len(idx) == len(cloud)
    elif case == "line":
        assert len(idx) == 0  # every point is filtered away
    elif case.startswith("scene"):
        assert 256 < len(idx) < len(cloud) and len(idx) % 256 != 0  # the kept points cross workgroup boundaries of the compaction
    ref = cov[idx]
    if len(idx):
        ulp = np.spacing(np.abs(ref).max(axis=1))
        d = np.abs(got["cov"].astype(np.float64) - ref.astype(np.float64)).max(axis=1)
        print("%s reg %d: kept %d of %d, worst difference %.3g ulp of the largest entry" % (case, reg, len(idx), len(cloud), (d / ulp).max()))
        assert np.all(d <= ulp)
    if reg == vr.NONE:
        assert same_bits(got["cov"], got["cov_raw"])


# ------------------------------------------------------------------------------------------------ voxel map

def edge_cloud():
    """voxels of 1, 6, 7 and 300 points, points exactly on voxel faces, in a shuffled order"""
    rng = np.random.default_rng(11)
    parts = [rng.uniform(0.6, 1.4, (300, 3)), np.array([[4.0, 1.0, 1.0]]), rng.uniform(0.6, 1.4, (6, 3)) + [0, 3, 0], rng.uniform(0.6, 1.4, (7, 3)) + [0, 0, 3]]
    faces = np.array([[0.5, 5.2, 5.1], [1.5, 5.2, 5.1], [-0.5, 5.2, 5.1], [2.5, 5.5, 5.1], [5.2, 0.5, 1.5], [5.2, -1.5, -0.5], [-2.5, -2.5, -2.5]])
    pts = np.concatenate(parts + [faces]).astype(F)
    return pts[rng.permutation(len(pts))]


VOXEL_CASES = {"edges": (edge_cloud, 1.0, vr.MIN_EIG, 5), "scene": (lambda: vr.scene_pair(3000)[1], 1.0, vr.PLANE, 20), "coarse": (lambda: vr.scene_pair(700)[1], 2.5, vr.PLANE, 20),
               "float_rule": (lambda: np.concatenate([np.full((1, 3), nr.FLOAT_RULE_POINT), np.random.default_rng(6).uniform(-3, 3, (700, 3))]).astype(F),
                              nr.FLOAT_RULE_RESOLUTION, vr.FROBENIUS, 20)}


@pytest.mark.parametrize("case", sorted(VOXEL_CASES))
def test_voxel_table_bit_exact(gorio, gpu, case):
    fn, res, reg, k = VOXEL_CASES[case]
    cloud = fn()
    g = make(gorio, gpu, resolution=res, regularization=reg, k_correspondences=k)
    g.setInputTarget(cloud)
    pts, tab = g.vgicp_cuda_points(1), g.vgicp_cuda_voxels()
    ref = vr.build_map(cloud[pts["kept_index"]], pts["cov"], res)  # the restatement is fed the GPU's own per-point covariances
    assert np.array_equal(tab["coord"], ref["coord"]) and np.array_equal(tab["num_points"], ref["num_points"])
    assert same_bits(tab["mean"], ref["mean"]) and same_bits(tab["cov"], ref["cov6"])
    assert ref["num_points"].sum() == len(pts["kept_index"])  # no voxel, no kept point is dropped
    if case == "edges":
        assert {1, 6, 7, 300} <= set(ref["num_points"].tolist())
    if case == "float_rule":
        assert np.any(np.all(tab["coord"] == nr.voxel_coord(cloud[:1], res)[0], axis=1))


# ------------------------------------------------------------------------------------------------ pairs and sums

@pytest.mark.parametrize("search,radius", [(nr.DIRECT1, -1.0), (nr.DIRECT7, -1.0), (nr.DIRECT27, -1.0), (nr.DIRECT_RADIUS, 1.5)])
def test_pair_list_per_offset_mode(gorio, gpu, search, radius):
    src, tgt, _ = vr.scene_pair(3000)
    g = make(gorio, gpu, search=search, radius=radius)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    err, H, b = g.linearize(POSE)
    r = ref_of(g, src, tgt, search=search, radius=radius)
    err_o, H_o, b_o = r.linearize(POSE)
    assert len(r.pairs) > 0 and np.array_equal(g.vgicp_cuda_pairs(), r.pairs)
    assert r.pairs[:, 0].max() < len(r.kept(r.source)["index"]) < len(src)  # items are kept points
    assert rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * abs(err_o)


@pytest.mark.parametrize("nn", [vr.CPU_PARALLEL_KDTREE, vr.GPU_RBF_KERNEL])
def test_linearize_and_compute_error(gorio, gpu, nn):
    src, tgt, _ = vr.scene_pair(3000)
    g = make(gorio, gpu, nn=nn, search=nr.DIRECT7)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    err, H, b = g.linearize(POSE)
    r = ref_of(g, src, tgt, nn_method=nn, search=nr.DIRECT7)
    err_o, H_o, b_o = r.linearize(POSE)
    assert np.array_equal(g.vgicp_cuda_pairs(), r.pairs)
    print("FastVGICPCuda nn %d linearize: pairs %d, H %.2e b %.2e err %.2e" % (nn, len(r.pairs), rel(H, H_o), rel(b, b_o), abs(err - err_o) / err_o))
    assert err_o > 0 and rel(H, H_o) < H_RTOL and rel(b, b_o) < H_RTOL and abs(err - err_o) <= H_RTOL * err_o
    assert np.array_equal(H, H.T)
    err2, H2, b2 = g.linearize(POSE)  # no floating-point atomics: the same bits
    assert err2 == err and np.array_equal(H2, H) and np.array_equal(b2, b)
    Tx = nr.known_transform(0.23, -0.12, 0.04, 0.035, 0.0)  # a second pose, stale pairs, R_lin of POSE
    assert g.compute_error(Tx) == pytest.approx(r.compute_error(Tx), rel=H_RTOL)
    assert g.compute_error(POSE) == pytest.approx(err_o, rel=H_RTOL)
    assert np.array_equal(g.vgicp_cuda_pairs(), r.pairs)  # compute_error left the pairs alone


# ------------------------------------------------------------------------------------------------ whole aligns

@functools.lru_cache(maxsize=None)
def ref_align(nn, opt):
    src, tgt, _ = vr.scene_pair(3000)
    r = ref_of(None, src, tgt, gpu_tables=False, nn_method=nn)
    return r.align(optimizer=opt)


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("nn", [vr.CPU_PARALLEL_KDTREE, vr.GPU_BRUTEFORCE, vr.GPU_RBF_KERNEL])
def test_whole_align(gorio, gpu, pose_err, nn, opt):
    src, tgt, T = vr.scene_pair(3000)
    ro = ref_align(vr.CPU_PARALLEL_KDTREE if nn == vr.GPU_BRUTEFORCE else nn, opt)
    # the scene was picked on the CPU (tests/test_vgicp_cuda_restatement.py) so that a one-ulp difference cannot flip a keep flag or a decision of the shell
    assert all(abs(x) >= 1e-3 for x in ro["rhos"]) and all(abs(m - 1.0) >= 0.01 for m in ro["measures"])
    g = make(gorio, gpu, nn=nn, optimizer=apd.OPT_LEVENBERG_MARQUARDT if opt == "LM" else apd.OPT_GAUSS_NEWTON)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    out = g.align()
    te, re_ = pose_err(ro["T"], out["T"])
    print("FastVGICPCuda nn %d %s: %d linearisations, pose difference %.2e m %.2e rad" % (nn, opt, out["n_linearize"], te, re_))
    assert te < 1e-4 and re_ < 1e-4
    assert (out["converged"], out["nr_iterations"], out["n_linearize"]) == (ro["converged"], ro["nr_iterations"], ro["n_linearize"])
    te, re_ = pose_err(T, out["T"])
    assert te < 0.05 and np.degrees(re_) < 1.0  # gicp_test.cpp:148-149
    again = g.align()
    assert again["T"].tobytes() == out["T"].tobytes() and again["H"].tobytes() == out["H"].tobytes()


@pytest.mark.parametrize("opt", ["LM", "GN"])
@pytest.mark.parametrize("case", ["disjoint", "all_filtered"])
def test_empty_pair_list(gorio, gpu, case, opt):
    src, tgt, _ = vr.scene_pair(700)
    far = src + F(500.0) if case == "disjoint" else line_cloud()
    r = ref_of(None, far, tgt, gpu_tables=False)
    ro = r.align(optimizer=opt)
    g = make(gorio, gpu, optimizer=apd.OPT_LEVENBERG_MARQUARDT if opt == "LM" else apd.OPT_GAUSS_NEWTON)
    g.setInputSource(far)
    g.setInputTarget(tgt)
    out = g.align()
    assert len(g.vgicp_cuda_pairs()) == 0 and len(r.pairs) == 0
    assert (len(g.vgicp_cuda_points(0)["kept_index"]) == 0) == (case == "all_filtered")
    assert (out["converged"], out["nr_iterations"], out["n_linearize"]) == (ro["converged"], ro["nr_iterations"], ro["n_linearize"])
    assert np.array_equal(out["T"], ro["T"]) and np.all(np.isfinite(out["T"])) and np.all(np.isfinite(out["H"]))
    err, H, b = g.linearize(np.eye(4))
    assert err == 0.0 and not H.any() and not b.any()
    assert g.compute_error(POSE) == 0.0


def test_target_filtered_away_gives_an_empty_map(gorio, gpu):
    src, _, _ = vr.scene_pair(700)
    g = make(gorio, gpu)
    g.setInputSource(src)
    g.setInputTarget(line_cloud())
    assert len(g.vgicp_cuda_voxels()["num_points"]) == 0
    err, H, b = g.linearize(np.eye(4))
    assert err == 0.0 and not H.any() and len(g.vgicp_cuda_pairs()) == 0


# ------------------------------------------------------------------------------------------------ lifecycle

def test_lifecycle_swap_and_changed_settings(gorio, gpu, pose_err):
    src, tgt, T = vr.scene_pair(3000)
    g = make(gorio, gpu)
    g.setInputSource(src)
    g.setInputTarget(tgt)
    out = g.align()
    ps, pt, vox = g.vgicp_cuda_points(0), g.vgicp_cuda_points(1), g.vgicp_cuda_voxels()
    g.swapSourceAndTarget()  # clouds, covariances and kept points change sides; the new target's map is built (fast_vgicp_cuda.cu:97-107)
    qs, qt = g.vgicp_cuda_points(0), g.vgicp_cuda_points(1)
    assert all(same_bits(ps[k], qt[k]) and same_bits(pt[k], qs[k]) for k in ("cov_raw", "cov")) and np.array_equal(ps["kept_index"], qt["kept_index"])
    ref = vr.build_map(src[qt["kept_index"]], qt["cov"], 1.0)
    tab = g.vgicp_cuda_voxels()
    assert np.array_equal(tab["coord"], ref["coord"]) and same_bits(tab["cov"], ref["cov6"]) and len(tab["coord"]) != len(vox["coord"])
    back = g.align()
    te, re_ = pose_err(np.linalg.inv(T), back["T"])
    assert out["converged"] and te < 0.05 and np.degrees(re_) < 1.0
    # a changed resolution rebuilds the map and nothing else (documented deviation)
    g.set_method(apd.METHOD_VGICP_CUDA, 2.0, apd.VOXEL_DIRECT1)
    tab2 = g.vgicp_cuda_voxels()
    ref2 = vr.build_map(src[qt["kept_index"]], qt["cov"], 2.0)
    assert np.array_equal(tab2["coord"], ref2["coord"]) and same_bits(tab2["cov"], ref2["cov6"]) and len(tab2["coord"]) < len(tab["coord"])
    assert same_bits(g.vgicp_cuda_points(1)["cov"], qt["cov"])
    # another regularisation: the raw covariances stay, kept points and map follow
    g.set_params(regularization=vr.MIN_EIG)
    q2 = g.vgicp_cuda_points(1)
    assert same_bits(q2["cov_raw"], qt["cov_raw"]) and len(q2["kept_index"]) == len(src)
    assert g.vgicp_cuda_voxels()["num_points"].sum() == len(src)
    # another neighbour method / kernel width: everything follows
    g.set_vgicp_cuda_params(vr.GPU_RBF_KERNEL, 0.5, 3.0)
    q3 = g.vgicp_cuda_points(1)
    assert not same_bits(q3["cov_raw"], q2["cov_raw"])
    g.set_vgicp_cuda_params(vr.GPU_RBF_KERNEL, 0.3, 3.0)
    q4 = g.vgicp_cuda_points(1)
    assert not same_bits(q4["cov_raw"], q3["cov_raw"])
    g.set_params(regularization=vr.MIN_EIG, k_correspondences=10)  # k shapes nothing in the RBF mode
    assert same_bits(g.vgicp_cuda_points(1)["cov_raw"], q4["cov_raw"])
    g.set_vgicp_cuda_params(vr.CPU_PARALLEL_KDTREE)
    assert same_bits(g.vgicp_cuda_points(1)["cov_raw"], vr.cov_knn(src, vr.knn(src, 10)))


def test_shared_target_refusals_and_the_unfiltered_surface(gorio, gpu):
    src, tgt, _ = vr.scene_pair(3000)
    a = make(gorio, gpu)
    a.setInputSource(src)
    a.setInputTarget(tgt)
    ra = a.align()
    b = make(gorio, gpu)
    b.setInputSource(src)
    b.setInputTargetShared(a)
    assert b.align()["T"].tobytes() == ra["T"].tobytes()  # the sharers share kept points, covariances and map
    for kw in (dict(resolution=2.0), dict(nn=vr.GPU_RBF_KERNEL), dict(regularization=vr.MIN_EIG), dict(k_correspondences=10)):
        c = make(gorio, gpu, **kw)
        with pytest.raises(gorio.GorioError) as e:
            c.setInputTargetShared(a)
        assert e.value.code == INVALID, kw
    b.set_params(regularization=vr.FROBENIUS)  # a sharer that changes its mind is refused at the align
    with pytest.raises(gorio.GorioError) as e:
        b.align()
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
    k = C.c_int(0)
    assert lib.gorio_apd_ndt_cuda_get_pairs(h, 0, C.byref(k), None, None) == STATE  # the other method's hook
    # the filter dropped points, and transform_source and the fitness score still see the whole cloud, as PCL does with input_
    assert len(a.vgicp_cuda_points(0)["kept_index"]) < n
    moved = a.transformSource(ra["T"])
    assert moved.shape == (n, 3) and np.all(np.isfinite(moved))
    plain = gorio.ApdGicp(device=gpu)
    plain.setInputSource(src)
    plain.setInputTarget(tgt)
    assert a.getFitnessScore(ra["T"]) == plain.getFitnessScore(ra["T"])
    with pytest.raises(gorio.GorioError) as e:  # no pairs held after new points
        a.setInputSource(src[:100])
        a.vgicp_cuda_pairs()
    assert e.value.code == STATE


def test_keyframe_target_by_id_equals_the_host_cloud(gorio, gpu):
    src, tgt, _ = vr.scene_pair(3000)
    store = gorio.KeyframeStore()
    kt = store.add(tgt)
    a, b = make(gorio, gpu), make(gorio, gpu)
    a.setInputTarget(tgt)
    a.setInputSource(src)
    b.setInputTargetKeyframe(store, kt)
    b.setInputSource(src)
    ra, rb = a.align(), b.align()
    assert ra["T"].tobytes() == rb["T"].tobytes() and ra["H"].tobytes() == rb["H"].tobytes() and ra["n_linearize"] == rb["n_linearize"] >= 1
    assert np.array_equal(a.vgicp_cuda_pairs(), b.vgicp_cuda_pairs())
    ta, tb = a.vgicp_cuda_voxels(), b.vgicp_cuda_voxels()
    assert all(np.array_equal(ta[k], tb[k]) for k in ta)
    store.close()
