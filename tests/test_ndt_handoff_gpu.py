"""NDT fed from the device-resident front end (include/gorio_ndt.h): gorio_ndt_set_source_from_scan / _set_target_from_scan against the
host round trip through gorio_scan_get_output, gorio_ndt_set_target_from_apd against gorio_apd_get_target_points, and
gorio_ndt_calculate_score_batch against the single calls.  Both sides of every comparison run the same kernels on the same points, so
everything is compared bit for bit; only the last test, the single score against the NumPy restatement, has a tolerance, and it is
the one tests/test_ndt_gpu.py uses for that comparison."""
import numpy as np
import pytest

import ndt_restatement as R
import ndt_scenes as S
import scan_pipeline_restatement as sr
import test_ndt_gpu as base

pytestmark = pytest.mark.gpu
F = np.float32
REL = base.REL  # the score against the restatement: tests/test_ndt_gpu.py's bound, not a new one
POSES = (np.zeros(6), np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03]))
NDT_KW = dict(resolution=1.0, search=R.DIRECT7)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _params(gorio, p):
    kw = {k: getattr(p, k) for k in ("power_threshold", "rotation", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul",
                                     "radius", "min_neighbors", "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size")}
    kw.update(enable_dynamic_object_removal=int(p.enable_dynamic_object_removal), deskew=int(p.deskew), ground=int(p.ground))
    sp = gorio.prep.scan_default_params(**kw)
    for k, v in p.reve.items():
        setattr(sp.reve, k, v)
    return sp


def _moved(xyz, t, yaw):
    c, s = np.cos(yaw), np.sin(yaw)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    return (xyz.astype(np.float64) @ Rz.T + np.asarray(t, np.float64)).astype(F)


def _same_align(a, b):
    assert np.array_equal(_bits(a["T"]), _bits(b["T"]))
    for k in ("converged", "nr_iterations", "n_derivatives", "n_hessians", "n_mt"):
        assert a[k] == b[k], k
    for k in ("trans_probability", "score"):
        assert np.array_equal(_bits(np.float64(a[k]).reshape(1)), _bits(np.float64(b[k]).reshape(1))), k


def _same_derivs(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(_bits(np.asarray(x, np.float64).reshape(-1)), _bits(np.asarray(y, np.float64).reshape(-1)))


def _same_voxels(a, b):
    assert set(a) == set(b) and len(a["leaf_index"]) > 0
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def _run(pipe, frame):
    raw, samples = frame
    pipe.load(raw)
    r = pipe.run(samples, sr.CHAIN_ANG_VEL)
    assert r["status"] == "ok"
    return r


@pytest.fixture(scope="module")
def case(gpu, gorio, oracle_apd):
    """Two small radar messages of the scan-pipeline tests, frame 1's published cloud, a host target and a host source made from it, and
    the host route's results for them: computed once, read by the tests."""
    frames, p = [], None
    for seed in sr.SEQUENCE_SEEDS[:2]:
        raw, p, samples = sr.chain_inputs(seed, False, sr.OUTLIER_STATISTICAL, oracle_apd, n_ground=sr.SEQUENCE_N_GROUND)
        frames.append((raw, samples))
    sp = _params(gorio, p)
    pipe = gorio.prep.ScanPipeline(sp)
    _run(pipe, frames[0])
    xyz1 = pipe.output()[0]
    pipe.close()
    assert 2000 < len(xyz1) < 6000 and np.isfinite(xyz1).all()
    tgt = _moved(xyz1, (0.25, -0.15, 0.02), 0.015)  # the keyframe: the same scene seen from a pose 0.3 m / 0.9 degrees away
    src = _moved(xyz1, (-0.2, 0.1, 0.0), -0.01)
    a = gorio.Ndt(device=gpu, **NDT_KW)
    a.set_source(xyz1)
    a.set_target(tgt)
    source_ref = dict(derivs=[a.derivatives(q, True) for q in POSES], align=a.align())
    a.set_source(src)
    a.set_target(xyz1)
    target_ref = dict(voxels=a.voxels(), align=a.align())
    a.close()
    assert source_ref["align"]["nr_iterations"] >= 1 and source_ref["derivs"][0][0] != 0.0  # the scene has leaves that count
    assert (target_ref["voxels"]["nr_points"] >= 6).sum() > 20
    return dict(frames=frames, params=sp, xyz1=xyz1, tgt=tgt, src=src, source_ref=source_ref, target_ref=target_ref)


def test_source_hand_off_equals_the_host_round_trip(gpu, gorio, case):
    pipe = gorio.prep.ScanPipeline(case["params"])
    _run(pipe, case["frames"][0])
    assert np.array_equal(_bits(pipe.output()[0]), _bits(case["xyz1"]))
    b = gorio.Ndt(device=gpu, **NDT_KW)
    b.set_source_from_scan(pipe)
    b.set_target(case["tgt"])
    for q, ref in zip(POSES, case["source_ref"]["derivs"]):
        _same_derivs(b.derivatives(q, True), ref)  # score, 6 gradient and 21 + mirrored Hessian sums
    _same_align(b.align(), case["source_ref"]["align"])
    assert b.capacities()["source"] >= len(case["xyz1"])
    b.set_source_from_scan(pipe)  # a second hand-off lands in the other buffer of the pair: the same source again
    _same_align(b.align(), case["source_ref"]["align"])
    b.close()
    pipe.close()


def test_target_hand_off_equals_the_host_round_trip(gpu, gorio, case):
    pipe = gorio.prep.ScanPipeline(case["params"])
    _run(pipe, case["frames"][0])
    b = gorio.Ndt(device=gpu, **NDT_KW)
    b.set_target_from_scan(pipe)
    b.set_source(case["src"])
    _same_voxels(b.voxels(), case["target_ref"]["voxels"])
    _same_align(b.align(), case["target_ref"]["align"])
    b.close()
    pipe.close()


def test_the_copy_is_independent_of_the_pipeline_and_moves_no_counter(gpu, gorio, case):
    pipe = gorio.prep.ScanPipeline(case["params"])
    _run(pipe, case["frames"][0])
    b, t = gorio.Ndt(device=gpu, **NDT_KW), gorio.Ndt(device=gpu, **NDT_KW)
    c0 = pipe.counters()
    assert c0 == dict(point_uploads=1, index_builds=2, point_downloads=0)
    b.set_source_from_scan(pipe)
    assert pipe.counters() == c0
    t.set_target_from_scan(pipe)
    assert pipe.counters() == c0
    r2 = _run(pipe, case["frames"][1])  # the pipeline goes on to its next frame, in the same buffers
    c1 = pipe.counters()
    assert c1 == dict(point_uploads=2, index_builds=4, point_downloads=0)
    assert r2["n_out"] > 0
    b.set_target(case["tgt"])
    _same_align(b.align(), case["source_ref"]["align"])
    t.set_source(case["src"])
    _same_voxels(t.voxels(), case["target_ref"]["voxels"])
    _same_align(t.align(), case["target_ref"]["align"])
    assert pipe.counters() == c1
    pipe.close()  # the handles keep what they copied
    _same_align(b.align(), case["source_ref"]["align"])
    b.close()
    t.close()


def test_state_errors_and_sharing(gpu, gorio, case):
    b = gorio.Ndt(device=gpu, **NDT_KW)
    b.set_source(case["xyz1"])
    b.set_target(case["tgt"])
    fresh = gorio.prep.ScanPipeline(case["params"])  # never loaded
    empty = gorio.prep.ScanPipeline(case["params"])  # its last run ended without a frame
    empty.load(case["frames"][0][0][:0])
    assert empty.run([], None)["status"] == "empty"
    for pipe in (fresh, empty):
        for call in (b.set_source_from_scan, b.set_target_from_scan):
            with pytest.raises(gorio.GorioError) as e:
                call(pipe)
            assert e.value.code == -3 and "produced no frame" in str(e.value)  # GORIO_ERR_STATE
    _same_align(b.align(), case["source_ref"]["align"])  # what it held is untouched
    fresh.close()
    empty.close()
    # a sharer that takes a scan as its target detaches alone
    pipe = gorio.prep.ScanPipeline(case["params"])
    _run(pipe, case["frames"][0])
    s1, s2 = gorio.Ndt(device=gpu, **NDT_KW), gorio.Ndt(device=gpu, **NDT_KW)
    s1.set_target_shared(b)
    s2.set_target_shared(b)
    owner_voxels, owner_caps = b.voxels(), b.capacities()
    s1.set_target_from_scan(pipe)
    _same_voxels(b.voxels(), owner_voxels)
    _same_voxels(s2.voxels(), owner_voxels)
    assert b.capacities() == owner_caps and s2.capacities()["target"] == 0 and s1.capacities()["target"] >= len(case["xyz1"])
    _same_voxels(s1.voxels(), case["target_ref"]["voxels"])
    s1.set_source(case["src"])
    _same_align(s1.align(), case["target_ref"]["align"])
    _same_align(b.align(), case["source_ref"]["align"])
    # the owner takes a scan: its sharer keeps the old target
    b.set_target_from_scan(pipe)
    _same_voxels(s2.voxels(), owner_voxels)
    _same_voxels(b.voxels(), case["target_ref"]["voxels"])
    for h in (b, s1, s2):
        h.close()
    pipe.close()


@pytest.mark.parametrize("leaf", [0.0, 0.5])
def test_submap_target_from_a_registration_handle(gpu, gorio, leaf):
    frames = [(S.clusters(700, 60 + k), None) for k in range(3)]
    rel = [np.eye(4) for _ in range(3)]
    for k in range(3):
        rel[k][:3, 3] = (0.2 * (2 - k), -0.1 * (2 - k), 0.0)
    g = gorio.ApdGicp()
    a, b = gorio.Ndt(device=gpu, **NDT_KW), gorio.Ndt(device=gpu, **NDT_KW)
    with pytest.raises(gorio.GorioError) as e:
        b.set_target_from_apd(g)  # no target yet
    assert e.value.code == -3
    n = g.setInputTargetSubmap(frames, rel, voxel_leaf=leaf)
    assert (n == 2100) if leaf == 0.0 else (200 < n < 2100)
    b.set_target_from_apd(g)
    xg, _ = g.getTargetPoints()
    assert len(xg) == n
    a.set_target(xg)
    va, vb = a.voxels(), b.voxels()
    _same_voxels(vb, va)
    if leaf == 0.0:
        assert (va["nr_points"] >= 6).sum() > 20
    src = _moved(frames[2][0], (0.1, -0.05, 0.02), 0.01)
    a.set_source(src)
    b.set_source(src)
    ra, rb = a.align(), b.align()
    _same_align(rb, ra)
    if leaf == 0.0:
        assert ra["nr_iterations"] >= 1 and ra["score"] != 0.0
    # the registration handle may move on
    g.setInputTargetSubmap(frames[:1], rel[:1], voxel_leaf=0.0)
    _same_voxels(b.voxels(), va)
    del g  # the registration handle is destroyed: the copy stays
    _same_align(b.align(), ra)
    a.close()
    b.close()


SIZES = (1, 255, 256, 257, 600)  # the edges of the 256-point blocks, and a job whose last block holds one point


@pytest.fixture(scope="module")
def score_case(gpu, gorio):
    """Handles of the batched score: five sources of SIZES against one shared target of 2048 points, a sixth handle with a target of its
    own at resolution 2; a pose per handle; the single scores."""
    tgt, tgt2 = S.clusters(2048, 41), S.clusters(1500, 43, offset=2.0)
    vm, vm2 = R.build_voxel_map(tgt, 1.0), R.build_voxel_map(tgt2, 2.0)
    owner = gorio.Ndt(device=gpu, **NDT_KW)
    owner.set_target(tgt)
    handles, sources = [], []
    for k, n in enumerate(SIZES):
        h = owner if k == 0 else gorio.Ndt(device=gpu, **NDT_KW)
        if k:
            h.set_target_shared(owner)
        src = _moved(tgt[np.linspace(0, len(tgt) - 1, n).astype(int)], (0.05, -0.03, 0.02), 0.0) if n > 1 else vm.mean[np.argmax(vm.count)][None, :].astype(F)
        h.set_source(src)
        handles.append(h)
        sources.append(src)
    own = gorio.Ndt(device=gpu, resolution=2.0, search=R.DIRECT7)
    own.set_target(tgt2)
    sources.append(_moved(tgt2[::5], (0.1, 0.05, -0.02), 0.0))
    own.set_source(sources[-1])
    handles.append(own)
    Ts = [R.pose_matrix(np.array([0.02 * k, -0.01 * k, 0.005 * k, 0.002 * k, -0.003 * k, 0.004 * k])) for k in range(1, len(handles) + 1)]
    single = np.array([h.calculate_score(T) for h, T in zip(handles, Ts)])
    assert (single != 0).all() and len(set(single.tolist())) == len(single)
    yield dict(handles=handles, sources=sources, Ts=Ts, single=single, maps=[vm] * len(SIZES) + [vm2], res=[1.0] * len(SIZES) + [2.0])
    for h in handles:
        h.close()


def test_score_batch_equals_the_single_calls_bit_for_bit(gpu, gorio, score_case):
    hs, Ts, single = score_case["handles"], score_case["Ts"], score_case["single"]
    got = gorio.ndt.calculate_score_batch(hs, Ts)
    assert np.array_equal(_bits(got), _bits(single))
    rev = gorio.ndt.calculate_score_batch(hs[::-1], Ts[::-1])
    assert np.array_equal(_bits(rev), _bits(single[::-1]))
    eye = np.eye(4, dtype=F)
    ident = np.array([h.calculate_score(eye) for h in hs])
    assert np.array_equal(_bits(gorio.ndt.calculate_score_batch(hs)), _bits(ident))  # T = NULL
    assert np.array_equal(_bits(gorio.ndt.calculate_score_batch(hs, [eye] * len(hs))), _bits(ident))
    assert np.array_equal(_bits(gorio.ndt.calculate_score_batch(hs[3:4], Ts[3:4])), _bits(single[3:4]))  # a batch of one
    # a handle twice
    with pytest.raises(gorio.GorioError) as e:
        gorio.ndt.calculate_score_batch([hs[0], hs[1], hs[0]], Ts[:3])
    assert e.value.code == -1 and "handle 2" in str(e.value)
    # a handle without a source: its error, its index; the others keep their state
    bare = gorio.Ndt(device=gpu, **NDT_KW)
    bare.set_target_shared(hs[0])
    with pytest.raises(gorio.GorioError) as e:
        gorio.ndt.calculate_score_batch([hs[1], hs[2], bare, hs[3]], [Ts[1], Ts[2], Ts[0], Ts[3]])
    assert e.value.code == -3 and "handle 2" in str(e.value) and "no source" in str(e.value)
    bare.close()
    again = np.array([h.calculate_score(T) for h, T in zip(hs, Ts)])
    assert np.array_equal(_bits(again), _bits(single))
    assert np.array_equal(_bits(gorio.ndt.calculate_score_batch(hs, Ts)), _bits(single))


def test_single_score_still_matches_the_restatement(gpu, gorio, score_case):
    for h, src, T, vm, res, got in zip(score_case["handles"], score_case["sources"], score_case["Ts"], score_case["maps"], score_case["res"], score_case["single"]):
        d1, d2, d3 = R.gauss_constants(res, 0.55)
        ref = R.calculate_score(vm, src, T, R.DIRECT7, d1, d2, d3)
        assert ref != 0.0 and abs(got - ref) <= REL * abs(ref), (len(src), got, ref)
