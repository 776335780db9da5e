"""The device-resident scan pipeline (include/gorio_scan.h) against the restated callback (tests/scan_pipeline_restatement.py): every stage's
survivors and coordinates bit for bit, the whole callback, its outcomes, a sequence through one handle, the hand-off to the registration
and the residency counters."""
import numpy as np
import pytest

import patchwork_restatement as pr
import scan_pipeline_restatement as sr

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _params(gorio, p):
    kw = {k: getattr(p, k) for k in ("power_threshold", "rotation", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul",
                                     "radius", "min_neighbors", "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size")}
    kw.update(enable_dynamic_object_removal=int(p.enable_dynamic_object_removal), deskew=int(p.deskew), ground=int(p.ground))
    sp = gorio.prep.scan_default_params(**kw)
    for k, v in p.reve.items():
        setattr(sp.reve, k, v)
    return sp


def _compare(pipe, got, ref, n_gated):
    """status, every stage the restatement reached (indices and coordinates, exact), and for an OK frame the published cloud."""
    assert got["status"] == ref["status"] and n_gated == ref["n_gated"]
    if ref["status"] in ("empty", "refused"):
        assert got["stage"] == ref["stage"]
    assert got["reve_success"] == ref["reve_success"]
    assert np.allclose(got["v_r"], ref["v_r"], rtol=1e-10, atol=1e-12) and np.allclose(got["sigma_v_r"], ref["sigma_v_r"], rtol=1e-9, atol=1e-14)
    for name in sr.STAGES:
        idx, xyz = pipe.stage(name, points=True)
        if name in ref["stages"]:
            ridx, rxyz = ref["stages"][name]
            assert np.array_equal(idx, ridx), name
            assert np.array_equal(_bits(xyz), _bits(rxyz)), name
        else:
            assert len(idx) == 0, name
    if ref["status"] == "ok":
        assert (got["n_out"], got["n_ground"], got["n_clusters"]) == (ref["n_out"], ref["n_ground"], ref["n_clusters"])
        xyz, inten, dop, lab = pipe.output()
        assert np.array_equal(_bits(xyz), _bits(ref["xyz"])) and np.array_equal(_bits(inten), _bits(ref["intensity"])) and np.array_equal(_bits(dop), _bits(ref["doppler"]))
        assert np.array_equal(lab, ref["label"])


def _frame(pipe, raw, p, samples, ang_vel, oracle_apd, patchwork=None):
    ref = sr.callback(raw, p, samples, ang_vel, oracle_apd, patchwork)
    n_gated, n_valid = pipe.load(raw)
    if "n_valid" in ref:
        assert n_valid == ref["n_valid"]
    got = pipe.run(samples, ang_vel)
    _compare(pipe, got, ref, n_gated)
    return got, ref


# ---- stages at the wave (64) and workgroup (256) boundaries of the compaction; 4097 points are 17 workgroup counts, one trip of the scan of
# the counts (1024 per trip).  test_compaction_scans_more_than_1024_workgroup_counts below goes past one trip.
def _stage_raw(n, mask, seed):
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-8, 25, n)], 1)
    r = np.linalg.norm(xyz, axis=1, keepdims=True)
    dop = -(xyz / r) @ np.array([4.0, 0.5, 0.0]) + rng.normal(0, 0.05, n)
    power = {"all": np.ones(n), "none": np.zeros(n), "alternating": (np.arange(n) % 2).astype(float), "last": (np.arange(n) == n - 1).astype(float)}[mask]
    return np.concatenate([xyz, power[:, None], dop[:, None]], 1).astype(F)


@pytest.mark.parametrize("mask", ["all", "none", "alternating", "last"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_stages_match_the_restatement_bit_for_bit(gpu, gorio, oracle_apd, n, mask):
    raw = _stage_raw(n, mask, 1000 + n)
    p = sr.default_params(rotation=sr.tilt(0.4, -0.03), distance_far=50.0, outlier_method=sr.OUTLIER_NONE, ground=False, reve=dict(use_ransac=0))
    pipe = gorio.prep.ScanPipeline(_params(gorio, p))
    got, ref = _frame(pipe, raw, p, [], (0.02, -0.01, 0.3), oracle_apd)
    kept = {"all": n, "none": 0, "alternating": n // 2, "last": 1}[mask]
    assert len(ref["stages"]["gate"][0]) == kept
    if kept >= 2000:  # the distance filter's own mask is a fourth pattern: it must have dropped and kept points
        assert 0 < len(ref["stages"]["distance"][0]) < kept and ref["status"] == "ok"
        assert not np.array_equal(_bits(ref["stages"]["deskew"][1]), _bits(ref["stages"]["dynamic"][1]))
    pipe.close()


def test_compaction_scans_more_than_1024_workgroup_counts(gpu, gorio):
    """More than 1024 x 256 points: the single-workgroup scan of the workgroup counts makes a second trip and carries the first trip's total.
    The gate alone (no other stage needs this size): survivors and their order against NumPy."""
    n = 1024 * 256 + 1000  # 1028 workgroup counts: trips of 1024 and 4
    rng = np.random.default_rng(77)
    raw = np.zeros((n, 5), F)
    raw[:, :3] = rng.uniform(-50, 50, (n, 3))
    raw[:, 3] = rng.random(n) < 0.4
    raw[-1, 3] = 1.0  # the last point of the last workgroup of the second trip
    raw[:, 4] = 1.0
    pipe = gorio.prep.ScanPipeline(gorio.prep.scan_default_params())
    n_gated, _ = pipe.load(raw)
    want = np.flatnonzero(raw[:, 3] > 0)
    assert n_gated == len(want) and want[-1] == n - 1 and (want >= 1024 * 256).sum() > 100
    idx, xyz = pipe.stage("gate", points=True)
    assert np.array_equal(idx, want) and np.array_equal(_bits(xyz), _bits(raw[want, :3]))  # identity rotation: the coordinates pass unchanged
    pipe.close()


# ---- the whole callback
@pytest.fixture(scope="module")
def chain_refs(oracle_apd):
    out = {}
    for seed, dor, method in sr.CHAIN_CASES:
        raw, p, samples = sr.chain_inputs(seed, dor, method, oracle_apd)
        out[(seed, dor, method)] = (raw, p, samples, sr.callback(raw, p, samples, sr.CHAIN_ANG_VEL, oracle_apd, pr.Patchworkpp()))
    return out


@pytest.mark.parametrize("case", sr.CHAIN_CASES, ids=lambda c: "seed%d-dor%d-outlier%d" % (c[0], c[1], c[2]))
def test_whole_callback_matches_the_restated_chain(gpu, gorio, chain_refs, case):
    raw, p, samples, ref = chain_refs[case]
    assert ref["status"] == "ok" and ref["margin"] > 1e-4  # Patchwork++ sits clear of its thresholds: a difference below is a bug, not a near-tie
    pipe = gorio.prep.ScanPipeline(_params(gorio, p))
    n_gated, n_valid = pipe.load(raw)
    assert n_valid == ref["n_valid"] and n_gated < len(raw)
    got = pipe.run(samples, sr.CHAIN_ANG_VEL)
    _compare(pipe, got, ref, n_gated)
    assert got["n_clusters"] >= 1 and pipe.output()[3].max() == got["n_clusters"]
    c = pipe.counters()
    assert c["point_uploads"] == 1 and c["index_builds"] == 2  # the outlier stage and DBSCAN
    pipe.close()


# ---- outcomes
def test_outcomes_skip_empty_refusal_and_recovery(gpu, gorio, oracle_apd, chain_refs):
    p = sr.default_params(enable_dynamic_object_removal=True)
    pipe = gorio.prep.ScanPipeline(_params(gorio, p))
    still = sr.raw_scan(5, n_ground=1500, v_true=(0, 0, 0), noise=0.01, movers=20, junk=0)
    nv = sr.callback(still, p, np.zeros((0, 5), U), None, oracle_apd, pr.Patchworkpp())["n_valid"]
    samples = np.random.default_rng(5).integers(0, nv, (3, 5)).astype(U)
    got, ref = _frame(pipe, still, p, samples, None, oracle_apd, pr.Patchworkpp())
    assert got["status"] == "zero_velocity" and got["reve_success"] and np.all(got["v_r"] == 0)
    two = sr.raw_scan(6, n_ground=1500, junk=0)[:2]  # two targets: the estimate fails (REVE needs more than 2), its inlier cloud is empty
    got, ref = _frame(pipe, two, p, [], None, oracle_apd, pr.Patchworkpp())
    assert got["status"] == "empty" and got["stage"] == sr.STAGES.index("dynamic") and not got["reve_success"]
    pipe.close()
    # a cloud of mean_k points or fewer: the statistical filter's own refusal, then a clean frame through the same handle
    raw, p, samples, ref = chain_refs[sr.CHAIN_CASES[0]]
    pipe = gorio.prep.ScanPipeline(_params(gorio, p))
    few = raw[np.isfinite(raw).all(1) & (raw[:, 3] > 0)][:p.mean_k]
    assert sr.callback(few, p, [], None, oracle_apd, pr.Patchworkpp())["status"] == "refused"
    pipe.load(few)
    with pytest.raises(gorio.GorioError) as e:
        pipe.run([], None)
    assert "fewer points than mean_k + 1" in str(e.value) and pipe.last_result["status"] == "refused" and pipe.last_result["stage"] == sr.STAGES.index("outlier")
    with pytest.raises(gorio.GorioError):  # the refused run consumed its load
        pipe.run([], None)
    n_gated, _ = pipe.load(raw)
    _compare(pipe, pipe.run(samples, sr.CHAIN_ANG_VEL), ref, n_gated)  # the refused frame never reached Patchwork++: its state is untouched
    pipe.close()


# ---- five scans through one handle: the Patchwork++ state is carried
def test_sequence_through_one_handle_matches_the_restated_chain(gpu, gorio, oracle_apd):
    pw, pipe = pr.Patchworkpp(), None
    states = []
    for seed in sr.SEQUENCE_SEEDS:
        raw, p, samples = sr.chain_inputs(seed, False, sr.OUTLIER_STATISTICAL, oracle_apd, n_ground=sr.SEQUENCE_N_GROUND)
        pipe = pipe or gorio.prep.ScanPipeline(_params(gorio, p))
        got, ref = _frame(pipe, raw, p, samples, sr.CHAIN_ANG_VEL, oracle_apd, pw)
        assert ref["status"] == "ok" and ref["margin"] > 1e-4
        states.append(pw.state()["sensor_height"])
    assert len(set(states)) > 1 or any(len(v) for v in pw.state()["update_elevation"])  # the state did evolve over the sequence
    pipe.close()


# ---- hand-off and residency
def test_hand_off_equals_set_input_and_keeps_the_scan_on_the_device(gpu, gorio, chain_refs):
    raw, p, samples, ref = chain_refs[sr.CHAIN_CASES[0]]
    pipe = gorio.prep.ScanPipeline(_params(gorio, p))
    kw = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)
    g1, g2 = gorio.ApdGicp(**kw), gorio.ApdGicp(**kw)
    pipe.load(raw)
    pipe.run(samples, sr.CHAIN_ANG_VEL)
    g1.setInputTargetFromScan(pipe)
    c = pipe.counters()
    assert c == dict(point_uploads=1, index_builds=2, point_downloads=0)
    tgt = pipe.output()
    # the next frame: the same message seen from a slightly turned sensor
    raw_b = raw.copy()
    with np.errstate(invalid="ignore"):  # the message's NaN / Inf points stay what they are
        raw_b[:, :3] = (raw[:, :3].astype(np.float64) @ sr.tilt(0.01, 0.0).T + np.array([0.2, -0.1, 0.0])).astype(F)
    pipe.load(raw_b)
    rb = pipe.run(samples, sr.CHAIN_ANG_VEL)
    assert rb["status"] == "ok"
    g1.setInputSourceFromScan(pipe)
    c2 = pipe.counters()
    assert c2["point_uploads"] == 2 and c2["index_builds"] == 4 and c2["point_downloads"] == 1  # one upload, two builds per frame; the hand-off builds none
    src = pipe.output()
    assert pipe.counters()["point_downloads"] == 2
    pipe.stage("ground", points=True)
    assert pipe.counters()["point_downloads"] == 3 and pipe.counters()["index_builds"] == 4
    assert np.array_equal(_bits(tgt[0]), _bits(ref["xyz"])) and np.array_equal(tgt[3], ref["label"])  # the handed-over target was not disturbed by the next frame
    g2.setInputTarget(tgt[0], tgt[3])
    g2.setInputSource(src[0], src[3])
    r1, r2 = g1.align(), g2.align()
    assert np.array_equal(_bits(r1["T"]), _bits(r2["T"])) and r1["nr_iterations"] == r2["nr_iterations"] and r1["converged"] == r2["converged"]
    assert r1["n_linearize"] == r2["n_linearize"] and r1["nr_iterations"] >= 1
    for which in (0, 1):
        a, b = g1.debugGetIndex(which), g2.debugGetIndex(which)
        assert a["n"] == b["n"] and a["kd_chunk"] == b["kd_chunk"]
        for k in ("sx", "sy", "sz", "orig", "tbox", "sbox", "bbox"):
            assert np.array_equal(a[k], b[k]), (which, k)
    pipe.close()  # the registration handle keeps the clouds it was handed
    r3 = g1.align()
    assert np.array_equal(_bits(r3["T"]), _bits(r1["T"]))
