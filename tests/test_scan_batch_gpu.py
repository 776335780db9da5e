"""The batched scan pipeline (include/gorio_scan_batch.h) against a twin set of single handles driven by gorio_scan_load / gorio_scan_run
(existing code, pinned against the restated callback by tests/test_scan_pipeline_gpu.py): every member bit for bit its single call's."""
import ctypes as C
import importlib

import numpy as np
import pytest

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


def _handle_error(pipe):
    pipe.lib.gorio_scan_handle_error.restype = C.c_char_p
    return pipe.lib.gorio_scan_handle_error(pipe.h).decode()


def _twin_frame(twin, raw, samples, ang_vel):
    """One frame through the single calls: (n_gated, n_valid, result dict with code and error as scan_run_batch reports them)."""
    gorio_error = importlib.import_module("go-rio_amd").GorioError
    ng, nv = twin.load(raw)
    code = 0
    try:
        twin.run(samples, ang_vel)
    except gorio_error as e:
        code = e.code
    return ng, nv, dict(twin.last_result, code=code, error=_handle_error(twin))


def _same_result(got, want):
    assert set(got) == set(want)
    for k in want:
        if k in ("v_r", "sigma_v_r"):
            assert np.asarray(got[k], np.float64).tobytes() == np.asarray(want[k], np.float64).tobytes(), k
        else:
            assert got[k] == want[k], (k, got[k], want[k])


def _same_readable(pipe, twin):
    """counters, every stage's indices and point bits, and the six output columns of an OK frame"""
    assert pipe.counters() == twin.counters()
    for name in sr.STAGES:
        idx, xyz = pipe.stage(name, points=True)
        tidx, txyz = twin.stage(name, points=True)
        assert np.array_equal(idx, tidx), name
        assert np.array_equal(_bits(xyz), _bits(txyz)), name
    if twin.last_result["status"] == "ok":
        a, b = pipe.output(), twin.output()
        for q in range(4):
            assert np.array_equal(_bits(a[q]), _bits(b[q])), q
    assert pipe.counters() == twin.counters()


def _batch_frame(gorio, pipes, twins, raws, samples, ang_vels):
    """One frame through the batch calls and through the twins; everything compared.  Returns the twins' results."""
    want = [_twin_frame(t, r, s, w) for t, r, s, w in zip(twins, raws, samples, ang_vels)]
    ng, nv = gorio.prep.scan_load_batch(pipes, raws)
    assert ng.tolist() == [w[0] for w in want] and nv.tolist() == [w[1] for w in want]
    got = gorio.prep.scan_run_batch(pipes, samples, ang_vels)
    for i, (p, t) in enumerate(zip(pipes, twins)):
        _same_result(got[i], want[i][2])
        assert p.last_result is got[i] and _handle_error(p) == want[i][2]["error"]
        _same_readable(p, t)
    return [w[2] for w in want]


@pytest.fixture(scope="module")
def sequence(oracle_apd):
    """the five sequence scans (about 3 k points each): (raw, params, samples)"""
    return [sr.chain_inputs(seed, False, sr.OUTLIER_STATISTICAL, oracle_apd, n_ground=sr.SEQUENCE_N_GROUND) for seed in sr.SEQUENCE_SEEDS]


@pytest.fixture(scope="module")
def chains(oracle_apd):
    return {case: sr.chain_inputs(*case, oracle_apd) for case in (sr.CHAIN_CASES[0], sr.CHAIN_CASES[3])}


def _drawn_samples(gorio, p, raw, seed):
    """three RANSAC samples drawn, as chain_inputs draws them, from the count of valid targets (read from a load of its own)"""
    probe = gorio.prep.ScanPipeline(_params(gorio, p))
    nv = probe.load(raw)[1]
    probe.close()
    return np.random.default_rng(seed).integers(0, nv, (3, 5)).astype(U)


def _close(pipes):
    for p in pipes:
        p.close()


# ---- 1. five members, two frames: the second frame starts from each handle's own Patchwork++ state
def test_five_members_two_frames_match_their_twins(gpu, gorio, sequence):
    pipes = [gorio.prep.ScanPipeline(_params(gorio, p)) for _, p, _ in sequence]
    twins = [gorio.prep.ScanPipeline(_params(gorio, p)) for _, p, _ in sequence]
    for shift in (0, 2):  # the second frame in rotated order: handle i gets scan i + 2
        order = [(i + shift) % 5 for i in range(5)]
        res = _batch_frame(gorio, pipes, twins, [sequence[j][0] for j in order], [sequence[j][2] for j in order], [sr.CHAIN_ANG_VEL] * 5)
        for r in res:  # the precondition, on the twins
            assert r["status"] == "ok" and r["n_clusters"] >= 1 and r["n_ground"] > 0
    d = gorio.prep.scan_batch_diag(pipes[0])
    assert d["rounds"] > 0 and d["launches"] > 0 and d["synchronisations"] > 0
    assert gorio.prep.scan_batch_diag(pipes[1]) == dict(rounds=0, launches=0, synchronisations=0)  # the tables live in the lead alone
    _close(pipes + twins)


# ---- 2. the mixed batch: every configuration and every way to end early in one call, then recovery
def test_mixed_batch_matches_twins_and_recovers(gpu, gorio, sequence, chains):
    raw_s, p_s, smp_s = chains[sr.CHAIN_CASES[0]]   # OK with STATISTICAL
    raw_r, p_r, smp_r = chains[sr.CHAIN_CASES[3]]   # OK with RADIUS and dynamic-object removal
    dor = sr.default_params(enable_dynamic_object_removal=True)
    still = sr.raw_scan(5, n_ground=1500, v_true=(0, 0, 0), noise=0.01, movers=20, junk=0)
    two = sr.raw_scan(6, n_ground=1500, junk=0)[:2]
    few = raw_s[np.isfinite(raw_s).all(1) & (raw_s[:, 3] > 0)][:p_s.mean_k]
    seq = sequence
    members = [  # (params, raw, samples or None = drawn from the twin's n_valid, ang_vel)
        (p_s, raw_s, smp_s, sr.CHAIN_ANG_VEL),
        (p_r, raw_r, smp_r, sr.CHAIN_ANG_VEL),
        (sr.default_params(rotation=sr.tilt(), outlier_method=sr.OUTLIER_NONE, ground=False), seq[0][0], seq[0][2], sr.CHAIN_ANG_VEL),
        (sr.default_params(rotation=sr.tilt(), deskew=False), seq[1][0], seq[1][2], sr.CHAIN_ANG_VEL),
        (seq[2][1], seq[2][0], seq[2][2], None),
        (dor, still, None, None),
        (dor, two, [], None),
        (p_s, few, [], None),
        (sr.default_params(), np.zeros((0, 5), F), [], sr.CHAIN_ANG_VEL),
    ]
    pipes = [gorio.prep.ScanPipeline(_params(gorio, m[0])) for m in members]
    twins = [gorio.prep.ScanPipeline(_params(gorio, m[0])) for m in members]
    samples = [m[2] if m[2] is not None else _drawn_samples(gorio, m[0], m[1], 5) for m in members]
    res = _batch_frame(gorio, pipes, twins, [m[1] for m in members], samples, [m[3] for m in members])
    assert [r["status"] for r in res] == ["ok"] * 5 + ["zero_velocity", "empty", "refused", "empty"]
    assert [r["stage"] for r in res[5:]] == [-1, sr.STAGES.index("dynamic"), sr.STAGES.index("outlier"), sr.STAGES.index("gate")]
    assert [r["code"] for r in res] == [0] * 7 + [-1, 0] and "fewer points than mean_k + 1" in res[7]["error"]
    assert all(r["error"] == "" for i, r in enumerate(res) if i != 7)
    with pytest.raises(gorio.GorioError) as e:  # every run consumed its load, the refused member's too
        gorio.prep.scan_run_batch(pipes, samples, [m[3] for m in members])
    assert e.value.code == -3 and "handles[0]" in str(e.value)
    # fresh OK scans through the same handles, in the handles' own configurations: the early members recover, and the refused member's
    # Patchwork++ state was untouched (its twin's never ran either: equal bits here say so)
    level = sr.raw_scan(120, n_ground=sr.SEQUENCE_N_GROUND)  # for the members whose rotation is the identity
    lv = (level, _drawn_samples(gorio, dor, level, 120))
    fresh = [(raw_s, smp_s), (raw_r, smp_r), (seq[3][0], seq[3][2]), (seq[4][0], seq[4][2]), (seq[0][0], seq[0][2]), lv, lv, (raw_s, smp_s), lv]
    res = _batch_frame(gorio, pipes, twins, [f[0] for f in fresh], [f[1] for f in fresh], [sr.CHAIN_ANG_VEL] * len(fresh))
    assert all(r["status"] == "ok" for r in res), [r["status"] for r in res]
    first = gorio.prep.ScanPipeline(_params(gorio, p_s))  # a handle that never saw the refused frame gives the same frame
    _, _, r0 = _twin_frame(first, raw_s, smp_s, sr.CHAIN_ANG_VEL)
    _same_result(pipes[7].last_result, r0)
    assert np.array_equal(_bits(pipes[7].output()[0]), _bits(first.output()[0]))
    _close(pipes + twins + [first])


# ---- 3. block boundaries of the compaction, load only
def _random_raw(n, seed):
    rng = np.random.default_rng(seed)
    raw = np.zeros((n, 5), F)
    raw[:, :3] = rng.uniform(-50, 50, (n, 3))
    raw[:, 3] = rng.random(n) < 0.4
    raw[:, 4] = 1.0
    return raw


@pytest.mark.parametrize("sizes", [(1, 255, 256, 257, 511, 512, 513), (100000, 100000, 70000)], ids=["block-edges", "count-scan-second-trip"])
def test_load_batch_at_block_boundaries(gpu, gorio, sizes):
    """(100000, 100000, 70000): 391 + 391 + 274 = 1056 workgroup counts, past the 1024 of one trip of the count scan"""
    if len(sizes) == 3:
        assert sum((n + 255) // 256 for n in sizes) > 1024
    raws = [_random_raw(n, 300 + i) for i, n in enumerate(sizes)]
    pipes = [gorio.prep.ScanPipeline(gorio.prep.scan_default_params()) for _ in sizes]
    twins = [gorio.prep.ScanPipeline(gorio.prep.scan_default_params()) for _ in sizes]
    want = [t.load(r) for t, r in zip(twins, raws)]
    ng, nv = gorio.prep.scan_load_batch(pipes, raws)
    assert ng.tolist() == [w[0] for w in want] and nv.tolist() == [w[1] for w in want]
    for p, t, r in zip(pipes, twins, raws):
        idx, xyz = p.stage("gate", points=True)
        tidx, txyz = t.stage("gate", points=True)
        assert np.array_equal(idx, tidx) and np.array_equal(_bits(xyz), _bits(txyz))
        assert np.array_equal(idx, np.flatnonzero(r[:, 3] > 0))  # and the twin is right
    _close(pipes + twins)


# ---- 4. the hand-offs after a batch run
def test_hand_off_after_a_batch_run(gpu, gorio, sequence):
    kw = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)
    raw, p, samples = sequence[0]
    raw_b = raw.copy()  # the next frame: the same message seen from a slightly turned sensor
    with np.errstate(invalid="ignore"):  # the message's NaN / Inf points stay what they are
        raw_b[:, :3] = (raw[:, :3].astype(np.float64) @ sr.tilt(0.01, 0.0).T + np.array([0.2, -0.1, 0.0])).astype(F)
    sel = [(raw, p, samples), (raw_b, p, samples)]
    pipes = [gorio.prep.ScanPipeline(_params(gorio, p)) for _, p, _ in sel]
    twins = [gorio.prep.ScanPipeline(_params(gorio, p)) for _, p, _ in sel]
    gorio.prep.scan_load_batch(pipes, [s[0] for s in sel])
    res = gorio.prep.scan_run_batch(pipes, [s[2] for s in sel], [sr.CHAIN_ANG_VEL] * 2)
    assert all(r["status"] == "ok" for r in res)
    for t, s in zip(twins, sel):
        t.load(s[0])
        t.run(s[2], sr.CHAIN_ANG_VEL)
    for p in pipes:
        assert p.counters() == dict(point_uploads=1, index_builds=2, point_downloads=0)
    g1, g2 = gorio.ApdGicp(**kw), gorio.ApdGicp(**kw)
    g1.setInputTargetFromScan(pipes[0])
    g1.setInputSourceFromScan(pipes[1])
    g2.setInputTargetFromScan(twins[0])
    g2.setInputSourceFromScan(twins[1])
    r1, r2 = g1.align(), g2.align()
    assert np.array_equal(_bits(r1["T"]), _bits(r2["T"])) and r1["nr_iterations"] == r2["nr_iterations"] and r1["converged"] == r2["converged"]
    assert r1["nr_iterations"] >= 1
    for p in pipes:
        assert p.counters() == dict(point_uploads=1, index_builds=2, point_downloads=0)  # the hand-off built and moved nothing
    store = gorio.keyframes.KeyframeStore()
    kid = store.add_from_scan(pipes[1])
    assert kid >= 0
    _close(pipes + twins)


# ---- 5. the shape of a call does not depend on the count; a batch of one is the single call
def test_shape_of_the_call_is_independent_of_the_count(gpu, gorio, sequence):
    diags = {}
    for count in (2, 5):
        sel = sequence[:count]
        pipes = [gorio.prep.ScanPipeline(_params(gorio, p)) for _, p, _ in sel]
        gorio.prep.scan_load_batch(pipes, [s[0] for s in sel])
        load_diag = gorio.prep.scan_batch_diag(pipes[0])
        res = gorio.prep.scan_run_batch(pipes, [s[2] for s in sel], [sr.CHAIN_ANG_VEL] * count)
        assert all(r["status"] == "ok" and r["n_clusters"] >= 1 for r in res)
        diags[count] = (load_diag, gorio.prep.scan_batch_diag(pipes[0]))
        _close(pipes)
    assert diags[2] == diags[5], diags
    assert diags[2][0]["synchronisations"] == 2 and diags[2][1]["synchronisations"] >= 8


def test_batch_of_one_gives_the_twins_bits(gpu, gorio, sequence):
    raw, p, samples = sequence[0]
    pipe, twin = gorio.prep.ScanPipeline(_params(gorio, p)), gorio.prep.ScanPipeline(_params(gorio, p))
    res = _batch_frame(gorio, [pipe], [twin], [raw], [samples], [sr.CHAIN_ANG_VEL])
    assert res[0]["status"] == "ok"
    # single and batched calls alternate on one handle
    ng, nv, want = _twin_frame(twin, sequence[1][0], sequence[1][2], sr.CHAIN_ANG_VEL)
    assert pipe.load(sequence[1][0]) == (ng, nv)
    pipe.run(sequence[1][2], sr.CHAIN_ANG_VEL)
    _same_readable(pipe, twin)
    _close([pipe, twin])
