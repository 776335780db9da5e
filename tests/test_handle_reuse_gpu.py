"""Handles reused across cloud sizes: every device buffer of a handle grows on demand and is kept when a later input fits, so a handle
that has seen a larger cloud, then a smaller one, then a larger one again runs on buffers with slack, stale tails and changed
reallocation moments.  Nothing of that may show in a result: every comparison here is against a FRESH handle given the same inputs, bit
for bit (aligns are deterministic: test_batch_equals_single, test_schedule_optimisations_do_not_change_results)."""
import importlib
import threading

import numpy as np
import pytest

import gicp_scenes as gs
import ground_scenes as grs
import sc_scenes as ss
import ugpm_shape_cases as ugpm_cases
from test_prep_gpu import _radar_targets
from test_ugpm_shapes_gpu import _DIAG, ERR_UNSUPPORTED, _batch, _records

synth = importlib.import_module("go-rio_amd.synth")

pytestmark = pytest.mark.gpu

KW = dict(corr_dist_threshold=2.0, transformation_epsilon=0.05, keep_knn_indices=1)
# (source, target) sizes in order: baseline; every group grows (sort keys 4096 -> 8192); shrink inside the kept capacity; larger than
# step 2 but inside its 1/8 slack; regrow (keys -> 16384)
STEPS = [(600, 700), (5000, 4600), (600, 700), (5300, 4600), (9000, 9000)]


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def _register(g, sx, sl, tx, tl):
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    g.calculateCovariances()
    out = dict(cov_s=g.getSourceCovariances(), cov_t=g.getTargetCovariances(), knn_s=g.getKnnIndices(0), knn_t=g.getKnnIndices(1))
    r = g.align()
    out["corr"], out["sqd"] = g.getCorrespondences()
    out["fitness"] = g.getFitnessScore()
    out.update(r)
    return out


@pytest.mark.parametrize("search", [0, 1])
def test_registration_handle_across_sizes(gpu, gorio, search):
    g = gorio.ApdGicp(search=search, **KW)
    for step, (n, m) in enumerate(STEPS):
        pair = gs.c1_pair(n, m)[:4]
        got = _register(g, *pair)
        ref = _register(gorio.ApdGicp(search=search, **KW), *pair)
        assert got["cov_s"].shape[0] == n and got["knn_t"].shape[0] == m and got["n_linearize"] >= 2
        for key in ref:
            assert _same(got[key], ref[key]), (step, n, m, key)


def _register_voxelised(g, sx, sl, tx, tl):
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    g.calculateCovariances()  # the map is accumulated from estimated covariances, not from injected identities
    vm = g.getVoxelMap()
    r = g.align()
    return dict(vm, T=r["T"], H=r["H"], n_linearize=r["n_linearize"], slots=g.getVoxelCorrespondences())


def test_voxelised_handle_across_sizes(gpu, gorio):
    def new():
        g = gorio.ApdGicp(search=1, **KW)
        g.set_method(gorio.apd.METHOD_VGICP, 1.0)
        return g

    g = new()
    for step in (0, 1, 2, 4):
        n, m = STEPS[step]
        pair = gs.c1_pair(n, m)[:4]
        got, ref = _register_voxelised(g, *pair), _register_voxelised(new(), *pair)
        assert len(got["num_points"]) > 50 and got["n_linearize"] >= 2
        for key in ref:
            assert _same(got[key], ref[key]), (step, n, m, key)


def test_batch_descriptors_grow_with_the_lead_handle(gpu, gorio):
    objs = [gorio.ApdGicp(**KW) for _ in range(5)]
    for rnd, count in enumerate((2, 5, 3)):
        pairs = [synth.scan_pair(1500 - 41 * q, 1500 + 53 * q, seed=800 + 10 * rnd + q)[:4] for q in range(count)]
        for o, (sx, sl, tx, tl) in zip(objs, pairs):
            o.setInputTarget(tx, tl)
            o.setInputSource(sx, sl)
        batch = gorio.align_batch(objs[:count])  # objs[0] leads every batch: its descriptor arrays hold 2, then 5, then 3 pairs
        for q, (sx, sl, tx, tl) in enumerate(pairs):
            f = gorio.ApdGicp(**KW)
            f.setInputTarget(tx, tl)
            f.setInputSource(sx, sl)
            assert _same(batch[q], f.align()), (rnd, q)


def test_shared_target_survives_the_owners_regrowth(gpu, gorio):
    sa, sla, t_old, tl_old, _ = synth.scan_pair(2500, 3000, seed=821)
    sb, slb = synth.radar_scan(2800, seed=822)
    _, _, t_new, tl_new, _ = synth.scan_pair(64, 6000, seed=823)

    def fresh(sx, sl, tx, tl):
        f = gorio.ApdGicp(**KW)
        f.setInputTarget(tx, tl)
        f.setInputSource(sx, sl)
        return f.align()

    a, b = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    a.setInputTarget(t_old, tl_old)
    a.setInputSource(sa, sla)
    b.setInputTargetShared(a)
    b.setInputSource(sb, slb)
    assert _same(a.align(), fresh(sa, sla, t_old, tl_old))
    a.setInputTarget(t_new, tl_new)  # the owner detaches (a new, larger cloud of its own); b keeps the old one alive
    assert _same(b.align(), fresh(sb, slb, t_old, tl_old))
    assert _same(a.align(), fresh(sa, sla, t_new, tl_new))
    assert _same(b.align(), fresh(sb, slb, t_old, tl_old))


def _in_thread(fn):
    """fn() on a thread of its own: the preprocessing contexts are thread_local, so a new thread starts with fresh ones."""
    box = {}

    def run():
        try:
            box["out"] = fn()
        except BaseException as e:  # noqa: BLE001 -- re-raised on the caller's thread
            box["err"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "err" in box:
        raise box["err"]
    return box["out"]


def test_prep_context_across_sizes(gpu, gorio):
    prep = gorio.prep
    clouds = [synth.radar_scan(n, seed=synth.BASE_SEED + 62 + k)[0] for k, n in enumerate((800, 6000, 800))]
    calls = [lambda x: prep.radius_outlier_mask(x, 2.0, 2), lambda x: prep.statistical_outlier_mask(x, 20, 1.0, return_distances=True),
             lambda x: prep.dbscan_labels(x), lambda x: prep.voxel_downsample(x, 0.1)]
    reused = _in_thread(lambda: [[c(x) for c in calls] for x in clouds])  # one context through all three sizes
    for k, x in enumerate(clouds):
        assert reused[k][0].sum() > 0 and reused[k][3].shape[0] < len(x)
        for j, c in enumerate(calls):
            assert _same(reused[k][j], _in_thread(lambda: c(x))), (k, j)


def test_ego_velocity_context_across_sizes(gpu, gorio):
    prep = gorio.prep
    cfg = prep.reve_default_config()
    cases = []
    for k, n in enumerate((300, 4000, 300)):
        t, rng = _radar_targets(20 + k, n=n, movers=n // 20)
        nv = _in_thread(lambda: prep.ego_velocity(t, [], cfg))["n_valid"]
        cases.append((t, rng.integers(0, nv, (3, 5)).astype(np.uint32)))
    reused = _in_thread(lambda: [prep.ego_velocity(t, s, cfg) for t, s in cases])
    for k, (t, s) in enumerate(cases):
        assert reused[k]["success"] and reused[k]["inlier"].sum() > 0
        assert _same(reused[k], _in_thread(lambda: prep.ego_velocity(t, s, cfg))), k


def _ugpm_window(S, seed):
    return dict(name=f"S{S}_{seed}", win=synth.window_for_states(S, seed=seed), kw={}, S=S)


def _ugpm_lpm(seed):
    w = synth.imu_window(seed=seed, duration=1.0, vel_hz=20.0)
    return dict(name=f"lpm_{seed}", win=w, kw=dict(type=ugpm_cases.LPM, infer_t=[w["start_t"] + 0.4, w["end_t"]]), S=None)


def _ugpm_run(gorio, cs):
    """One batch call on this thread's context: (raw records, diagnostics, error code)."""
    b, code = _batch(gorio, cs), 0
    try:
        b.run()
    except gorio.GorioError as e:
        code = e.code
    return b.out.copy(), b.diagnostics(), code, b


def test_ugpm_context_across_batches(gpu, gorio):
    """One thread's UGPM context through five batches: small; every buffer grows and the LPM buffers appear; one window inside the kept
    capacities with stale tails behind it; a refused window between two valid ones; the window arrays grow again.  Each batch equals the
    same batch on a fresh thread (a fresh context, no iteration budget from an earlier batch) bit for bit, as
    test_mixed_batch_equals_single_windows relies on batch = single."""
    w = synth.imu_window(seed=7102, duration=2.0)
    chunked = dict(name="chunked", win=w, kw=dict(quantum=0.7123, infer_t=[w["start_t"] + 0.6, w["start_t"] + 1.3, w["end_t"]]), S=None)
    batches = [
        [_ugpm_window(21, 7001), _ugpm_window(21, 7002)],
        [_ugpm_window(17, 7011), _ugpm_window(21, 7012), _ugpm_window(66, 7013), _ugpm_lpm(7014), _ugpm_window(17, 7015), chunked, _ugpm_window(66, 7016),
         _ugpm_lpm(7017), _ugpm_window(21, 7018)],
        [_ugpm_window(21, 7021)],
        [_ugpm_window(66, 7031), _ugpm_window(161, 7032), _ugpm_window(21, 7033)],
        [_ugpm_window((17, 21, 33, 40, 41, 66)[k % 6], 7040 + k) for k in range(16)] + [_ugpm_lpm(7060)],
    ]
    reused = _in_thread(lambda: [_ugpm_run(gorio, cs)[:3] for cs in batches])
    for step, cs in enumerate(batches):
        out, diag, code = reused[step]
        ref_out, ref_diag, ref_code, b = _in_thread(lambda: _ugpm_run(gorio, cs))
        assert code == ref_code == (ERR_UNSUPPORTED if step == 3 else 0), step
        for k, c in enumerate(cs):
            refused = step == 3 and k == 1
            assert diag[k]["status"] == (ERR_UNSUPPORTED if refused else 0), (step, k)
            assert [diag[k][q] for q in _DIAG + ("status",)] == [ref_diag[k][q] for q in _DIAG + ("status",)], (step, c["name"])
            o = sum(b.counts[:k])
            got, ref = out[o:o + b.counts[k]], ref_out[o:o + b.counts[k]]
            assert len(got) == len(c["kw"].get("infer_t", [0]))
            if refused:
                assert np.isnan(got).all() and np.isnan(ref).all()
            else:
                assert np.isfinite(got[:, :14]).all() and np.array_equal(got, ref), (step, c["name"])
            if c["S"] is not None and not refused:
                assert diag[k]["nb_state"] == c["S"] and diag[k]["iters_rot"] > 0 and diag[k]["iters_vel"] > 0


def test_scan_context_handle_across_database_growth(gpu, gorio):
    scans, _ = ss.loop_sequence(n_lap=39, seed=13, n_points=600)  # 78 keyframes, two laps
    sc = gorio.ScanContext()
    asked = []  # detect calls so far: they advance the tree-making counter and the snapshot, host state a fresh handle has to share
    done = 0
    for count in (3, 70, 5):  # crosses the 64-scan floor of the database and regrows the scratch buffers; then a small addition
        sc.add_scans(scans[done : done + count])
        done += count
        fresh = gorio.ScanContext()
        fresh.add_scans(scans[:done])
        for q, cand in asked:
            fresh.detect(q, cand)
        q, cand = done - 1, np.arange(done - 1, dtype=np.int32)
        got = sc.detect(q, cand)
        assert _same(got, fresh.detect(q, cand)), done
        assert got[3]["early_return"] == (done == 3)  # beyond the first three scans the query really searches the database
        asked.append((q, cand))
        assert _same(sc.state(), fresh.state())
        for i in (0, done // 2, done - 1):
            assert _same(sc.descriptor(i), fresh.descriptor(i)), (done, i)
            assert _same(sc.distance(i, done - 1 - i), fresh.distance(i, done - 1 - i)), (done, i)


def test_ground_handle_across_sizes(gpu, gorio):
    frames = [grs.scan(40 + k, n_ground=ng) for k, ng in enumerate((400, 18400, 400))]  # about 2000, 20000 and 2000 points
    assert len(frames[0][0]) < 2500 and len(frames[1][0]) > 19000
    seg = gorio.ground.GroundSegmenter()
    for k, (xyz, inten) in enumerate(frames):
        got = seg.estimate(xyz, inten)
        fresh = gorio.ground.GroundSegmenter()  # a fresh handle that has seen the same frames: its adaptive state matches
        for fx, fi in frames[:k]:
            fresh.estimate(fx, fi)
        ref = fresh.estimate(xyz, inten)
        assert len(got[0]) > 100 and _same(got, ref), k
        assert _same(seg.get_state(), fresh.get_state()), k
        assert _same(seg.diagnostics(), fresh.diagnostics()), k
