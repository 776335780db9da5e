"""The keyframe store (include/gorio_keyframes.h) on the MI355X: a keyframe held on the device must serve every consumer -- registration
source and target, NDT, the scan-to-submap target, the Scan Context database -- with the bits the host entry points give for host copies
of the same cloud.  All comparisons are on bit patterns."""
import importlib

import numpy as np
import pytest

import sc_scenes as ss
import scan_pipeline_restatement as sr

synth = importlib.import_module("go-rio_amd.synth")

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
INVALID, STATE = -1, -3
KW = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)


def _bits(a):
    return np.ascontiguousarray(a, F).view(U)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _same_align(ra, rb):
    assert _same(ra["T"], rb["T"]) and ra["H"].tobytes() == rb["H"].tobytes()
    assert (ra["converged"], ra["nr_iterations"], ra["n_linearize"]) == (rb["converged"], rb["nr_iterations"], rb["n_linearize"])
    assert ra["nr_iterations"] >= 1


def _same_index(a, b, which):
    """debugGetIndex of both handles: equal, or absent on both (FastVGICP searches no target index)."""
    try:
        ia = a.debugGetIndex(which)
    except RuntimeError as e:
        assert e.code == STATE
        with pytest.raises(RuntimeError):
            b.debugGetIndex(which)
        return
    ib = b.debugGetIndex(which)
    assert ia["n"] == ib["n"] and ia["kd_chunk"] == ib["kd_chunk"]
    for k in ("sx", "sy", "sz", "orig", "tbox", "sbox", "bbox"):
        assert np.array_equal(ia[k], ib[k]), (which, k)


@pytest.fixture(scope="module")
def pair():
    sx, sl, tx, tl, _ = synth.scan_pair(2048, 2048, seed=1)
    return sx, sl, tx, tl


# ---------------------------------------------------------------------------------------------------------------- 1. round trip
def _odd_cloud(n, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-50, 50, (n, 3)).astype(F)
    if n:
        xyz[0, 0] = np.nan
        xyz[n - 1, 2] = -np.inf
        xyz[n // 2, 1] = np.inf
    return xyz, rng.uniform(-5, 40, n).astype(F), rng.integers(0, 4, n).astype(F)


@pytest.mark.parametrize("with_columns", [True, False])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 255, 256, 257, 3000])
def test_round_trip_returns_the_input_bits(gpu, gorio, n, with_columns):
    xyz, inten, lab = _odd_cloud(n, 10 + n)
    store = gorio.KeyframeStore()
    kid = store.add(xyz, inten if with_columns else None, lab if with_columns else None)
    assert kid == 0 and store.count() == (1, 1)
    info = store.info(kid)
    assert info == dict(n=n, resident=1, has_intensity=int(with_columns), cov_count=0, cov_k=0, cov_reg=0, index_built=0, sharers=0)  # nothing derived yet
    gx, gi, gl = store.get(kid, intensity=with_columns)
    assert gx.shape == (n, 3) and _same(gx, xyz)
    if with_columns:
        assert _same(gi, inten) and _same(gl, lab)
    else:
        assert gi is None and not gl.any()
        if n:
            with pytest.raises(gorio.GorioError) as e:
                store.get(kid, intensity=True)
            assert e.value.code == STATE
    assert store.counters() == dict(point_uploads=1, point_downloads=1, device_copies=0)
    assert store.add(xyz[: n // 2]) == 1  # ids ascend
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 2. from a scan
def _scan_params(gorio, p):
    kw = {k: getattr(p, k) for k in ("power_threshold", "rotation", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul",
                                     "radius", "min_neighbors", "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size")}
    kw.update(enable_dynamic_object_removal=int(p.enable_dynamic_object_removal), deskew=int(p.deskew), ground=int(p.ground))
    sp = gorio.prep.scan_default_params(**kw)
    for k, v in p.reve.items():
        setattr(sp.reve, k, v)
    return sp


def test_keyframe_from_a_scan_shares_the_pipelines_output(gpu, gorio, oracle_apd):
    raw, p, samples = sr.chain_inputs(*sr.CHAIN_CASES[0], oracle_apd)
    pipe = gorio.prep.ScanPipeline(_scan_params(gorio, p))
    store = gorio.KeyframeStore()
    with pytest.raises(gorio.GorioError) as e:  # no output yet
        store.add_from_scan(pipe)
    assert e.value.code == STATE and store.count() == (0, 0)
    pipe.load(raw)
    assert pipe.run(samples, sr.CHAIN_ANG_VEL)["status"] == "ok"
    c0 = pipe.counters()
    kid = store.add_from_scan(pipe)
    assert pipe.counters() == c0  # no point went up or down, no index was built
    assert store.counters() == dict(point_uploads=0, point_downloads=0, device_copies=1)  # the intensity column
    xyz, inten, _, lab = pipe.output()
    info = store.info(kid)
    assert info["n"] == len(xyz) > 256 and info["has_intensity"] and info["index_built"] and info["sharers"] == 1  # the DBSCAN stage's index; the pipeline's handle

    def undisturbed():
        gx, gi, gl = store.get(kid)
        return _same(gx, xyz) and _same(gi, inten) and _same(gl, lab)

    assert undisturbed()
    raw_b = raw.copy()
    with np.errstate(invalid="ignore"):
        raw_b[:, :3] = (raw[:, :3].astype(np.float64) @ sr.tilt(0.01, 0.0).T + np.array([0.2, -0.1, 0.0])).astype(F)
    pipe.load(raw_b)
    assert pipe.run(samples, sr.CHAIN_ANG_VEL)["status"] == "ok"
    assert not _same(pipe.output()[0][:64], xyz[:64])  # the pipeline did move on
    assert undisturbed() and store.info(kid)["sharers"] == 0
    pipe.close()
    assert undisturbed()
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 3. registration equality
@pytest.mark.parametrize("method", ["apdgicp", "gicp", "vgicp"])
def test_registration_from_keyframes_equals_host_arrays(gpu, gorio, pair, method):
    sx, sl, tx, tl = pair
    apd = importlib.import_module("go-rio_amd.apd")
    store = gorio.KeyframeStore()
    kt, ks = store.add(tx, label=tl), store.add(sx, label=sl)
    a, b = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    for g in (a, b):
        g.set_method(dict(apdgicp=apd.METHOD_APDGICP, gicp=apd.METHOD_GICP, vgicp=apd.METHOD_VGICP)[method], voxel_resolution=1.0)
    a.setInputTarget(tx, tl)
    a.setInputSource(sx, sl)
    b.setInputTargetKeyframe(store, kt)
    b.setInputSourceKeyframe(store, ks)
    assert store.counters() == dict(point_uploads=2, point_downloads=0, device_copies=0) and store.info(ks)["sharers"] == 1
    _same_align(a.align(), b.align())
    for which in (0, 1):
        _same_index(a, b, which)
    assert a.getSourceCovariances().tobytes() == b.getSourceCovariances().tobytes() and a.getTargetCovariances().tobytes() == b.getTargetCovariances().tobytes()
    e = store.add(np.zeros((0, 3), F))
    for fn in (b.setInputSourceKeyframe, b.setInputTargetKeyframe):  # an empty keyframe is refused like n <= 0 in setInputSource
        with pytest.raises(gorio.GorioError) as err:
            fn(store, e)
        assert err.value.code == INVALID
    store.close()


def test_ndt_from_keyframes_equals_host_arrays(gpu, gorio, pair):
    sx, _, tx, _ = pair
    kw = dict(resolution=1.0, search=2)  # DIRECT7
    store = gorio.KeyframeStore()
    kt, ks = store.add(tx), store.add(sx)
    a, b = gorio.Ndt(**kw), gorio.Ndt(**kw)
    a.set_target(tx)
    a.set_source(sx)
    b.set_target_from_keyframe(store, kt)
    b.set_source_from_keyframe(store, ks)
    assert store.counters()["device_copies"] == 2
    ra, rb = a.align(), b.align()
    assert _same(ra["T"], rb["T"]) and ra["nr_iterations"] == rb["nr_iterations"] >= 1
    assert np.float64(ra["trans_probability"]).tobytes() == np.float64(rb["trans_probability"]).tobytes() and ra["converged"] == rb["converged"]
    nan_src = sx.copy()
    nan_src[5, 1] = np.nan
    kn = store.add(nan_src)
    with pytest.raises(gorio.GorioError) as e:  # refused as by set_source_from_scan; the held source stays
        b.set_source_from_keyframe(store, kn)
    assert e.value.code == INVALID and _same(b.align()["T"], ra["T"])
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 4. carry-over
def test_covariances_and_index_carry_over_to_the_next_target(gpu, gorio, pair):
    sx, sl, tx, tl = pair
    n = len(sx)
    store = gorio.KeyframeStore()
    kt, ks = store.add(tx, label=tl), store.add(sx, label=sl)
    a, b = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    a.setInputTarget(tx, tl)
    a.setInputSource(sx, sl)
    b.setInputTargetKeyframe(store, kt)
    b.setInputSourceKeyframe(store, ks)
    assert store.info(ks)["cov_count"] == 0 and not store.info(ks)["index_built"]
    _same_align(a.align(), b.align())
    info = store.info(ks)
    assert info["cov_count"] == n and info["index_built"] and (info["cov_k"], info["cov_reg"]) == (b.params.k_correspondences, b.params.regularization)
    # a fresh handle takes the keyframe as TARGET: its covariances are there at once, and they are those of the align's source
    c, d = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    c.setInputTargetKeyframe(store, ks)
    covs = c.getTargetCovariances()
    assert covs.shape[0] == n and covs.tobytes() == a.getSourceCovariances().tobytes()
    c.setInputSource(tx, tl)
    d.setInputTarget(sx, sl)
    d.setInputSource(tx, tl)
    rd = d.align()
    _same_align(c.align(), rd)
    # another k_correspondences: refused, the handle keeps what it had
    e = gorio.ApdGicp(k_correspondences=10, **KW)
    e.setInputTarget(tx, tl)
    for fn in (e.setInputTargetKeyframe, e.setInputSourceKeyframe):
        with pytest.raises(gorio.GorioError) as err:
            fn(store, ks)
        assert err.value.code == INVALID and "k_correspondences" in str(err.value)
    ex, el = e.getTargetPoints()
    assert _same(ex, tx) and _same(el, tl) and e._n_tgt == n
    # scan_matching_odometry_nodelet.cpp:588: the source of the align that made the keyframe becomes the next scan-to-scan target
    k2 = store.add_from_apd(b, 0)
    assert k2 == 2 and store.info(k2)["cov_count"] == n and store.info(k2)["index_built"] and store.info(k2)["sharers"] >= 2
    f = gorio.ApdGicp(**KW)
    f.setInputTargetKeyframe(store, k2)
    f.setInputSource(tx, tl)
    _same_align(f.align(), rd)
    gx, _, gl = store.get(k2, intensity=False)
    assert _same(gx, sx) and _same(gl, sl)
    with pytest.raises(gorio.GorioError) as err:  # a side without a cloud
        store.add_from_apd(gorio.ApdGicp(**KW), 1)
    assert err.value.code == STATE and store.count() == (3, 3)
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 5. submap
def _submap_frames():
    """Ten frames: sizes at the block (256) boundaries, an empty one, one that is all NaN, one with NaN at its block edges."""
    frames = []
    for k, n in enumerate((0, 1, 255, 256, 257, 3000, 100, 600, 300, 1000)):
        xyz, lab = synth.radar_scan(max(n, 1), seed=700 + k)
        xyz, lab = xyz[:n].copy(), lab[:n].copy()
        if k == 6:
            xyz[:] = np.nan
        if k == 7:
            xyz[[0, 255, 256, n - 1], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
        frames.append((xyz, lab))
    rel = [synth.gt_transform([0.6 * k, 0.05 * k, 0.01 * k], [0.1 * k, -0.05 * k, 1.2 * k]) for k in range(len(frames))]
    return frames, rel


@pytest.fixture(scope="module")
def submap_case(gorio, gpu):
    frames, rel = _submap_frames()
    store = gorio.KeyframeStore()
    ids = [store.add(x, label=l) for x, l in frames]
    yield frames, rel, store, ids
    store.close()


@pytest.mark.parametrize("leaf", [0.0, 0.5])
@pytest.mark.parametrize("count", [1, 10])
def test_submap_from_keyframes_equals_host_assembly_and_oracle(gpu, gorio, oracle_apd, submap_case, count, leaf):
    frames, rel, store, ids = submap_case
    pick = [5] if count == 1 else list(range(10))
    fr, T, kid = [frames[k] for k in pick], [rel[k] for k in pick], [ids[k] for k in pick]
    xo, lo = oracle_apd.submap_assemble(fr, T, leaf)
    a, b = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    na = a.setInputTargetSubmap(fr, T, voxel_leaf=leaf)
    c0 = store.counters()
    nb = b.setInputTargetSubmapKeyframes(store, kid, T, voxel_leaf=leaf)
    assert store.counters() == c0
    assert na == nb == len(xo) and (leaf > 0 or nb == sum(int(np.isfinite(x).all(1).sum()) for x, _ in fr))
    (xa, la), (xb, lb) = a.getTargetPoints(), b.getTargetPoints()
    assert _same(xb, xa) and _same(lb, la) and _same(xb, xo) and _same(lb, lo)


def test_submap_scan_wraps_past_1024_blocks(gpu, gorio, oracle_apd):
    """More than 1024 x 256 points in one call: the single-workgroup scan of the block counts makes a second trip."""
    rng = np.random.default_rng(3)
    frames = []
    for n in (140001, 125000):
        xyz = rng.uniform(-80, 80, (n, 3)).astype(F)
        xyz[rng.random(n) < 0.1, 1] = np.nan
        xyz[n - 1] = 1.0  # the last point of the last block survives
        frames.append((xyz, rng.integers(0, 3, n).astype(F)))
    rel = [synth.gt_transform([0.3, -0.2, 0.1], [1.0, 2.0, -30.0]), np.eye(4)]
    assert sum((len(x) + 255) // 256 for x, _ in frames) > 1024
    store = gorio.KeyframeStore()
    ids = [store.add(x, label=l) for x, l in frames]
    a, b = gorio.ApdGicp(**KW), gorio.ApdGicp(**KW)
    na, nb = a.setInputTargetSubmap(frames, rel), b.setInputTargetSubmapKeyframes(store, ids, rel)
    xo, lo = oracle_apd.submap_assemble(frames, rel, 0.0)
    assert na == nb == len(xo) > 1024 * 256 * 0.85
    (xa, la), (xb, lb) = a.getTargetPoints(), b.getTargetPoints()
    assert _same(xb, xa) and _same(lb, la) and _same(xb, xo) and _same(lb, lo)
    store.close()


def test_submap_without_a_finite_point_is_refused(gpu, gorio, submap_case):
    frames, rel, store, ids = submap_case
    g = gorio.ApdGicp(**KW)
    g.setInputTarget(*frames[5])
    for pick in ([0], [6], [0, 6, 0]):  # empty; all NaN; both, one of them twice
        with pytest.raises(gorio.GorioError) as e:
            g.setInputTargetSubmapKeyframes(store, [ids[k] for k in pick], [rel[k] for k in pick])
        assert e.value.code == INVALID and "no finite point" in str(e.value)
    with pytest.raises(gorio.GorioError) as e:
        g.setInputTargetSubmapKeyframes(store, [ids[5], 99], [rel[5], rel[5]])
    assert e.value.code == INVALID and "has not been added" in str(e.value)
    g._n_tgt = len(frames[5][0])
    assert _same(g.getTargetPoints()[0], frames[5][0])  # a failed call changes nothing


# ---------------------------------------------------------------------------------------------------------------- 6. Scan Context
def test_scan_context_from_keyframes_equals_add_scans(gpu, gorio):
    scans = [ss.keyframe(0.0, 900), (np.zeros((0, 3), F), np.zeros(0, F)), ss.keyframe(0.6, 902)]
    store = gorio.KeyframeStore()
    ids = [store.add(x, i) for x, i in scans]
    a, b = gorio.ScanContext(), gorio.ScanContext()
    assert a.add_scans(scans) == 0 and b.add_keyframes(store, ids) == 0
    assert store.counters()["device_copies"] == 1 and b.state()["n_scans"] == 3
    for k in range(3):
        for u, v in zip(a.descriptor(k), b.descriptor(k)):
            assert u.tobytes() == v.tobytes(), k
    assert b.descriptor(0)[0].any() and not b.descriptor(1)[0].any()
    ra, rb = a.detect(2, [0, 1]), b.detect(2, [0, 1])
    assert ra[:3] == rb[:3] and ra[0] == -1  # fewer than NUM_EXCLUDE_RECENT keyframes: the early return, on both
    # nine more, one at a time, the last one back at the first one's place: a query past NUM_EXCLUDE_RECENT searches the database
    more = [ss.keyframe(0.3 * k, 900 + k) for k in range(3, 11)] + [ss.keyframe(0.0, 950)]
    for k, (x, i) in enumerate(more):
        assert a.add_scan(x, i) == 3 + k and b.add_keyframes(store, [store.add(x, i)]) == 3 + k
    assert a.descriptor(11)[0].tobytes() == b.descriptor(11)[0].tobytes()
    ra, rb = a.detect(11, list(range(11))), b.detect(11, list(range(11)))
    assert ra[0] == rb[0] == 0 and np.float32(ra[1]).tobytes() == np.float32(rb[1]).tobytes() and ra[2] == rb[2]
    assert b.add_keyframes(store, [ids[2], ids[2]]) == 12 and b.descriptor(13)[0].tobytes() == b.descriptor(2)[0].tobytes()  # a keyframe may be listed again
    bare = store.add(scans[0][0])  # no intensity column
    with pytest.raises(gorio.GorioError) as e:
        b.add_keyframes(store, [ids[0], bare])
    assert e.value.code == STATE and "intensity" in str(e.value) and b.state()["n_scans"] == 14
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 7. batches
@pytest.fixture(scope="module")
def four_clouds():
    return [synth.scan_pair(1500 + 111 * k, 1700 + 97 * k, seed=20 + k)[:4] for k in range(4)]


@pytest.mark.parametrize("shared", ["source", "target"])
def test_batches_share_one_keyframe(gpu, gorio, pair, four_clouds, shared):
    """loop_detector.cpp:222 / :391: the new keyframe against each of four candidates, as the source or as the target of all four."""
    sx, sl, _, _ = pair
    store = gorio.KeyframeStore()
    kid = store.add(sx, label=sl)
    singles, batch = [gorio.ApdGicp(**KW) for _ in range(4)], [gorio.ApdGicp(**KW) for _ in range(4)]
    for q in range(4):
        ox, ol = four_clouds[q][2], four_clouds[q][3]
        if shared == "source":
            singles[q].setInputSource(sx, sl), singles[q].setInputTarget(ox, ol)
            batch[q].setInputSourceKeyframe(store, kid), batch[q].setInputTarget(ox, ol)
        else:
            singles[q].setInputTarget(sx, sl), singles[q].setInputSource(ox, ol)
            batch[q].setInputTargetKeyframe(store, kid), batch[q].setInputSource(ox, ol)
    assert store.info(kid)["sharers"] == 4
    want = [g.align() for g in singles]
    got = gorio.align_batch(batch)
    info = store.info(kid)
    assert info["cov_count"] == len(sx) and info["index_built"]
    for q in range(4):
        _same_align(want[q], got[q])
    Ts = np.stack([r["T"] for r in want])
    ws = [g.getFitnessScore(T) for g, T in zip(singles, Ts)]
    scores, inl = gorio.fitness_score_batch(batch, Ts)
    assert scores.tobytes() == np.array([w[0] for w in ws]).tobytes() and inl.tobytes() == np.array([w[1] for w in ws]).tobytes()
    assert len({w[0] for w in ws}) == 4
    store.close()


# ---------------------------------------------------------------------------------------------------------------- 8. lifetime
@pytest.mark.parametrize("how", ["release", "destroy"])
def test_handles_keep_a_keyframe_the_store_lets_go_of(gpu, gorio, pair, how):
    sx, sl, tx, tl = pair
    inten = np.linspace(0, 30, len(tx)).astype(F)
    store = gorio.KeyframeStore()
    kt, ks, k2 = store.add(tx, inten, tl), store.add(sx, label=sl), store.add(tx[:700], inten[:700], tl[:700])
    g = gorio.ApdGicp(**KW)
    g.setInputTargetKeyframe(store, kt)
    g.setInputSourceKeyframe(store, ks)
    r0 = g.align()
    if how == "destroy":
        store.close()
    else:
        store.release(kt)
        store.release(ks)
        assert store.count() == (3, 1) and store.info(kt) == dict.fromkeys(("n", "resident", "has_intensity", "cov_count", "cov_k", "cov_reg", "index_built", "sharers"), 0)
        h, nd, sc = gorio.ApdGicp(**KW), gorio.Ndt(), gorio.ScanContext()
        calls = [lambda: h.setInputSourceKeyframe(store, kt), lambda: h.setInputTargetKeyframe(store, kt), lambda: nd.set_source_from_keyframe(store, kt),
                 lambda: nd.set_target_from_keyframe(store, kt), lambda: h.setInputTargetSubmapKeyframes(store, [k2, kt], [np.eye(4)] * 2),
                 lambda: sc.add_keyframes(store, [k2, kt]), lambda: store.get(kt), lambda: store.release(kt)]
        for q, call in enumerate(calls):
            with pytest.raises(gorio.GorioError) as e:
                call()
            assert e.value.code == STATE and "released" in str(e.value), q
        assert sc.state()["n_scans"] == 0
        gx, gi, gl = store.get(k2)  # the ids after it are unaffected
        assert _same(gx, tx[:700]) and _same(gi, inten[:700]) and _same(gl, tl[:700])
        assert h.setInputTargetSubmapKeyframes(store, [k2], [np.eye(4)]) == 700 and store.add(sx[:5]) == 3
    _same_align(g.align(), r0)  # the handle holds what it was given
    gx, gl = g.getTargetPoints()
    assert _same(gx, tx) and _same(gl, tl)
    store.close()
