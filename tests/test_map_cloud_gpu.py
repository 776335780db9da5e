"""The map cloud (include/gorio_map.h) on the MI355X against tests/map_cloud_restatement.py, BIT FOR BIT: xyz and intensity in order for
resolution <= 0, the centres in order for resolution > 0, and the fields of gorio_map_info_t.  No tolerance: the kernels perform the
restatement's operations.  (The one thing the header leaves open is the payload of a NaN coordinate that a kept NaN point produces:
NaNs are compared by position.)"""
import numpy as np
import pytest

import map_cloud_restatement as mr
import scan_pipeline_restatement as sr

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
INVALID, STATE, UNSUPPORTED = -1, -3, -5
FRAME_BYTES, RECORD_BYTES = 72, 52  # what generate uploads: per listed keyframe, and once with resolution > 0 (include/gorio_map.h)


def _same(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(U)[~na], b.view(U)[~nb])


def _add(store, frames):
    return [store.add(x, i) for x, i in frames]


def _check(mc, store, ids, frames, poses, res):
    """generate on the device == the restatement on host copies of the same keyframes; returns the restatement's (xyz, info)."""
    xyz, inten = mc.generate(store, ids, poses, res)
    wx, wi, winfo = mr.generate(frames, poses, res)
    assert xyz.shape == wx.shape, (xyz.shape, wx.shape, mc.info(), winfo)
    assert _same(xyz, wx) and _same(inten, wi)
    assert mc.info() == winfo
    return wx, winfo


def _inside(n, seed, reach=45.0):
    """n points that all pass the gate (|p| < reach < 50), 0.1 m jitter around a 0.5 m grid so that voxels are shared."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (rng.uniform(1.0, reach, n) / np.linalg.norm(v, axis=1))[:, None]
    v = np.round(v / 0.5) * 0.5 + rng.normal(0.0, 0.1, (n, 3))
    v = v.astype(F)
    assert mr.gate(v).all()
    return v, rng.uniform(0, 40, n).astype(F)


# ------------------------------------------------------------------------------------------------------------------ keyframe sizes
@pytest.mark.parametrize("res", [0.0, -1.0, 0.5])
def test_keyframe_sizes_around_the_wave_and_the_block(gpu, gorio, res):
    sizes = [0, 1, 63, 64, 65, 255, 256, 257]
    frames, poses = mr.scene(sizes, seed=40)
    frames[4] = (frames[4][0], None)  # one keyframe without an intensity column contributes 0
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    _, info = _check(mc, store, ids, frames, poses, res)
    assert info["n_listed"] == sum(sizes) and 0 < info["n_kept"] < sum(sizes)  # the gate dropped some
    for k in (7, 1):  # a single keyframe
        _check(mc, store, [ids[k]], [frames[k]], [poses[k]], res)
    order = [5, 0, 7, 2, 0, 3]  # another order, an empty keyframe twice
    _check(mc, store, [ids[k] for k in order], [frames[k] for k in order], [poses[k] for k in order], res)
    xyz, inten = mc.generate(store, [ids[0], ids[0]], [poses[0], poses[1]], res)  # only empty keyframes: not an error
    assert xyz.shape == (0, 3) and inten.shape == (0,) and mc.info()["n_listed"] == 0
    mc.close()
    store.close()


def _scan_params(gorio, p):
    kw = {k: getattr(p, k) for k in ("power_threshold", "rotation", "scan_period", "distance_near", "distance_far", "z_low", "z_high", "outlier_method", "mean_k", "stddev_mul",
                                     "radius", "min_neighbors", "dbscan_core_min_pts", "dbscan_eps", "dbscan_min_cluster_size", "dbscan_max_cluster_size")}
    kw.update(enable_dynamic_object_removal=int(p.enable_dynamic_object_removal), deskew=int(p.deskew), ground=int(p.ground))
    sp = gorio.prep.scan_default_params(**kw)
    for k, v in p.reve.items():
        setattr(sp.reve, k, v)
    return sp


def test_keyframe_that_came_from_a_scan(gpu, gorio, oracle_apd):
    raw, p, samples = sr.chain_inputs(*sr.CHAIN_CASES[0], oracle_apd)
    pipe = gorio.prep.ScanPipeline(_scan_params(gorio, p))
    pipe.load(raw)
    assert pipe.run(samples, sr.CHAIN_ANG_VEL)["status"] == "ok"
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    kid = store.add_from_scan(pipe)
    xyz, inten, _, _ = pipe.output()
    assert len(xyz) > 256 and inten.any()
    extra = _inside(300, 3)
    k2 = store.add(*extra)
    frames, poses = [(xyz, inten), extra, (xyz, inten)], [mr.curve_pose(2), mr.curve_pose(5), mr.curve_pose(9)]
    for res in (0.0, 0.3):
        _check(mc, store, [kid, k2, kid], frames, poses, res)
    pipe.close()  # the store's share keeps the cloud
    _check(mc, store, [kid], frames[:1], poses[:1], 0.0)
    mc.close()
    store.close()


# ------------------------------------------------------------------------------------------------------------------ block scan
def test_block_scan_wraps_past_1024_blocks(gpu, gorio):
    """More than 1024 x 256 points in one call: the single-workgroup scan of the block counts makes a second trip."""
    rng = np.random.default_rng(3)
    frames = []
    for n in (140001, 125000):
        xyz = rng.uniform(-40, 40, (n, 3)).astype(F)  # the corners lie beyond 50 m
        xyz[rng.random(n) < 0.05, 1] = np.nan
        xyz[n - 1] = 1.0  # the last point of the last block survives
        frames.append((xyz, rng.uniform(0, 40, n).astype(F)))
    poses = [mr.curve_pose(3), np.eye(4)]
    assert sum((len(x) + 255) // 256 for x, _ in frames) > 1024
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    _, info = _check(mc, store, ids, frames, poses, 0.0)
    assert 1024 * 256 * 0.6 < info["n_kept"] < info["n_listed"]
    _, info = _check(mc, store, ids, frames, poses, 1.0)
    assert info["n_finite"] < info["n_kept"] and info["n_voxels"] > 4096
    mc.close()
    store.close()


# ------------------------------------------------------------------------------------------------------------------ gate, NaN, Inf
def test_gate_edges_nan_and_inf(gpu, gorio):
    above = np.nextafter(F(40.0), F(np.inf))
    xyz = np.array([[30, 40, 0], [30, above, 0], [0, 0, 50], [np.nan, 1, 1], [np.inf, 0, 0], [1, -np.inf, 0], [0, 0, np.nextafter(F(50.0), F(np.inf))], [2.5, 1.5, 0.5]], F)
    inten = np.arange(1, 9, dtype=F)
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    kid = store.add(xyz, inten)
    got, gi = mc.generate(store, [kid], [np.eye(4)], 0.0)
    assert gi.tolist() == [1.0, 3.0, 4.0, 8.0] and np.isnan(got[2]).all() and _same(got[[0, 1, 3]], xyz[[0, 2, 7]])  # the NaN point survives
    for res in (0.0, 0.5):
        _, info = _check(mc, store, [kid], [(xyz, inten)], [np.eye(4)], res)
    assert (info["n_kept"], info["n_finite"], info["n_voxels"]) == (4, 3, 3)  # ... and vanishes with a resolution
    # the first kept point is not finite: the anchor falls to the next finite one
    lead = np.array([[np.inf, 0, 0], [np.nan, 1, 1], [2.5, 1.5, 0.5], [2.6, 1.5, 0.5], [-3.0, 0.2, 0.1]], F)
    k2 = store.add(lead)
    _, info = _check(mc, store, [k2, kid], [(lead, None), (xyz, inten)], [np.eye(4), mr.curve_pose(1)], 1.0)
    assert info["anchor"] == [2.0, 1.0, 0.0] and info["min_k"][0] < 0
    # one point: one centre, the point's own float
    k3 = store.add(np.array([[10.1, 20.2, -0.3]], F))
    got, gi = mc.generate(store, [k3], [np.eye(4)], 0.05)
    assert _same(got, np.array([[10.1, 20.2, -0.3]], F)) and gi.tolist() == [0.0]
    # only non-finite kept points: no voxel
    k4 = store.add(np.array([[np.nan, 0, 0], [0, np.nan, 0]], F))
    _, info = _check(mc, store, [k4], [(np.array([[np.nan, 0, 0], [0, np.nan, 0]], F), None)], [np.eye(4)], 0.5)
    assert (info["n_kept"], info["n_finite"], info["n_voxels"]) == (2, 0, 0)
    mc.close()
    store.close()


@pytest.mark.parametrize("res", [0.0, 0.05])
def test_every_point_gated_away(gpu, gorio, res):
    rng = np.random.default_rng(8)
    v = rng.normal(size=(700, 3))
    v *= (rng.uniform(50.5, 90.0, 700) / np.linalg.norm(v, axis=1))[:, None]
    v = v.astype(F)
    v[5, 0] = np.inf
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, [(v, None), (v[:300], None)])
    xyz, inten = mc.generate(store, ids, [np.eye(4), mr.curve_pose(1)], res)  # GORIO_OK with 0 points
    assert xyz.shape == (0, 3) and inten.shape == (0,)
    assert mc.info() == dict(n_listed=1000, n_kept=0, n_finite=0, n_voxels=0, anchor=[0.0] * 3, min_k=[0] * 3, max_k=[0] * 3)
    mc.close()
    store.close()


# ------------------------------------------------------------------------------------------------------------------ the float pose
def test_pose_is_cast_to_float_not_applied_in_double(gpu, gorio):
    frames, poses = mr.scene([500, 500], seed=9)
    qf, _ = mr.stage_a(frames, poses)
    qd, _ = mr.stage_a(frames, poses, mr.transform_double)
    assert np.float64(np.float32(poses[1][0, 3])) != poses[1][0, 3]  # a translation that changes under the cast
    n_diff = int((qf.view(U) != qd.view(U)).any(axis=1).sum())
    assert n_diff > len(qf) // 4  # the input tells the two transforms apart
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    got, _ = mc.generate(store, ids, poses, 0.0)
    assert _same(got, qf) and not _same(got, qd)
    _check(mc, store, ids, frames, poses, 0.05)  # (an ulp in a point seldom moves it to another voxel: the centres cannot tell the two apart)
    mc.close()
    store.close()


# ------------------------------------------------------------------------------------------------------------------ the lattice
def test_negative_cells_with_the_anchor_in_the_middle(gpu, gorio):
    frames, poses = mr.scene([900] * 5, seed=21)
    order = [2, 0, 4, 1, 3]  # the first keyframe listed stands in the middle of the trajectory
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    _, info = _check(mc, store, [ids[k] for k in order], [frames[k] for k in order], [poses[k] for k in order], 0.3)
    assert all(lo < -20 for lo in info["min_k"][:2]) and all(hi > 20 for hi in info["max_k"][:2])
    mc.close()
    store.close()


def test_the_same_keyframe_listed_five_times(gpu, gorio):
    frames, poses = mr.scene([1500], seed=33)
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    one, info1 = _check(mc, store, ids, frames, poses, 0.1)
    five, info5 = _check(mc, store, ids * 5, frames * 5, poses * 5, 0.1)
    assert _same(one, five) and info5["n_kept"] == 5 * info1["n_kept"] and info5["n_voxels"] == info1["n_voxels"]
    raw, _ = _check(mc, store, ids * 5, frames * 5, poses * 5, 0.0)
    assert len(raw) == 5 * info1["n_kept"]
    mc.close()
    store.close()


@pytest.mark.parametrize("kept", [1, 4095, 4096, 4097, 16383, 16384, 16385, 70001])
def test_kept_totals_around_the_sorts_size_steps(gpu, gorio, kept):
    """The tiled sort pads to one 4096-key tile, then to powers of two: totals at, below and above the steps, and five merge levels."""
    split = [kept // 3, kept - kept // 3]  # two keyframes; the first is empty for kept = 1
    frames = [_inside(n, 50 + kept + k) for k, n in enumerate(split)]
    poses = [mr.curve_pose(1), mr.curve_pose(4)]
    store, mc = gorio.KeyframeStore(), gorio.MapCloud()
    ids = _add(store, frames)
    _, info = _check(mc, store, ids, frames, poses, 0.5)
    assert info["n_kept"] == info["n_finite"] == kept and 0 < info["n_voxels"] <= kept
    mc.close()
    store.close()


@pytest.fixture(scope="module")
def four_frames(gorio, gpu):
    frames, poses = mr.scene([3000, 2500, 3100, 2900], seed=60)
    store = gorio.KeyframeStore()
    ids = _add(store, frames)
    yield frames, poses, store, ids
    store.close()


@pytest.mark.parametrize("res", [0.05, 0.5, 1.0])
def test_resolutions(gpu, gorio, four_frames, res):
    frames, poses, store, ids = four_frames
    mc = gorio.MapCloud()
    _, info = _check(mc, store, ids, frames, poses, res)
    assert 0 < info["n_voxels"] < info["n_finite"]
    mc.close()


# ------------------------------------------------------------------------------------------------------------------ limits and state
def test_refusals_leave_the_previous_result(gpu, gorio, four_frames):
    frames, poses, store, ids = four_frames
    mc = gorio.MapCloud()
    held, _ = _check(mc, store, ids[:2], frames[:2], poses[:2], 0.0)  # stage A's output is the result held
    before = (mc.info(), mc.counters(), mc.capacities())
    far = [np.eye(4), np.eye(4)]
    far[1][0, 3] = 300.0
    pts = np.array([[1, 1, 1]], F)
    a, b, gone = store.add(pts), store.add(pts), store.add(pts)
    store.release(gone)
    for res, what in ((1e-4, "2^21"), (1e-8, "2^30")):  # two keyframes 300 m apart: 3e6 cells, then 3e10
        with pytest.raises(gorio.GorioError) as e:
            mc.generate(store, [a, b], far, res)
        assert e.value.code == UNSUPPORTED and what in str(e.value)
    with pytest.raises(gorio.GorioError) as e:
        mc.generate(store, [ids[0], gone], poses[:2], 0.05)
    assert e.value.code == STATE and "keyframe %d has been released" % gone in str(e.value)
    with pytest.raises(gorio.GorioError) as e:
        mc.generate(store, [ids[0], gone + 1], poses[:2], 0.05)
    assert e.value.code == INVALID and "has not been added" in str(e.value)
    got, _ = mc.get()
    after = (mc.info(), mc.counters(), mc.capacities())
    assert _same(got, held) and after[0] == before[0] and after[1] == dict(before[1], points_downloaded=before[1]["points_downloaded"] + len(held))
    assert after[2]["result"] == before[2]["result"] and after[2]["stage"] == before[2]["stage"]
    _check(mc, store, [a, b], [(pts, None)] * 2, far, 0.01)  # 30 000 cells apart: fine
    mc.close()


def test_handle_reuse_keeps_its_buffers(gpu, gorio, four_frames):
    frames, poses, store, ids = four_frames
    small = [_inside(40, 1)]
    ks = _add(store, small)
    empty = store.add(np.zeros((0, 3), F))
    mc = gorio.MapCloud()
    calls = [(ids, frames, poses), (ks, small, [mr.curve_pose(7)]), ([empty], [(np.zeros((0, 3), F), None)], [np.eye(4)]), (ids, frames, poses)]
    caps = None
    for q, (i, f, p) in enumerate(calls):
        for res in (0.05, 0.0):
            got = mc.generate(store, i, p, res)
            fresh = gorio.MapCloud()
            want = fresh.generate(store, i, p, res)
            assert _same(got[0], want[0]) and _same(got[1], want[1]) and mc.info() == fresh.info(), (q, res)
            fresh.close()
            _check(mc, store, i, f, p, res)
        if q == 0:
            caps = mc.capacities()
            assert caps["stage"] >= 11500 and caps["keys"] >= 16384 and caps["result"] > 0
        assert mc.capacities() == caps, q  # grown by the first large call, kept when a smaller map follows
    mc.close()


def test_repeat_run_gives_identical_bits(gpu, gorio, four_frames):
    frames, poses, store, ids = four_frames
    mc = gorio.MapCloud()
    for res in (0.05, 0.0):
        a = mc.generate(store, ids, poses, res)
        b = mc.generate(store, ids, poses, res)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[0]) > 1000
    mc.close()


def test_counters(gpu, gorio, four_frames):
    frames, poses, store, ids = four_frames
    mc = gorio.MapCloud()
    c0 = store.counters()
    assert mc.counters() == dict(generates=0, points_downloaded=0, bytes_uploaded=0)
    n1 = mc.generate_only(store, ids, poses, 0.5)
    assert mc.counters() == dict(generates=1, points_downloaded=0, bytes_uploaded=4 * FRAME_BYTES + RECORD_BYTES)  # nothing came down yet
    xyz, _ = mc.get()
    assert len(xyz) == n1 and mc.counters()["points_downloaded"] == n1
    n2 = mc.generate_only(store, ids[:3], poses[:3], 0.0)
    mc.get()
    mc.get()
    assert mc.counters() == dict(generates=2, points_downloaded=n1 + 2 * n2, bytes_uploaded=7 * FRAME_BYTES + RECORD_BYTES)
    with pytest.raises(gorio.GorioError):
        mc.generate_only(store, [999], poses[:1], 0.0)
    assert mc.counters()["generates"] == 2
    assert store.counters() == c0  # the map takes the keyframes where they are: no upload, download or device copy of the store's
    assert all(store.info(k)["sharers"] == 0 for k in ids)  # the shares held during the call are back
    mc.close()
