"""Batch surface on the MI355X: gorio_apd_fitness_score_batch against the single fitness calls (bit for bit), its validation, and the two
C++ drivers of the batch members -- FastAPDGICP::alignBatch / getFitnessScoreBatch / getInlierFractionBatch in the loop-closure pattern
of loop_detector.cpp:386-422, VelPreintegration::batch against single constructions."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

synth = importlib.import_module("go-rio_amd.synth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
LOOP_DRIVER = os.path.join(HOST, "test", "loop_closure_batch")
PREINT_DRIVER = os.path.join(HOST, "test", "preint_batch")
DBL_MAX = np.finfo(np.float64).max

pytestmark = pytest.mark.gpu


def _far(T):
    """T moved 1 km away: no source point has a target point within a few metres."""
    T = np.array(T, np.float32)
    T[:3, 3] += 1000.0
    return T


def _fitness_pairs(gorio):
    """16 (object, pose) pairs: mixed source sizes (1 point included), brute and pruned search, five sources sharing one 100k-point
    target, two sharing a scan-sized target, and one pose that puts the source far from everything."""
    big_x, big_l = synth.local_map(100000, seed=synth.BASE_SEED + 7)
    owner = gorio.ApdGicp(search=1)
    owner.setInputTarget(big_x, big_l)
    objs, Ts, keep = [], [], [owner]
    for q in range(5):  # against the shared 100k map, pruned search
        sx, sl = synth.radar_scan(1500 + 700 * q, seed=900 + q)
        g = gorio.ApdGicp(search=1)
        g.setInputTargetShared(owner)
        g.setInputSource(sx, sl)
        objs.append(g)
        Ts.append(synth.gt_transform().astype(np.float32) if q % 2 else np.eye(4, dtype=np.float32))
    for q in range(8):  # scan pairs of their own, both search modes
        sx, sl, tx, tl, T = synth.scan_pair(300 + 611 * q, 2500 - 150 * q, seed=950 + q)
        g = gorio.ApdGicp(search=q % 2)
        g.setInputTarget(tx, tl)
        g.setInputSource(sx, sl)
        objs.append(g)
        Ts.append(_far(T) if q == 3 else T.astype(np.float32))
    sx, sl, tx, tl, T = synth.scan_pair(1, 1200, seed=970)  # a 1-point source
    g = gorio.ApdGicp(search=0)
    g.setInputTarget(tx, tl)
    g.setInputSource(sx[:1], sl[:1])
    objs.append(g)
    Ts.append(T.astype(np.float32))
    sx, sl, tx, tl, T = synth.scan_pair(3000, 3000, seed=971)  # two sources on one shared scan-sized target, brute force
    a = gorio.ApdGicp(search=0)
    a.setInputTarget(tx, tl)
    a.setInputSource(sx, sl)
    b = gorio.ApdGicp(search=0)
    b.setInputTargetShared(a)
    b.setInputSource(sx[::2], sl[::2])
    objs += [a, b]
    Ts += [T.astype(np.float32), T.astype(np.float32)]
    assert len(objs) == 16
    return objs, np.stack(Ts), keep


@pytest.mark.parametrize("max_range,inlier_dist", [(DBL_MAX, 0.0), (1.0, 1.0), (4.0, 0.0)])
def test_fitness_batch_equals_single_calls(gpu, gorio, max_range, inlier_dist):
    objs, Ts, _keep = _fitness_pairs(gorio)
    single = [o.getFitnessScore(Ts[q], max_range=max_range, inlier_dist=inlier_dist) for q, o in enumerate(objs)]
    scores, fracs = gorio.fitness_score_batch(objs, Ts, max_range=max_range, inlier_dist=inlier_dist)
    for q in range(len(objs)):
        assert scores[q] == single[q][0] and fracs[q] == single[q][1], (q, scores[q], single[q])
    assert fracs[8] == 0.0
    if max_range == DBL_MAX:
        assert np.all(scores < DBL_MAX)  # every point qualifies, however far
    else:
        assert scores[8] == DBL_MAX  # the source moved 1 km away: no point within max_range
        assert np.all(scores[np.arange(16) != 8] < DBL_MAX)
    # the single calls again after the batch: the batch left every handle scoring as before
    again = [o.getFitnessScore(Ts[q], max_range=max_range, inlier_dist=inlier_dist) for q, o in enumerate(objs)]
    assert again == single
    with pytest.raises(gorio.GorioError):
        objs[0].getCorrespondences()  # corr_valid is false afterwards, as after the single call


def test_fitness_batch_errors_leave_handles_untouched(gpu, gorio):
    sx, sl, tx, tl, T = synth.scan_pair(2000, 2200, seed=980)
    T = T.astype(np.float32)
    a, b = gorio.ApdGicp(search=1), gorio.ApdGicp()
    for g in (a, b):
        g.setInputTarget(tx, tl)
        g.setInputSource(sx, sl)
    before = [a.getFitnessScore(T), b.getFitnessScore(T)]
    Ts = np.stack([T, T])

    with pytest.raises(gorio.GorioError) as e:
        gorio.fitness_score_batch([a, a], Ts)  # the same handle twice
    assert e.value.code == -1 and "handles[1]" in str(e.value)

    s = gorio.ApdGicp()
    s.setInputTarget(tx, tl)
    s.setInputSource(sx, sl)
    s.debugSetShard(2, 0)
    with pytest.raises(gorio.GorioError) as e:
        gorio.fitness_score_batch([a, s], Ts)  # a sharded handle
    assert e.value.code == -3 and "handles[1]" in str(e.value)

    m = gorio.ApdGicp()
    m.setInputSource(sx, sl)  # no target
    with pytest.raises(gorio.GorioError) as e:
        gorio.fitness_score_batch([a, b, m], np.stack([T, T, T]))
    assert e.value.code == -3 and "handles[2]" in str(e.value)

    assert [a.getFitnessScore(T), b.getFitnessScore(T)] == before
    scores, fracs = gorio.fitness_score_batch([a, b], Ts)
    assert (scores[0], fracs[0]) == before[0] and (scores[1], fracs[1]) == before[1]


def _loop_file(path, target, cands):
    tx, tl = target
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", len(cands), tx.shape[0]))
        f.write(np.concatenate([tx, tl[:, None]], axis=1).astype(np.float32).tobytes())
        for sx, sl, guess in cands:
            f.write(struct.pack("<i", sx.shape[0]))
            f.write(np.concatenate([sx, sl[:, None]], axis=1).astype(np.float32).tobytes())
            f.write(np.ascontiguousarray(guess, np.float32).tobytes())
    return path


def test_loop_closure_driver_batch_equals_single(gpu, gorio, oracle_apd, tmp_path, pose_err):
    """N x (setInputSource, align, getFitnessScore) on one object == alignBatch + getFitnessScoreBatch over N objects sharing the target."""
    target = synth.radar_scan(3000, seed=1000)
    cands = []
    for k in range(6):
        pose = np.eye(4)
        pose[:3, 3] = [0.3 * k, -0.1 * k, 0.0]
        pose[:3, :3] = synth.rpy_to_matrix([0, 0, 1.0 * k])
        sx, sl = synth.radar_scan(1800 + 97 * k, seed=1010 + k, sensor_pose=pose)
        cands.append((sx, sl, np.eye(4, dtype=np.float32)))
    r = subprocess.run([LOOP_DRIVER, _loop_file(str(tmp_path / "loop.bin"), target, cands)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    tail = lines.pop()
    assert tail == {"mismatch_error": "runtime_error", "unchanged": 1}
    single = [l for l in lines if l["mode"] == "single"]
    batch = [l for l in lines if l["mode"] == "batch"]
    assert len(single) == len(batch) == len(cands)
    for s, b in zip(single, batch):
        for key in ("T", "converged", "nr_iterations", "H", "fitness", "inlier", "aligned0"):
            assert s[key] == b[key], (s["i"], key)
    # the poses against the CPU oracle
    p = oracle_apd.launch_params()
    ct = oracle_apd.calculate_covariances(target[0], p)
    close = 0
    for (sx, sl, guess), b in zip(cands, batch):
        ro = oracle_apd.align(guess, sx, sl, target[0], target[1], oracle_apd.calculate_covariances(sx, p), ct, p)
        dt, dr = pose_err(ro["T"], np.array(b["T"], np.float32).reshape(4, 4))
        close += dt < 1e-4 and dr < 1e-4
    assert close >= 2


def _imu_requests(path, wins):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(wins)))
        for win, typ, quantum, groups in wins:
            for t, d in ((win["gyr_t"], win["gyr"]), (win["vel_t"], win["vel"])):
                f.write(struct.pack("<i", len(t)))
                f.write(np.concatenate([np.asarray(t)[:, None], d], axis=1).astype(np.float64).tobytes())
            f.write(struct.pack("<didi", win["start_t"], typ, quantum, len(groups)))
            for g in groups:
                f.write(struct.pack("<i", len(g)))
                f.write(np.asarray(g, np.float64).tobytes())
    return path


def _preint_requests(bad=None):
    reqs = []
    for k in range(8):
        win = synth.imu_window(seed=1100 + k, duration=0.6 + 0.1 * k)
        s, e = win["start_t"], win["end_t"]
        if k in (1, 4):  # LPM (IterativeIntegrator output)
            reqs.append((win, 0, -1.0, [[e]]))
        elif k == 6:  # chunked
            reqs.append((win, 1, 0.4, [[e]]))
        else:
            reqs.append((win, 1, -1.0, [[0.5 * (s + e), e], [e]]))
        if k == bad:  # inference time before start_t: GyroVelData::get's invalid_argument (TYPES:160)
            reqs[-1] = (win, 1, -1.0, [[s - 0.1]])
    return reqs


def test_preint_driver_batch_equals_single(gpu, gorio, tmp_path):
    r = subprocess.run([PREINT_DRIVER, _imu_requests(str(tmp_path / "imu.bin"), _preint_requests())], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    single = [l for l in lines if l["mode"] == "single"]
    batch = [l for l in lines if l["mode"] == "batch"]
    assert len(single) == len(batch) == 8
    for s, b in zip(single, batch):
        assert s["records"] == b["records"] and s["inflated"] == b["inflated"], s["k"]
        assert s["overloads_refused"] == b["overloads_refused"] == 2
        assert np.all(np.isfinite(np.array(b["records"])))


def test_preint_driver_failing_window(gpu, gorio, tmp_path):
    path = _imu_requests(str(tmp_path / "imu_bad.bin"), _preint_requests(bad=5))
    r = subprocess.run([PREINT_DRIVER, path, "errors"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["single_index"] == 5 and out["single_error"] == "invalid_argument"
    assert out["batch_error"] == out["single_error"] and "window 5" in out["batch_message"]
