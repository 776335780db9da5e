"""Time per call of the k-NN and radius queries of include/gorio_search.h, device-pointer forms, beside the library's own searches of
the same clouds in the same run:

    python tools/search_bench.py [--repeats 30] [--warmup 5] [--out FILE.json]

Per cloud (a 16 384-point radar scan, a 100 000-point local map) with 16 384 queries (another scan, a few decimetres off):
  knn20          gorio_search_knn_device, k = 20: `repeats` calls enqueued back to back, one device synchronise, host clock / repeats
  knn20_self     the same with the cloud's own points as queries (no query sort)
  radius1m       gorio_search_radius_device, 1 m: the call synchronises by itself (it needs the totals); host clock per call, median
  self_knn_stage stage 0 of gorio_apd_get_stage_times for the cloud alone: self k-NN (k = 20) + covariances, device events
  nn_search      stage 1 per launch of a 20-iteration Gauss-Newton align of the queries against the cloud: one 1-NN correspondence search
A GPU is required; nothing here falls back."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gorio = importlib.import_module("go-rio_amd")
synth = gorio.synth


class Hip:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")

    def dev(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p.value

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
        return p.value

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0


def timed_enqueue(hip, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    hip.sync()
    t = time.perf_counter()
    for _ in range(repeats):
        fn()
    hip.sync()
    return (time.perf_counter() - t) / repeats


def timed_calls(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = Hip()
    nq, k = 16384, 20
    pose = np.eye(4)
    pose[:3, 3] = [0.3, -0.2, 0.05]
    q, ql = synth.radar_scan(nq, seed=synth.BASE_SEED + 11, sensor_pose=pose)
    clouds = {"scan16k": synth.radar_scan(16384, seed=synth.BASE_SEED + 10), "map100k": synth.local_map(100000, seed=synth.BASE_SEED + 12)}
    d_q = hip.dev(q)
    rows = []
    for name, (xyz, lab) in clouds.items():
        n = len(xyz)
        s = gorio.Search()
        s.set_cloud(xyz)
        m = max(n, nq)
        d_idx, d_sqd, d_cnt = hip.alloc(4 * m * k), hip.alloc(4 * m * k), hip.alloc(4 * m)
        row = dict(cloud=name, n=n, nq=nq, k=k, repeats=a.repeats)
        row["knn20_ms"] = 1e3 * timed_enqueue(hip, lambda: s.knn_device(d_q, nq, 12, k, d_idx, d_sqd, d_cnt), a.warmup, a.repeats)
        row["knn20_self_ms"] = 1e3 * timed_enqueue(hip, lambda: s.knn_device(None, n, 12, k, d_idx, d_sqd, d_cnt), a.warmup, a.repeats)
        res = {}

        def radius():
            res["cnt"], res["total"] = s.radius_device(d_q, nq, 12, 1.0)

        med, lo, hi = timed_calls(radius, a.warmup, a.repeats)
        row.update(radius1m_ms=1e3 * med, radius1m_min_ms=1e3 * lo, radius1m_max_ms=1e3 * hi, radius1m_total=int(res["total"]), radius1m_longest=int(res["cnt"].max()))
        s.close()
        # the library's own searches of the same cloud
        reg = gorio.ApdGicp(search=1, k_correspondences=k)
        st = []
        for _ in range(a.warmup + a.repeats):
            reg.setInputTarget(xyz, lab)  # new points: covariances and index are stale again
            reg.setProfiling(True)
            reg.calculateCovariances()
            sec, cnt = reg.getStageTimes()
            st.append((sec[0], sec[4]))
        st = np.array(st[a.warmup:])
        row["self_knn_stage_ms"] = 1e3 * float(np.median(st[:, 0]))
        row["index_build_ms"] = 1e3 * float(np.median(st[:, 1]))
        al = gorio.ApdGicp(search=1, k_correspondences=k, corr_dist_threshold=2.0, max_iterations=20, optimizer=0, rotation_epsilon=0.0, transformation_epsilon=0.0)
        al.setInputTarget(xyz, lab)
        nn = []
        for _ in range(3 + max(a.repeats // 5, 3)):
            al.setInputSource(q, ql)
            al.setProfiling(True)
            al.align()
            sec, cnt = al.getStageTimes()
            nn.append(sec[1] / max(cnt[1], 1))
        row["nn_search_ms"] = 1e3 * float(np.median(nn[3:]))
        row["knn20_over_self_stage"] = row["knn20_ms"] / row["self_knn_stage_ms"]
        row["knn20_self_over_self_stage"] = row["knn20_self_ms"] / row["self_knn_stage_ms"]
        row["knn20_over_nn_search"] = row["knn20_ms"] / row["nn_search_ms"]
        row["radius1m_over_nn_search"] = row["radius1m_ms"] / row["nn_search_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
