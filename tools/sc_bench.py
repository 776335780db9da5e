"""Latency of the Scan Context ABI (include/gorio_sc.h): adding 1 scan of 5 k points and 256 such scans in one gorio_sc_add_scans,
gorio_sc_detect against 2 k and 20 k candidates, and one gorio_sc_detect_batch of 64 queries of 5 k candidates, over a database of
20 k keyframes.  Wall time per call, host packing and the copies included.  The C++ reference's own time (nanoflann + Eigen) was
not measured, so no speed-up is claimed.  Prints one JSON line.

    python tools/sc_bench.py [--reps 20]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
gorio = importlib.import_module("go-rio_amd")


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def _scan(rng, n):
    r = rng.uniform(1, 79, n)
    t = np.deg2rad(rng.uniform(-56, 56, n))
    xyz = np.stack([r * np.cos(t), r * np.sin(t), rng.normal(0, 1, n)], 1).astype(np.float32)
    return xyz, rng.uniform(0, 60, n).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {}
    one = [_scan(rng, 5000)]
    many = [_scan(rng, 5000) for _ in range(256)]
    sc = gorio.ScanContext()
    res["add_1x5k_ms"] = round(_time(lambda: sc.add_scans(one), args.reps), 3)
    res["add_256x5k_ms"] = round(_time(lambda: sc.add_scans(many), max(args.reps // 4, 3)), 3)
    db = gorio.ScanContext()
    small = [_scan(rng, 200) for _ in range(2500)]
    for _ in range(8):
        db.add_scans(small)
    n_db = db.state()["n_scans"]
    for n_cand in (2000, 20000):
        cand = np.arange(n_cand, dtype=np.int32)
        res[f"detect_{n_cand // 1000}k_candidates_ms"] = round(_time(lambda: db.detect(n_db - 1, cand), args.reps), 3)
    queries = [int(q) for q in rng.choice(np.arange(10000, n_db), 64, replace=False)]
    cands = [np.sort(rng.choice(n_db, 5000, replace=False)).astype(np.int32) for _ in queries]
    res["detect_batch_64x5k_ms"] = round(_time(lambda: db.detect_batch(queries, cands), args.reps), 3)
    res["database"] = n_db
    print(json.dumps({"sc_bench": res}))


if __name__ == "__main__":
    main()
