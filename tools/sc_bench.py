"""Latency of the Scan Context ABI (include/gorio_sc.h): adding 1 scan of 5 k points and 256 such scans in one gorio_sc_add_scans,
gorio_sc_detect against 2 k and 20 k candidates, and one gorio_sc_detect_batch of 64 queries of 5 k candidates, over a database of
20 k keyframes.  Wall time per call, host packing and the copies included.  The C++ reference's own time (nanoflann + Eigen) was
not measured, so no speed-up is claimed.  Prints one JSON line.

    python tools/sc_bench.py [--reps 20]

--exhaustive times the four calls of include/gorio_sc_pairs.h instead (one JSON line, "sc_exhaustive_bench"), over a database of 4096
keyframes: gorio_sc_distance_matrix and gorio_sc_best_matches at 256, 1024 and 4096 keyframes squared; gorio_sc_distance_pairs over the
same pairs at 256 and 1024 squared (the listed-pairs kernel against the tile kernel); gorio_sc_detect_exhaustive over the 2000 queries
of a 2000-keyframe session, each with every earlier keyframe as a candidate, beside gorio_sc_detect_batch over the same queries; and
the yardstick of the library without these calls, one gorio_sc_distance call (median of 2000), with the loop over each matrix's pairs
extrapolated from it.  --exhaustive --yardstick-only runs just the two old calls, so a library without the new symbols can be timed.
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


def exhaustive(args):
    rng = np.random.default_rng(2)
    reps = max(args.reps // 4, 3)
    db = gorio.ScanContext()
    for _ in range(4):
        db.add_scans([_scan(rng, 200) for _ in range(1024)])
    res = {"database": db.state()["n_scans"]}
    res["distance_call_us"] = round(_time(lambda: db.distance(100, 3000), 2000) * 1e3, 2)
    n_q = 2000
    queries = list(range(n_q))
    cands = [np.arange(max(q, 1), dtype=np.int32) for q in queries]
    res["session_candidates_total"] = int(sum(max(q - 9, 0) for q in queries if q >= 10))
    res["detect_batch_2000_session_ms"] = round(_time(lambda: db.detect_batch(queries, cands), reps), 3)
    if not args.yardstick_only:
        res["detect_exhaustive_2000_session_ms"] = round(_time(lambda: db.detect_exhaustive(queries, cands), reps), 3)
        for n in (256, 1024, 4096):
            idx = np.arange(n, dtype=np.int32)
            res[f"distance_matrix_{n}sq_ms"] = round(_time(lambda: db.distance_matrix(idx, idx), reps), 3)
            res[f"distance_matrix_{n}sq_dist_only_ms"] = round(_time(lambda: db.distance_matrix(idx, idx, want_shift=False), reps), 3)
            res[f"best_matches_{n}_gap10_ms"] = round(_time(lambda: db.best_matches(idx, 10), reps), 3)
            res[f"distance_loop_{n}sq_extrapolated_ms"] = round(res["distance_call_us"] * n * n * 1e-3, 1)
            if n <= 1024:
                q, c = np.repeat(idx, n), np.tile(idx, n)
                res[f"distance_pairs_{n}sq_ms"] = round(_time(lambda: db.distance_pairs(q, c), reps), 3)
        res["counters"] = db.pairs_counters()
    print(json.dumps({"sc_exhaustive_bench": res}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--exhaustive", action="store_true")
    ap.add_argument("--yardstick-only", action="store_true")
    args = ap.parse_args()
    if args.exhaustive:
        return exhaustive(args)
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
