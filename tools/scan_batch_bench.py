#!/usr/bin/env python3
"""Batched scan pipeline against the single calls (include/gorio_scan_batch.h): in ONE process, over the same handles and messages,
alternate "N gorio_scan_load + gorio_scan_run pairs" and "one gorio_scan_load_batch + gorio_scan_run_batch", for N = 1, 8, 64 and both
outlier filters.  The scene is that of profiles/r05/scan_pipeline.md: scan_pipeline_restatement.raw_scan, 10 820 raw points, the
nodelet's default parameters, deskew on.  Three warm-up rounds, then --reps timed rounds (at least 10); prints one JSON line per
(method, N) with the median and min - max in milliseconds per batch and per scan and the scan_batch_diag figures.

    python tools/scan_batch_bench.py [--reps 12] [--counts 1,8,64] [--methods statistical,radius] [--mode both|batch]

--mode batch makes no single call at all (the samples are drawn after a gorio_scan_load_batch): for a kernel trace of the batch alone.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

ANG_VEL = (0.01, -0.02, 0.15)


def _stats(v):
    v = np.sort(np.asarray(v)) * 1e3
    return dict(median=round(float(np.median(v)), 3), min=round(float(v[0]), 3), max=round(float(v[-1]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--methods", default="statistical,radius")
    ap.add_argument("--mode", choices=("both", "batch"), default="both")
    a = ap.parse_args()
    reps = max(a.reps, 10)
    import scan_pipeline_restatement as sr

    gorio = importlib.import_module("go-rio_amd")
    prep = gorio.prep
    scenes = [sr.raw_scan(seed) for seed in (1, 2, 3)]
    for method, name in ((prep.OUTLIER_STATISTICAL, "statistical"), (prep.OUTLIER_RADIUS, "radius")):
        if name not in a.methods.split(","):
            continue
        for count in [int(c) for c in a.counts.split(",")]:
            pipes = [prep.ScanPipeline(prep.scan_default_params(outlier_method=method)) for _ in range(count)]
            raws = [scenes[i % len(scenes)] for i in range(count)]
            rng = np.random.default_rng(7)
            ws = [ANG_VEL] * count
            if a.mode == "batch":
                nvs = prep.scan_load_batch(pipes, raws)[1]
            else:
                nvs = [p.load(r)[1] for p, r in zip(pipes, raws)]
            samples = [rng.integers(0, nv, (3, 5)).astype(np.uint32) for nv in nvs]  # drawn once from the counts of valid targets, the same for both sides
            if a.mode == "batch":
                prep.scan_run_batch(pipes, samples, ws)
            else:
                for p, s in zip(pipes, samples):
                    p.run(s, ANG_VEL)
            t_single, t_batch, t_load, t_run = [], [], [], []
            for rep in range(a.warmup + reps):
                t0 = time.perf_counter()
                for p, r, s in zip(pipes, raws, samples):
                    if a.mode == "both":
                        p.load(r)
                        p.run(s, ANG_VEL)
                t1 = time.perf_counter()
                prep.scan_load_batch(pipes, raws)
                t2 = time.perf_counter()
                res = prep.scan_run_batch(pipes, samples, ws)
                t3 = time.perf_counter()
                assert all(x["status"] == "ok" for x in res)
                if rep >= a.warmup:
                    t_single.append(t1 - t0)
                    t_batch.append(t3 - t1)
                    t_load.append(t2 - t1)
                    t_run.append(t3 - t2)
            diag = prep.scan_batch_diag(pipes[0])
            out = dict(outlier=name, count=count, reps=reps, raw_points=int(raws[0].shape[0]), single_ms=_stats(t_single), batch_ms=_stats(t_batch), load_batch_ms=_stats(t_load),
                       run_batch_ms=_stats(t_run), single_ms_per_scan=round(_stats(t_single)["median"] / count, 3), batch_ms_per_scan=round(_stats(t_batch)["median"] / count, 3),
                       run_batch_diag=diag)
            print(json.dumps(out), flush=True)
            for p in pipes:
                p.close()


if __name__ == "__main__":
    main()
