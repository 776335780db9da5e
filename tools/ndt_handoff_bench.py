#!/usr/bin/env python3
"""Development timing of the front end with the default registration (NDT_OMP) fed from the scan pipeline; not wired into bench.py.

One front-end frame = preprocess (ScanPipeline.load + run), give the frame to the registration as its source, align against a keyframe
that is already set, getFitnessScore at the result (a registration handle of gorio_apd.h with the library's default search, as the
drop-in class keeps one).  Two routes over the same messages:

    host      xyz = pipe.output(); ndt.set_source(xyz); fitness handle: setInputSource(xyz)      (download, two uploads)
    handoff   ndt.set_source_from_scan(pipe); fitness handle: setInputSourceFromScan(pipe)       (device-to-device)

The messages are scan_pipeline_restatement.raw_scan of the scan-pipeline profile (10 820 raw points, 9000 ground points): --frames of
them, cycled.  The keyframe is the first message's output.  Every figure is the median (with min and max) of --reps frames after
--warmup untimed ones, wall clock; every stage ends with a stream synchronisation by construction.  --routes host runs on a tree
that has no hand-off yet.  With --scores: N single calculate_score calls against one calculate_score_batch, N handles sharing one
target, for N = 8 and 64.  Prints one JSON line.

    python tools/ndt_handoff_bench.py [--reps 30] [--warmup 5] [--routes host,handoff] [--scores]
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
gorio = importlib.import_module("go-rio_amd")
import scan_pipeline_restatement as sr  # noqa: E402  (scenes only)

ANG_VEL = (0.01, -0.02, 0.15)


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t))}


def frame_main(a, out):
    rot = sr.tilt()
    raws = [sr.raw_scan(200 + k, n_ground=9000, rotation=rot) for k in range(a.frames)]
    params = gorio.prep.scan_default_params(rotation=rot)
    k_ransac = params.reve.n_ransac_points
    routes = a.routes.split(",")
    res = {"n_raw": int(raws[0].shape[0]), "frames": a.frames}
    for route in routes:
        pipe = gorio.prep.ScanPipeline(params)
        ndt = gorio.Ndt(transformation_epsilon=0.01, max_iterations=64)
        fit = gorio.ApdGicp()
        rng = np.random.default_rng(7)

        def preprocess(raw):
            _, nv = pipe.load(raw)
            samples = rng.integers(0, nv, (3, k_ransac)).astype(np.uint32)
            r = pipe.run(samples, ANG_VEL)
            assert r["status"] == "ok"
            return r

        preprocess(raws[0])
        key = pipe.output()
        ndt.set_target(key[0])
        fit.setInputTarget(key[0], key[3])
        names = ("preprocess", "set_source", "align", "fitness", "frame")
        t = {k: [] for k in names}
        n_out, iters = [], []
        for i in range(a.warmup + a.reps):
            raw = raws[(i + 1) % a.frames]
            t0 = time.perf_counter()
            r = preprocess(raw)
            t1 = time.perf_counter()
            if route == "host":
                xyz, _, _, lab = pipe.output()
                ndt.set_source(xyz)
                fit.setInputSource(xyz, lab)
            else:
                ndt.set_source_from_scan(pipe)
                fit.setInputSourceFromScan(pipe)
            t2 = time.perf_counter()
            al = ndt.align()
            t3 = time.perf_counter()
            fit.getFitnessScore(al["T"])
            t4 = time.perf_counter()
            if i >= a.warmup:
                for k, v in zip(names, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                    t[k].append(v * 1e3)
                n_out.append(r["n_out"])
                iters.append(al["n_derivatives"] + al["n_hessians"])
        res[route] = {k: stats(v) for k, v in t.items()}
        res[route].update(n_out_median=float(np.median(n_out)), align_evaluations_median=float(np.median(iters)), counters=pipe.counters())
        ndt.close()
        pipe.close()
    out["frame"] = res


def score_main(a, out):
    sx, _, tx, _, _ = gorio.synth.scan_pair(10240, 10240, seed=1)
    res = {"n_source": int(sx.shape[0]), "n_target": int(tx.shape[0])}
    for count in (8, 64):
        hs = []
        for i in range(count):
            h = gorio.Ndt()
            if i == 0:
                h.set_target(tx)
            else:
                h.set_target_shared(hs[0])
            h.set_source(sx)
            hs.append(h)
        rng = np.random.default_rng(17)
        Ts = []
        for _ in range(count):
            T = np.eye(4, dtype=np.float32)
            T[:3, 3] = rng.uniform(-0.1, 0.1, 3)
            Ts.append(T)
        single, batch = [], []
        for i in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            s1 = [h.calculate_score(T) for h, T in zip(hs, Ts)]
            t1 = time.perf_counter()
            s2 = gorio.ndt.calculate_score_batch(hs, Ts)
            t2 = time.perf_counter()
            if i >= a.warmup:
                single.append((t1 - t0) * 1e3)
                batch.append((t2 - t1) * 1e3)
        res[str(count)] = {"single_calls": stats(single), "one_batch": stats(batch), "equal": bool(np.array_equal(np.array(s1), s2))}
        for h in hs:
            h.close()
    out["scores"] = res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--routes", default="host,handoff")
    ap.add_argument("--scores", action="store_true")
    a = ap.parse_args()
    out = {"reps": a.reps, "warmup": a.warmup}
    if a.routes:
        frame_main(a, out)
    if a.scores:
        score_main(a, out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
