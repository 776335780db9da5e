#!/usr/bin/env python3
"""Development timing of the pose-graph edge scoring (include/gorio_kf_edges.h) against the routes to the same scores without it; GPU
only (it fails without a device), not wired into bench.py.

The work is the back end's keyframe queue (radar_graph_slam_nodelet.cpp:585-591): `count` odometry edges (keyframe k, keyframe k - 1,
relative pose of their odometry) between count + 1 resident keyframes of --points points each, every keyframe a synthetic radar scan of
one scene from a sensor that moves 0.2 m and turns 0.8 degrees per keyframe.  Three routes to the `count` fitness scores:

  handles        one registration handle per edge, made beforehand (pruned search): per edge the two keyframe hand-offs and
                 gorio_apd_fitness_score -- the recipe of INTEGRATION.md section 2.  count synchronisations.
  handles_batch  the same handles and hand-offs, then ONE gorio_apd_fitness_score_batch (possible here because the sources are distinct).
  edges          ONE gorio_kf_edge_fitness.

Each route is timed twice: "first" = on a fresh store, where the call(s) also build the search index of every keyframe (the store is
made and filled untimed), and "warm" = the same call again on that store.  The routes alternate in one process after a warm-up of every
shape; every timed region ends in a call that synchronises the stream.  Figures: median, min and max over --reps repetitions, host
wall clock, milliseconds per call (= per `count` edges).  The scores of the three routes are compared bit for bit.  One JSON line.

    python tools/edge_bench.py [--reps 20] [--first-reps 5] [--warmup 3] [--points 5000 16384] [--counts 1 8 64]
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
synth = gorio.synth

KW = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)
N_SCANS = 8  # distinct scans; keyframe k is scan k mod N_SCANS (a keyframe of its own on the device all the same)


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "reps": len(t)}


def pose(k):
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0, 0, 0.8 * k])
    T[:3, 3] = [0.2 * k, -0.03 * k, 0.0]
    return T


def fill(scans, count):
    store = gorio.KeyframeStore()
    ids = [store.add(*scans[k % N_SCANS]) for k in range(count + 1)]
    return store, ids


def run_handles(regs, store, edges, batch):
    for g, (tgt, src, _) in zip(regs, edges):
        g.setInputTargetKeyframe(store, tgt)
        g.setInputSourceKeyframe(store, src)
    Ts = [np.asarray(T, np.float64).astype(np.float32) for _, _, T in edges]
    if batch:
        return gorio.fitness_score_batch(regs, Ts)[0]
    return np.array([g.getFitnessScore(T, inlier_dist=0.0)[0] for g, T in zip(regs, Ts)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--first-reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, nargs="+", default=[5000, 16384])
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 8, 64])
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("edge_bench.py needs a GPU: there is nothing to time without one")
    out = {"reps": a.reps, "first_reps": a.first_reps, "warmup": a.warmup, "cases": []}
    regs_all = [gorio.ApdGicp(**KW) for _ in range(max(a.counts))]
    routes = ("handles", "handles_batch", "edges")
    for n in a.points:
        scans = []
        for k in range(N_SCANS):
            xyz, lab = synth.radar_scan(n, seed=900 + k, sensor_pose=pose(k))
            scans.append((xyz, None, lab))
        for count in a.counts:
            regs = regs_all[:count]
            t = {r: {"first": [], "warm": []} for r in routes}
            scores = {}
            counters = None
            for i in range(a.warmup + max(a.reps, a.first_reps)):
                for route in routes:
                    store, ids = fill(scans, count)  # untimed: fresh keyframes, no index
                    # keyframe k is scan k mod N_SCANS seen from pose(k mod N_SCANS): the relative pose of its odometry
                    edges = [(ids[k], ids[k - 1], np.linalg.inv(pose(k % N_SCANS)) @ pose((k - 1) % N_SCANS)) for k in range(1, count + 1)]
                    for phase in ("first", "warm"):
                        reps = a.first_reps if phase == "first" else a.reps
                        t0 = time.perf_counter()
                        if route == "edges":
                            s = store.edge_fitness(edges)[0].copy()
                        else:
                            s = run_handles(regs, store, edges, route == "handles_batch")
                        t1 = time.perf_counter()
                        if a.warmup <= i < a.warmup + reps:
                            t[route][phase].append((t1 - t0) * 1e3)
                    scores[route] = s
                    if route == "edges":
                        counters = store.edge_counters()
                    else:
                        for g in regs:  # let go of the keyframes before the store goes
                            g.clearSource()
                            g.clearTarget()
                    store.close()
            case = {"points": n, "n_edges": count, "scores_equal": bool(np.array_equal(scores["edges"], scores["handles"]) and np.array_equal(scores["edges"], scores["handles_batch"])),
                    "edge_counters_after_two_calls": counters}
            case.update({r: {p: stats(v) for p, v in t[r].items()} for r in routes})
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
