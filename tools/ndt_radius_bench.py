#!/usr/bin/env python3
"""Development timing of NDT's radius neighbourhood (gorio_ndt_set_radius_search, include/gorio_ndt.h) against DIRECT7; not wired
into bench.py.

On the shapes of tools/ndt_bench.py (the real LiDAR pair of tests/golden/real_lidar_pair.npz and a 16 384 x 16 384 synthetic radar
pair), on ONE handle and the same clouds, the switch turned over between the two series: milliseconds per derivative evaluation (with
and without the Hessian), per computeHessian, per calculate_score and per align, and the one-off cost of the centroid cloud and its
index.  Every figure is (median, min, max) of --reps timed calls after --warmup untimed ones, wall clock around a call that ends with
a stream synchronisation (an evaluation is one host round trip by construction).  Prints one JSON line.

    python tools/ndt_radius_bench.py [--reps 30] [--warmup 5]

With --batch N: N handles sharing one target, guesses perturbed per handle with a fixed seed, all radius and then all DIRECT7: N serial
aligns against one align_batch, with the batch's stats and the time per round.

    python tools/ndt_radius_bench.py --batch 8

With --loop K: nothing but K radius derivative evaluations on the real pair after the warm-up, for a kernel trace that splits an
evaluation into its query, search and walk launches:

    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/ndt_radius_bench.py --loop 200
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
POSE = np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03])
TYPICAL = dict(transformation_epsilon=0.01, max_iterations=64, search=gorio.ndt.DIRECT7)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def workloads():
    g = np.load(os.path.join(ROOT, "tests", "golden", "real_lidar_pair.npz"))
    T = gorio.synth.gt_transform([0.30, -0.20, 0.05], [0.5, -0.4, 2.0])
    moved = (g["a_1"][:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    yield "real_pair", g["a_0"][:, :3].copy(), moved
    sx, _, tx, _, _ = gorio.synth.scan_pair(16384, 16384, seed=1)
    yield "synthetic_16384", sx, tx


def series(n, reps, warmup):
    r = {}
    r["derivatives_hessian_ms"] = median_ms(lambda: n.derivatives(POSE, True), reps, warmup)
    r["derivatives_no_hessian_ms"] = median_ms(lambda: n.derivatives(POSE, False), reps, warmup)
    r["hessian_only_ms"] = median_ms(lambda: n.hessian(POSE), reps, warmup)
    r["calculate_score_ms"] = median_ms(lambda: n.calculate_score(np.eye(4)), reps, warmup)
    r["align_ms"] = median_ms(lambda: n.align(), reps, warmup)
    res = n.align()
    r["align_evaluations"] = res["n_derivatives"] + res["n_hessians"]
    r["align_ms_per_evaluation"] = r["align_ms"][0] / max(r["align_evaluations"], 1)
    return r


def single_main(a):
    out = {"reps": a.reps, "warmup": a.warmup, "workloads": {}}
    for name, src, tgt in workloads():
        w = {"n_source": int(src.shape[0]), "n_target": int(tgt.shape[0])}
        n = gorio.Ndt(**TYPICAL)
        n.set_source(src)

        def index_build():
            n.set_target(tgt)  # upload + stale map
            n.centroids()      # map build + centroid cloud + its index + read-back

        def map_build():
            n.set_target(tgt)
            n.voxels()

        ib, mb = median_ms(index_build, a.reps, a.warmup), median_ms(map_build, a.reps, a.warmup)
        w["map_and_centroid_index_ms"], w["map_alone_ms"] = ib, mb
        n.set_target(tgt)
        w["n_leaves"], w["n_centroids"] = int(n.voxels()["leaf_index"].size), int(n.centroids()[0].shape[0])
        n.set_radius_search(True)
        w["radius"] = series(n, a.reps, a.warmup)
        n.derivatives(POSE)
        w["neighbours_per_point_mean_max"] = [float(np.diff(n.neighbours()[0]).mean()), int(np.diff(n.neighbours()[0]).max())]
        n.set_radius_search(False)
        w["DIRECT7"] = series(n, a.reps, a.warmup)
        w["radius_over_direct7"] = {k: w["radius"][k][0] / w["DIRECT7"][k][0] for k in ("derivatives_hessian_ms", "derivatives_no_hessian_ms", "align_ms")}
        n.close()
        out["workloads"][name] = w
    print(json.dumps(out))


def batch_main(a):
    rng = np.random.default_rng(17)
    guesses = []
    for _ in range(a.batch):
        G = np.eye(4, dtype=np.float32)
        ang = np.deg2rad(rng.uniform(-1.0, 1.0))
        G[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]
        G[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        guesses.append(G)
    out = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "workloads": {}}
    for name, src, tgt in workloads():
        w = {"n_source": int(src.shape[0]), "n_target": int(tgt.shape[0])}
        hs = []
        for i in range(a.batch):
            n = gorio.Ndt(**TYPICAL)
            if i == 0:
                n.set_target(tgt)
            else:
                n.set_target_shared(hs[0])
            n.set_source(src)
            hs.append(n)
        for mode, on in (("radius", True), ("DIRECT7", False)):
            for n in hs:
                n.set_radius_search(on)
            r = {"serial_ms": median_ms(lambda: [n.align(g) for n, g in zip(hs, guesses)], a.reps, a.warmup),
                 "batch_ms": median_ms(lambda: gorio.ndt.align_batch(hs, guesses), a.reps, a.warmup)}
            _, st = gorio.ndt.align_batch(hs, guesses)
            r["stats"] = {"rounds": st.rounds, "evaluations": st.evaluations, "launches": st.launches}
            r["batch_ms_per_round"] = r["batch_ms"][0] / max(st.rounds, 1)
            w[mode] = r
        for n in hs:
            n.close()
        out["workloads"][name] = w
    print(json.dumps(out))


def loop_main(a):
    _, src, tgt = next(workloads())
    n = gorio.Ndt(radius_search=True, **TYPICAL)
    n.set_target(tgt)
    n.set_source(src)
    for _ in range(a.warmup + a.loop):
        n.derivatives(POSE, True)
    n.close()
    print(json.dumps({"loop": a.loop, "warmup": a.warmup, "n_source": int(src.shape[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="N sharing handles: N serial aligns against one align_batch, radius and DIRECT7")
    ap.add_argument("--loop", type=int, default=0, help="only K radius derivative evaluations on the real pair (for a kernel trace)")
    a = ap.parse_args()
    if a.loop > 0:
        return loop_main(a)
    if a.batch > 0:
        return batch_main(a)
    return single_main(a)


if __name__ == "__main__":
    main()
