#!/usr/bin/env python3
"""Development timing of NDT_OMP on the GPU (include/gorio_ndt.h); not wired into bench.py.

Milliseconds per voxel-map build, per derivative evaluation (with and without the Hessian) and per align, on the real LiDAR pair of
tests/golden/real_lidar_pair.npz and on a 16 384 x 16 384 synthetic radar pair, for DIRECT1 / 7 / 26.  Every figure is the median of
--reps timed calls after --warmup untimed ones, wall clock around a call that ends with a stream synchronisation (each evaluation is
one host round trip by construction).  Prints one JSON line.

    python tools/ndt_bench.py [--reps 30] [--warmup 5]

With --batch N: N handles on the same two workloads, the guesses perturbed per handle with a fixed seed (up to 0.1 m per axis and
1 degree of yaw), and per search three timings of the same N aligns: N serial align calls on handles with private targets, N serial
align calls on handles that share one target, and one align_batch on the sharing handles (with its stats).  The map builds are outside
the timed region in all three (every handle has aligned once before).

    python tools/ndt_bench.py --batch 16 [--reps 30] [--warmup 5]
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
SEARCHES = {"DIRECT1": gorio.ndt.DIRECT1, "DIRECT7": gorio.ndt.DIRECT7, "DIRECT26": gorio.ndt.DIRECT26}


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


def batch_guesses(count, seed=17):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        G = np.eye(4, dtype=np.float32)
        a = np.deg2rad(rng.uniform(-1.0, 1.0))
        G[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        G[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        out.append(G)
    return out


def batch_main(a):
    out = {"batch": a.batch, "reps": a.reps, "warmup": a.warmup, "workloads": {}}
    guesses = batch_guesses(a.batch)
    for name, src, tgt in workloads():
        w = {"n_source": int(src.shape[0]), "n_target": int(tgt.shape[0])}
        private, shared = [], []
        for i in range(a.batch):
            n = gorio.Ndt(transformation_epsilon=0.01, max_iterations=64)
            n.set_target(tgt)
            n.set_source(src)
            private.append(n)
            m = gorio.Ndt(transformation_epsilon=0.01, max_iterations=64)
            if i == 0:
                m.set_target(tgt)
            else:
                m.set_target_shared(shared[0])
            m.set_source(src)
            shared.append(m)
        for sname, s in SEARCHES.items():
            for n in private + shared:
                n.set_params(search=s)
            r = {}
            r["serial_private_ms"] = median_ms(lambda: [n.align(g) for n, g in zip(private, guesses)], a.reps, a.warmup)
            r["serial_shared_ms"] = median_ms(lambda: [n.align(g) for n, g in zip(shared, guesses)], a.reps, a.warmup)
            r["batch_shared_ms"] = median_ms(lambda: gorio.ndt.align_batch(shared, guesses), a.reps, a.warmup)
            res, st = gorio.ndt.align_batch(shared, guesses)
            r["stats"] = {"rounds": st.rounds, "evaluations": st.evaluations, "launches": st.launches}
            r["serial_over_batch"] = r["serial_private_ms"][0] / r["batch_shared_ms"][0]
            r["equal_to_serial"] = all(np.array_equal(x["T"], n.align(g)["T"]) for x, n, g in zip(res, private, guesses))
            w[sname] = r
        for n in private + shared:
            n.close()
        out["workloads"][name] = w
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0, help="N handles: N serial aligns (private / shared target) against one align_batch")
    a = ap.parse_args()
    if a.batch > 0:
        return batch_main(a)
    out = {"reps": a.reps, "warmup": a.warmup, "workloads": {}}
    p = np.array([0.12, -0.08, 0.03, 0.01, -0.02, 0.03])
    for name, src, tgt in workloads():
        w = {"n_source": int(src.shape[0]), "n_target": int(tgt.shape[0])}
        n = gorio.Ndt(transformation_epsilon=0.01, max_iterations=64)
        n.set_source(src)

        def build():
            n.set_target(tgt)  # upload + stale map
            n.voxels()         # map build + read-back of the leaves

        def upload():
            n.set_target(tgt)

        b, u = median_ms(build, a.reps, a.warmup), median_ms(upload, a.reps, a.warmup)
        w["map_build_ms"] = {"median_with_upload_and_readback": b[0], "min": b[1], "max": b[2], "upload_alone_median": u[0]}
        n.set_target(tgt)
        w["n_leaves"] = int(n.voxels()["leaf_index"].size)
        for sname, s in SEARCHES.items():
            n.set_params(search=s)
            r = {}
            r["derivatives_hessian_ms"] = median_ms(lambda: n.derivatives(p, True), a.reps, a.warmup)
            r["derivatives_no_hessian_ms"] = median_ms(lambda: n.derivatives(p, False), a.reps, a.warmup)
            r["hessian_only_ms"] = median_ms(lambda: n.hessian(p), a.reps, a.warmup)
            r["align_ms"] = median_ms(lambda: n.align(), a.reps, a.warmup)
            res = n.align()
            r["align_evaluations"] = res["n_derivatives"] + res["n_hessians"]
            r["align_iterations"] = res["nr_iterations"]
            w[sname] = r
        n.close()
        out["workloads"][name] = w
    print(json.dumps(out))


if __name__ == "__main__":
    main()
