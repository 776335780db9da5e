#!/usr/bin/env python3
"""Development timing of ICP (GORIO_METHOD_ICP) next to FAST_GICP and GICP_OMP on the same clouds; not wired into bench.py.

Workload: synthetic radar scan pairs of go-rio_amd/synth.py at 5 k x 5 k and 16 k x 16 k points, pruned search, the parameters
registrations.cpp ships for each method (transformation epsilon 0.01, 64 iterations, 2.5 m; k = 20 and 20 optimizer iterations where they
apply).  Wall clock around calls that end in a stream synchronisation, after --warmup untimed calls; search indices and covariances are
outside the timed region (every handle has aligned before).  Per size:
    icp / icp_recip   one align; its time over its correspondence passes is the time per ICP iteration
    icp_step          one gorio_apd_icp_step (search, pairs, fold, one copy back)
    fast_gicp         one align (Gauss-Newton / LM loop on the device); time over its linearisations
    gicp_omp          one align; time over its round trips (evaluations + updates)
    gicp_omp_update   one gorio_apd_gicp_omp_update (search, update, one copy back): the pass an ICP iteration is compared with
and the loop-closure shape, N = 16 and 64 candidate sources against one shared target: N single ICP aligns against one
gorio_apd_icp_align_batch, with a check that both give the same bits.  One JSON line; --markdown writes the tables.

    python tools/icp_time.py [--reps 7] [--warmup 2] [--sizes 5000 16000] [--counts 16 64] [--markdown out.md]
"""
import argparse
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def guesses(count, seed=17):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        G = np.eye(4, dtype=np.float32)
        a = np.deg2rad(rng.uniform(-1.0, 1.0))
        G[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        G[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        out.append(G)
    return np.stack(out)


def timed(fn, warmup, reps):
    for _ in range(warmup):
        res = fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t, res


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), n=len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16000])
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    common = dict(max_iterations=64, transformation_epsilon=0.01, corr_dist_threshold=2.5, search=apd.SEARCH_PRUNED)

    def icp(recip=False):
        g = gorio.ApdGicp(device=0, **common)
        g.set_method(apd.METHOD_ICP)
        g.set_icp_params(recip)
        return g

    out = {"reps": a.reps, "warmup": a.warmup, "sizes": {}, "batches": {}}
    for n in a.sizes:
        src, _, tgt, _, _ = gorio.synth.scan_pair(n, n, seed=1)
        row = {}

        def put(name, t, units, what):
            s = stats(t)
            row[name] = dict(s, units=int(units), unit=what, per_unit_us=1e3 * s["median"] / max(1, units))

        for name, recip in (("icp", False), ("icp_recip", True)):
            g = icp(recip)
            g.setInputTarget(tgt)
            g.setInputSource(src)
            t, r = timed(lambda: g.align(), a.warmup, a.reps)
            put(name, t, r["n_linearize"], "correspondence passes")
            row[name]["converged"] = bool(r["converged"])
            if not recip:
                t, _ = timed(lambda: g.icp_step(np.eye(4, dtype=np.float32)), a.warmup, a.reps)
                put("icp_step", t, 1, "pass")
        g = gorio.ApdGicp(device=0, k_correspondences=20, **common)
        g.set_method(apd.METHOD_GICP)
        g.setInputTarget(tgt)
        g.setInputSource(src)
        t, r = timed(lambda: g.align(), a.warmup, a.reps)
        put("fast_gicp", t, r["n_linearize"], "linearisations")
        g = gorio.ApdGicp(device=0, k_correspondences=20, rotation_epsilon=2e-3, **common)
        g.set_method(apd.METHOD_GICP_OMP)
        g.setGicpOmpParams(1e-3, 20)
        g.setInputTarget(tgt)
        g.setInputSource(src)
        t, r = timed(lambda: g.align(), a.warmup, a.reps)
        put("gicp_omp", t, r["n_linearize"] + r["nr_iterations"], "evaluations + updates")
        t, _ = timed(lambda: g.gicpOmpUpdate(np.eye(4, dtype=np.float32)), a.warmup, a.reps)
        put("gicp_omp_update", t, 1, "pass")
        out["sizes"][str(n)] = row
        sources = [gorio.synth.radar_scan(n, seed=101 + q)[0] for q in range(max(a.counts))]
        for count in a.counts:
            G = guesses(count)
            objs = []
            for q in range(count):
                g = icp()
                if q == 0:
                    g.setInputTarget(tgt)
                else:
                    g.setInputTargetShared(objs[0])
                g.setInputSource(sources[q])
                objs.append(g)
            ts, rs = timed(lambda: [g.align(G[q]) for q, g in enumerate(objs)], a.warmup, a.reps)
            tb, rb = timed(lambda: gorio.icp_align_batch(objs, G), a.warmup, a.reps)
            bits = [hashlib.sha256(b"".join(r["T"].tobytes() for r in res)).hexdigest() for res in (rs, rb)]
            out["batches"]["%d/%d" % (n, count)] = dict(single=stats(ts), batch=stats(tb), rounds=rb[0]["batch_diag"]["rounds"], launches=rb[0]["batch_diag"]["launches"],
                                                       passes=int(sum(r["n_linearize"] for r in rs)), longest=int(max(r["n_linearize"] for r in rs)),
                                                       converged=int(sum(r["converged"] for r in rs)), same_bits=bits[0] == bits[1])
            del objs
    print(json.dumps(out))
    if a.markdown:
        def cell(s):
            return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
        with open(a.markdown, "w") as f:
            f.write("| points | what | call [ms]: median (min .. max) | units per call | time per unit [us] |\n|---|---|---|---|---|\n")
            for n, row in out["sizes"].items():
                for name, s in row.items():
                    f.write("| %s | %s | %s | %d %s | %.1f |\n" % (n, name, cell(s), s["units"], s["unit"], s["per_unit_us"]))
            f.write("\n| points / N | N single aligns [ms] | one batch [ms] | single / batch | rounds | launches | passes summed (longest) | converged | same bits |\n|---|---|---|---|---|---|---|---|---|\n")
            for key, c in out["batches"].items():
                f.write("| %s | %s | %s | %.1f | %d | %d | %d (%d) | %d | %s |\n" % (key, cell(c["single"]), cell(c["batch"]), c["single"]["median"] / c["batch"]["median"], c["rounds"], c["launches"],
                                                                                 c["passes"], c["longest"], c["converged"], c["same_bits"]))


if __name__ == "__main__":
    main()
