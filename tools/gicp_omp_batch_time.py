#!/usr/bin/env python3
"""Development timing of batched GICP_OMP aligns (gorio_apd_gicp_omp_align_batch); not wired into bench.py.

Workload: the loop-closure shape on synthetic radar scans of go-rio_amd/synth.py -- one target shared by N candidate sources (N other
scans of the same scene), N = 1, 4, 16, 64, at 5 k x 5 k and 16 k x 16 k points, pruned search, the parameters registrations.cpp:91-100
ships (transformation epsilon 0.01, 64 iterations, 2.5 m, k = 20, 20 optimizer iterations), guesses perturbed per candidate with a fixed
seed.  Two timings per (size, N), wall clock around calls that end in a stream synchronisation, after --warmup untimed passes:
    single   N consecutive align() calls, one per handle
    batch    one gicp_omp_align_batch over the N handles (only where the package has it)
Covariances and search indices are outside the timed region (every handle has aligned once before).

A build can only be compared with another build in another process.  Without --worker the tool starts workers one after the other,
alternating between this tree and, with --baseline ROOT, another checkout of the repository (the parent commit, built), --rounds times
each, and prints one JSON line: per (size, N) the median and the min / max over all timed calls of every kind, the medians of the single
rounds (the run-to-run spread), the rounds of a batch, and whether all poses are the same bits in every worker.

    python tools/gicp_omp_batch_time.py [--baseline /path/to/parent/checkout] [--reps 7] [--warmup 2] [--rounds 2] [--markdown out.md]
"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (5000, 16000)
COUNTS = (1, 4, 16, 64)


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


def worker(a):
    sys.path.insert(0, a.root)
    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    has_batch = hasattr(gorio, "gicp_omp_align_batch")
    out = {"root": a.root, "has_batch": has_batch, "cases": {}}
    for n in a.sizes:
        _, _, tgt, _, _ = gorio.synth.scan_pair(n, n, seed=1)
        sources = [gorio.synth.radar_scan(n, seed=101 + q)[0] for q in range(max(a.counts))]
        for count in a.counts:
            G = guesses(count)
            objs = []
            for q in range(count):
                g = gorio.ApdGicp(device=0, k_correspondences=20, max_iterations=64, transformation_epsilon=0.01, rotation_epsilon=2e-3, corr_dist_threshold=2.5,
                                  search=apd.SEARCH_PRUNED)
                g.set_method(apd.METHOD_GICP_OMP)
                g.setGicpOmpParams(1e-3, 20)
                if q == 0:
                    g.setInputTarget(tgt)
                else:
                    g.setInputTargetShared(objs[0])
                g.setInputSource(sources[q])
                objs.append(g)

            def single():
                return [g.align(G[q]) for q, g in enumerate(objs)]

            def batch():
                return gorio.gicp_omp_align_batch(objs, G)

            case = {}
            for kind, fn in (("single", single), ("batch", batch)):
                if kind == "batch" and not has_batch:
                    continue
                for _ in range(a.warmup):
                    res = fn()
                t = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    res = fn()
                    t.append((time.perf_counter() - t0) * 1e3)
                case[kind + "_ms"] = t
                case[kind + "_bits"] = hashlib.sha256(b"".join(r["T"].tobytes() for r in res)).hexdigest()
                case[kind + "_evaluations"] = [int(r["n_linearize"]) for r in res]
                case[kind + "_outer"] = [int(r["nr_iterations"]) for r in res]
                if kind == "batch":
                    case["rounds"] = res[0]["batch_diag"]["rounds"]
                    case["launches"] = res[0]["batch_diag"]["launches"]
            out["cases"]["%d/%d" % (n, count)] = case
            del objs
    print(json.dumps(out))


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), n=len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--counts", type=int, nargs="+", default=list(COUNTS))
    ap.add_argument("--timeout", type=int, default=420, help="seconds one worker may take")
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    roots = [("new", a.root)] + ([("parent", a.baseline)] if a.baseline else [])
    runs = {name: [] for name, _ in roots}
    for _ in range(a.rounds):
        for name, root in roots:  # alternating: whatever else the machine does hits both builds alike
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--reps", str(a.reps), "--warmup", str(a.warmup), "--sizes"] + [str(s) for s in a.sizes]
            cmd += ["--counts"] + [str(c) for c in a.counts]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            sys.stderr.write("worker %s: exit status %d after %.0f s\n" % (name, r.returncode, time.perf_counter() - t0))
            sys.stderr.flush()
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit("worker %s failed with exit status %d: nothing more is started" % (name, r.returncode))
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"reps": a.reps, "warmup": a.warmup, "rounds": a.rounds, "cases": {}}
    same_bits = True
    for key in runs["new"][0]["cases"]:
        c = {}
        bits = set()
        for name in runs:
            for kind in ("single", "batch"):
                per_run = [r["cases"][key][kind + "_ms"] for r in runs[name] if kind + "_ms" in r["cases"][key]]
                if not per_run:
                    continue
                c["%s_%s" % (name, kind)] = dict(stats(np.concatenate(per_run)), run_medians=[float(np.median(t)) for t in per_run])
                bits.update(r["cases"][key][kind + "_bits"] for r in runs[name])
        first = runs["new"][0]["cases"][key]
        c.update(rounds=first.get("rounds"), launches=first.get("launches"), evaluations=first["single_evaluations"], outer=first["single_outer"], same_bits=len(bits) == 1)
        same_bits = same_bits and len(bits) == 1
        out["cases"][key] = c
    out["same_bits_everywhere"] = same_bits
    print(json.dumps(out))
    if a.markdown:
        kinds = [k for k in ("parent_single", "new_single", "new_batch") if any(k in c for c in out["cases"].values())]
        with open(a.markdown, "w") as f:
            f.write("| points / N | " + " | ".join("%s ms: median (min .. max) [run medians]" % k for k in kinds) + " | rounds | longest member (evaluations + outer) | same bits |\n")
            f.write("|---|" + "---|" * (len(kinds) + 3) + "\n")
            for key, c in out["cases"].items():
                cells = []
                for k in kinds:
                    s = c.get(k)
                    cells.append("-" if s is None else "%.2f (%.2f .. %.2f) [%s]" % (s["median"], s["min"], s["max"], ", ".join("%.2f" % m for m in s["run_medians"])))
                longest = max(e + o for e, o in zip(c["evaluations"], c["outer"]))
                f.write("| %s | %s | %s | %d | %s |\n" % (key, " | ".join(cells), c["rounds"], longest, c["same_bits"]))


if __name__ == "__main__":
    main()
