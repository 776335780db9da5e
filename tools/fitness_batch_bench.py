"""Time of scoring N C4-shaped pairs (16 384 x 16 384 synthetic radar points, pruned search, scored at the ground-truth pose):
N single gorio_apd_fitness_score calls against ONE gorio_apd_fitness_score_batch.  The search indices are built by a warm-up pass, as
they would be after the aligns of a loop-closure check; both paths then do the same searches.  Prints one JSON line.

    python tools/fitness_batch_bench.py [--pairs 64] [--points 16384] [--reps 20] [--search pruned|brute]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
gorio = importlib.import_module("go-rio_amd")
synth = gorio.synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--search", choices=["pruned", "brute"], default="pruned")
    args = ap.parse_args()
    search = 1 if args.search == "pruned" else 0
    objs, Ts = [], []
    for q in range(args.pairs):
        sx, sl, tx, tl, T = synth.scan_pair(args.points, args.points, seed=synth.BASE_SEED + 3 + q)
        g = gorio.ApdGicp(corr_dist_threshold=2.0, search=search)
        g.setInputTarget(tx, tl)
        g.setInputSource(sx, sl)
        objs.append(g)
        Ts.append(T.astype(np.float32))
    Ts = np.stack(Ts)

    def singles():
        return [o.getFitnessScore(Ts[q], inlier_dist=0.0) for q, o in enumerate(objs)]

    def batch():
        return gorio.fitness_score_batch(objs, Ts)

    ref = singles()  # warm-up: search indices, buffers, code objects
    s, f = batch()
    assert all(s[q] == ref[q][0] and f[q] == ref[q][1] for q in range(args.pairs)), "batch differs from the single calls"
    t_single, t_batch = [], []
    for _ in range(args.reps):  # interleaved, so that clock drift hits both alike
        t0 = time.perf_counter()
        singles()
        t1 = time.perf_counter()
        batch()
        t2 = time.perf_counter()
        t_single.append(t1 - t0)
        t_batch.append(t2 - t1)
    ms_single, ms_batch = 1e3 * float(np.median(t_single)), 1e3 * float(np.median(t_batch))
    print(json.dumps(dict(pairs=args.pairs, points=args.points, search=args.search, reps=args.reps,
                          single_calls_ms=round(ms_single, 4), batch_ms=round(ms_batch, 4),
                          single_ms_per_score=round(ms_single / args.pairs, 4), batch_ms_per_score=round(ms_batch / args.pairs, 4),
                          speedup=round(ms_single / ms_batch, 3),
                          single_ms_min=round(1e3 * min(t_single), 4), batch_ms_min=round(1e3 * min(t_batch), 4))))


if __name__ == "__main__":
    main()
