#!/usr/bin/env python3
"""FastGICPMultiPoints (GORIO_METHOD_GICP_MP) on the GPU: time per align and per stage of its passes (query transform, radius search, merge +
linearise, shell) at 5 k x 5 k and 16 k x 16 k points, and beside them the FastGICP single align of the same clouds from the same build,
for orientation only.  Per-align times are medians over --reps timed aligns after --warmup untimed ones (covariances and the search index
are built by the warm-up; an align re-uses them, as a scan-matching loop does).  The stage split comes from a separate set of aligns with
the handle's profiling on, which drains the stream after every stage, so its stages add up to more than an unprofiled align.  One JSON
line; --markdown writes a table.

--batch N is the loop-closure shape instead: N handles on ONE shared target (covariances and index reused), every handle a source of its
own, timed as one gorio_apd_gicp_mp_align_batch call and as N single aligns one by one, with the batch's rounds, launches and
synchronisations.  A library without the batch call (an older build named by GORIO_AMD_LIB) gives the one-by-one figures alone."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def room_pair(n, seed):
    import icp_scenes as S

    tgt = S.room(n, seed)
    pick = np.random.default_rng(seed + 1).integers(0, n, n)
    src = S.moved(tgt[pick], np.linalg.inv(S.T_TRUE.astype(np.float64)), seed + 2)
    return src, tgt


def batch_mode(a, gorio, apd):
    import icp_scenes as S

    has_batch = hasattr(apd.load_library(), "gorio_apd_gicp_mp_align_batch")
    rows = []
    for n in a.sizes:
        tgt = S.room(n, 40 + n)
        for count in a.batch:
            hs = []
            for q in range(count):
                pick = np.random.default_rng(41 + n + q).integers(0, n, n)
                src = S.moved(tgt[pick], np.linalg.inv(S.T_TRUE.astype(np.float64)), 42 + n + q)
                g = gorio.ApdGicp(k_correspondences=20, regularization=3, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5, search=apd.SEARCH_PRUNED)
                g.set_method(apd.METHOD_GICP_MP)
                if q == 0:
                    g.setInputTarget(tgt)
                else:
                    g.setInputTargetShared(hs[0])
                g.setInputSource(src)
                hs.append(g)

            def timed(fn):
                for _ in range(a.warmup):
                    fn()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    r = fn()
                    ts.append(time.perf_counter() - t0)
                return statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, r

            one = timed(lambda: [g.align() for g in hs])
            row = dict(n=n, count=count, one_by_one_ms=one[0], one_by_one_min_ms=one[1], one_by_one_max_ms=one[2], passes=[r["n_linearize"] for r in one[3]])
            if has_batch:
                b = timed(lambda: apd.gicp_mp_align_batch(hs))
                assert all(x["T"].tobytes() == y["T"].tobytes() for x, y in zip(b[3], one[3])), "the batch and the single aligns differ"
                row.update(batch_ms=b[0], batch_min_ms=b[1], batch_max_ms=b[2], **b[3][0]["batch_diag"])
            rows.append(row)
            del hs
    print(json.dumps(dict(bench="gicp_mp_batch", reps=a.reps, warmup=a.warmup, lib=os.path.basename(gorio.LIB_PATH), rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16384])
    ap.add_argument("--markdown")
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="handles on one shared target: batch call against one by one")
    a = ap.parse_args()
    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    if a.batch:
        return batch_mode(a, gorio, apd)
    rows = []
    for n in a.sizes:
        src, tgt = room_pair(n, 40 + n)

        def timed(g):
            for _ in range(a.warmup):
                g.align()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                r = g.align()
                ts.append(time.perf_counter() - t0)
            return statistics.median(ts), min(ts), max(ts), r

        mp = gorio.ApdGicp(k_correspondences=20, regularization=3, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5, search=apd.SEARCH_PRUNED)
        mp.set_method(apd.METHOD_GICP_MP)
        mp.setInputTarget(tgt)
        mp.setInputSource(src)
        t0 = time.perf_counter()
        mp.gicp_mp_covariances(0)
        mp.gicp_mp_covariances(1)
        t_cov = time.perf_counter() - t0  # first call: k-NN lists, covariances, index, allocations
        med, lo, hi, r = timed(mp)
        d = mp.gicp_mp_diag()
        mp.setProfiling(True)
        s0 = mp.gicp_mp_diag()["stage_seconds"]
        for _ in range(a.reps):
            mp.align()
        s1 = mp.gicp_mp_diag()["stage_seconds"]
        mp.setProfiling(False)
        stages = {k: (s1[k] - s0[k]) / a.reps for k in s1}
        gi = gorio.ApdGicp(k_correspondences=20, regularization=3, max_iterations=64, rotation_epsilon=2e-3, transformation_epsilon=5e-4, search=apd.SEARCH_PRUNED)
        gi.set_method(apd.METHOD_GICP)
        gi.setInputTarget(tgt)
        gi.setInputSource(src)
        gmed, glo, ghi, gr = timed(gi)
        rows.append(dict(n=n, align_ms=med * 1e3, align_min_ms=lo * 1e3, align_max_ms=hi * 1e3, passes=r["n_linearize"], converged=r["converged"], neighbours=d["total"], used=d["used"],
                         first_covariances_ms=t_cov * 1e3, stage_ms={k: v * 1e3 for k, v in stages.items()}, fast_gicp_align_ms=gmed * 1e3, fast_gicp_min_ms=glo * 1e3,
                         fast_gicp_max_ms=ghi * 1e3, fast_gicp_linearisations=gr["n_linearize"]))
    print(json.dumps(dict(bench="gicp_mp", reps=a.reps, warmup=a.warmup, rows=rows)))
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write("| points | align ms (median, min - max) | passes | neighbours of the last pass | query ms | search ms | merge + linearise ms | shell ms | FastGICP align ms (linearisations) |\n")
            f.write("|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                s = r["stage_ms"]
                f.write("| %d x %d | %.3f (%.3f - %.3f) | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f (%d) |\n" % (
                    r["n"], r["n"], r["align_ms"], r["align_min_ms"], r["align_max_ms"], r["passes"], r["neighbours"], s["query"], s["search"], s["linearize"], s["shell"],
                    r["fast_gicp_align_ms"], r["fast_gicp_linearisations"]))


if __name__ == "__main__":
    main()
