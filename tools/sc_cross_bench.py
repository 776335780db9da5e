"""Latency of the cross-database Scan Context calls (include/gorio_sc_cross.h) beside what a caller could do without them.  Two databases
of 4096 keyframes (Q, the query side, and D) and a merged handle M that holds Q's scans and then D's.  Wall time per call through the
Python binding, in ms: host packing, the upload, the launches, the copies back and the one synchronisation.  The forms of a row are
alternated inside one process, in three rounds after a warm-up; every figure is the median of --reps calls and the three rounds are
listed, not averaged.  Prints one JSON line ("sc_cross_bench").

    python tools/sc_cross_bench.py [--reps 5] [--sizes 256 1024 4096]

  top_matches_{n}sq_k{k}        Q.top_matches(D) for rows 0 .. n - 1 against the columns 0 .. n - 1, k = 1, 3, 8
  yardstick_{n}sq_k{k}          M.distance_matrix(rows, 4096 + cols, dist only) followed by numpy.argpartition and a sort of the k picks
                                on the host (k = 1: argmin); yardstick_matrix_{n}sq is the matrix call alone
  triangle_top1_{n} / triangle_best_{n}
                                Q.top_matches(k = 1, col_end = max(0, r - 9)) against Q.best_matches(rows, 10): the same pairs
  cross_matrix_{n}sq / matrix_{n}sq
                                Q.cross_distance_matrix(D, rows, cols) against Q.distance_matrix(rows, cols), dist and shift
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
N_DB = 4096


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return round(float(np.median(ts)) * 1e3, 3)


def _scan(rng, n):
    r = rng.uniform(1, 79, n)
    t = np.deg2rad(rng.uniform(-56, 56, n))
    xyz = np.stack([r * np.cos(t), r * np.sin(t), rng.normal(0, 1, n)], 1).astype(np.float32)
    return xyz, rng.uniform(0, 60, n).astype(np.float32)


def host_top(dist, k):
    """What a caller does with a matrix that came down: the k smallest of every row, in ascending order."""
    if k == 1:
        c = dist.argmin(axis=1)[:, None]
        return c, np.take_along_axis(dist, c, 1)
    part = np.argpartition(dist, k - 1, axis=1)[:, :k]
    d = np.take_along_axis(dist, part, 1)
    o = np.argsort(d, axis=1, kind="stable")
    return np.take_along_axis(part, o, 1), np.take_along_axis(d, o, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024, 4096])
    args = ap.parse_args()
    rng = np.random.default_rng(2)
    q, d, m = gorio.ScanContext(), gorio.ScanContext(), gorio.ScanContext()
    session_q = [_scan(rng, 200) for _ in range(N_DB)]
    session_d = [_scan(rng, 200) for _ in range(N_DB)]
    for h, parts in ((q, [session_q]), (d, [session_d]), (m, [session_q, session_d])):
        for part in parts:
            for lo in range(0, N_DB, 1024):
                h.add_scans(part[lo:lo + 1024])
    forms = {}
    for n in args.sizes:
        idx = np.arange(n, dtype=np.int32)
        ends = np.full(n, n, np.int32)
        tri = np.maximum(0, idx - 9).astype(np.int32)
        forms[f"yardstick_matrix_{n}sq"] = lambda idx=idx: m.distance_matrix(idx, N_DB + idx, want_shift=False)
        for k in (1, 3, 8):
            forms[f"top_matches_{n}sq_k{k}"] = lambda idx=idx, ends=ends, k=k: q.top_matches(d, idx, ends, k)
            forms[f"yardstick_{n}sq_k{k}"] = lambda idx=idx, k=k: host_top(m.distance_matrix(idx, N_DB + idx, want_shift=False)[0], k)
        forms[f"triangle_top1_{n}"] = lambda idx=idx, tri=tri: q.top_matches(None, idx, tri, 1)
        forms[f"triangle_best_{n}"] = lambda idx=idx: q.best_matches(idx, 10)
        forms[f"cross_matrix_{n}sq"] = lambda idx=idx: q.cross_distance_matrix(d, idx, idx)
        forms[f"matrix_{n}sq"] = lambda idx=idx: q.distance_matrix(idx, idx)
    for fn in forms.values():  # warm every shape once before anything is timed
        fn()
    res = {name: [] for name in forms}
    for _ in range(3):
        for name, fn in forms.items():
            res[name].append(_time(fn, args.reps))
    # the same answer from both forms, at the largest size timed (ties aside: the host form does not order them by column)
    n = max(args.sizes)
    idx = np.arange(n, dtype=np.int32)
    got = q.top_matches(d, idx, np.full(n, n, np.int32), 3)
    want = host_top(m.distance_matrix(idx, N_DB + idx, want_shift=False)[0], 3)
    res["same_distances_as_yardstick"] = bool(got[1].tobytes() == want[1].tobytes())
    res["database"] = [q.state()["n_scans"], d.state()["n_scans"], m.state()["n_scans"]]
    res["cross_counters"] = q.cross_counters()
    print(json.dumps({"sc_cross_bench": res}))


if __name__ == "__main__":
    main()
