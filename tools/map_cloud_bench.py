#!/usr/bin/env python3
"""Development timing of the map cloud (include/gorio_map.h) against the only route to the same map without it; GPU only (it fails without
a device), not wired into bench.py.

The keyframes are radar-like frames of --points points (16 384, what the scan pipeline puts out for a full message) along a curving
trajectory, 1.3 m apart (tests/map_cloud_restatement.scene); --distinct different frames are uploaded in turn, each under its own pose.
Shapes: every count of --keyframes (100 and 1000) at resolution 0.05 (every shipped launch file) and at resolution 0 (save_map_service
with the raw cloud).  Timed per shape, alternating in one process after a warm-up of every shape:
    generate        gorio_map_generate alone: the map stays on the device (the call ends in a stream synchronise)
    generate_get    gorio_map_generate + gorio_map_get into a preallocated host array: the finished map on the host
    download        gorio_kf_get (xyz and intensity) of every listed keyframe into a preallocated host array: what the host route must do
                    FIRST.  It is a lower bound for that route, not the route: the reference's loop over every point and, with a
                    resolution, its octree still come after it.
Figures: median, min and max of --reps repetitions, wall clock, in ms.  Also printed per shape: the points listed, kept and put out, and
the bytes the gate and scatter kernels must move (20 B read per listed point, twice -- the count pass and the scatter pass read the
point, the scatter pass also its intensity: 16 + 20 -- and 16 B written per kept point), for the bytes/s of a kernel trace.  One JSON line.

    python tools/map_cloud_bench.py [--reps 10] [--warmup 2] [--points 16384] [--keyframes 100 1000] [--distinct 50]
"""
import argparse
import ctypes as C
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
import map_cloud_restatement as mr  # noqa: E402  (scenes only)

RESOLUTIONS = (0.05, 0.0)


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "reps": len(t)}


def ptr(a, offset=0):
    return C.c_void_p(a.__array_interface__["data"][0] + offset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[100, 1000])
    ap.add_argument("--distinct", type=int, default=50)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("map_cloud_bench.py needs a GPU: there is nothing to time without one")
    lib = gorio.load_library()
    n_max = max(a.keyframes)
    distinct = [mr.radar_like_frame(a.points, 1000 + 17 * k) for k in range(min(a.distinct, n_max))]
    store = gorio.KeyframeStore()
    ids = np.array([store.add(*distinct[k % len(distinct)]) for k in range(n_max)], np.int32)
    poses = np.stack([mr.curve_pose(k) for k in range(n_max)]).reshape(n_max, 16)
    mc = gorio.MapCloud()
    host = np.zeros((n_max * a.points, 4), np.float32)  # preallocated: the finished map, or every keyframe one behind the other

    def generate(count, res):
        n = C.c_int(-1)
        rc = lib.gorio_map_generate(mc.h, store.h, ptr(ids), ptr(poses), count, C.c_double(res), C.byref(n))
        assert rc == 0, rc
        return n.value

    def get(n):
        rc = lib.gorio_map_get(mc.h, ptr(host), ptr(host, 12), 16, max(n, 1))
        assert rc == 0, rc

    def download(count):
        off = 0
        for k in range(count):
            rc = lib.gorio_kf_get(store.h, int(ids[k]), ptr(host, 16 * off), ptr(host, 16 * off + 12), None, 16, a.points)
            assert rc == 0, rc
            off += a.points

    shapes = [(count, res) for count in a.keyframes for res in RESOLUTIONS]
    t = {s: {"generate": [], "generate_get": [], "download": []} for s in shapes}
    sizes = {}
    for i in range(a.warmup + a.reps):
        for s in shapes:
            count, res = s
            t0 = time.perf_counter()
            n = generate(count, res)
            t1 = time.perf_counter()
            n = generate(count, res)
            get(n)
            t2 = time.perf_counter()
            download(count)
            t3 = time.perf_counter()
            if i >= a.warmup:
                for k, v in zip(("generate", "generate_get", "download"), (t1 - t0, t2 - t1, t3 - t2)):
                    t[s][k].append(v * 1e3)
            sizes[s] = (n, mc.info())
    out = {"reps": a.reps, "warmup": a.warmup, "points_per_keyframe": a.points, "distinct_frames": len(distinct), "shapes": []}
    for s in shapes:
        n, info = sizes[s]
        row = {"keyframes": s[0], "resolution": s[1], "n_listed": info["n_listed"], "n_kept": info["n_kept"], "n_out": n, "map_bytes_to_host": 16 * n,
               "keyframe_bytes_to_host": 20 * info["n_listed"], "gate_count_bytes": 16 * info["n_listed"], "scatter_bytes": 20 * info["n_listed"] + 16 * info["n_kept"]}
        row.update({k: stats(v) for k, v in t[s].items()})
        out["shapes"].append(row)
    mc.close()
    store.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
