"""Per-scan latency of gorio_ground_estimate (Patchwork++ ground segmentation, id = 1) on synthetic radar / LiDAR scans of about
3 k, 10 k and 60 k points, of one gorio_ground_estimate_batch over 16 handles, and the LM iterations per plane fit.  The NumPy
restatement's time on the host CPU is printed beside it as a LOWER-QUALITY point of comparison only: the reference's own time (Ceres +
PCL) cannot be measured without those libraries.  Prints one JSON line.

    python tools/ground_bench.py [--reps 20] [--no-restatement]
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
import ground_scenes as gs  # noqa: E402


def _time(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-restatement", action="store_true")
    args = ap.parse_args()
    scenes = {"3k": gs.scan(1), "10k": gs.scan(2, n_ground=8200), "60k": gs.large_scan(3)}
    res = {}
    for name, (xyz, inten) in scenes.items():
        seg = gorio.ground.GroundSegmenter()
        ms = _time(lambda: seg.estimate(xyz, inten, id=1), args.reps)
        dg = seg.diagnostics()
        its = [int(i) for p in dg["patches"] for i in p["lm_iterations"][:p["n_fits"]]]
        r = {"points": int(len(xyz)), "ms_per_scan": round(ms, 3), "fits": len(its), "lm_iterations_mean": round(float(np.mean(its)), 2) if its else 0,
             "lm_iterations_max": max(its) if its else 0, "final_lm_iterations": int(dg["frame"]["final_lm_iterations"])}
        if not args.no_restatement and name != "60k":
            import patchwork_restatement as pr

            t = time.perf_counter()
            pr.Patchworkpp().estimate_ground(xyz, inten, id=1)
            r["numpy_restatement_ms_lower_quality"] = round((time.perf_counter() - t) * 1e3, 1)
        res[name] = r
    clouds = [gs.scan(100 + k) for k in range(16)]
    segs = [gorio.ground.GroundSegmenter() for _ in clouds]
    ms_b = _time(lambda: gorio.ground.estimate_batch(segs, clouds, id=1), args.reps)
    singles = [gorio.ground.GroundSegmenter() for _ in clouds]
    ms_s = _time(lambda: [s.estimate(x, i, id=1) for s, (x, i) in zip(singles, clouds)], args.reps)
    res["batch16_3k"] = {"ms_per_batch": round(ms_b, 3), "ms_per_scan": round(ms_b / 16, 3), "ms_16_single_calls": round(ms_s, 3)}
    print(json.dumps({"ground_bench": res}))


if __name__ == "__main__":
    main()
