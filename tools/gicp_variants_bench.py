"""Linearisations per second of the FastGICP / FastVGICP methods on the shapes of bench.py's C4 (64 pairs of 16 384 x 16 384 points) and
C3 (one 16 384-point scan against a 100 000-point local map): Gauss-Newton, 20 fixed iterations, the same synthetic inputs, the same
step as bench.py's scan-matching part (every step re-sets all clouds from HBM-resident buffers, so covariances -- and in VGICP mode the
voxel map -- are rebuilt every step, then ONE gorio_apd_align_batch).  No GP windows run beside it.  Wall-clock around synchronised
steps after warm-up; prints one JSON line per (shape, method) with the per-repeat rates.

    python tools/gicp_variants_bench.py --workload c4 --steps 20 --warmup 5 --repeats 3
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c4", choices=["c4", "c3"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--methods", default="apd,gicp,vgicp1,vgicp7,vgicp27")
    args = ap.parse_args()
    import torch

    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    synth = gorio.synth
    dev = torch.device("cuda", 0)
    n = args.points
    seed0 = synth.BASE_SEED + 3  # bench.py's inputs of rank 0
    if args.workload == "c4":
        pairs = [synth.scan_pair(n, n, seed=seed0 + q) for q in range(args.pairs)]
    else:
        sx, sl = synth.radar_scan(n, seed=seed0)
        tx, tl = synth.local_map(100000, seed=seed0 + 1)
        pairs = [(sx, sl, tx, tl, synth.gt_transform())]

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    resident = [dict(s=[to_dev(p[0][:, 0]), to_dev(p[0][:, 1]), to_dev(p[0][:, 2]), to_dev(p[1])], t=[to_dev(p[2][:, 0]), to_dev(p[2][:, 1]), to_dev(p[2][:, 2]), to_dev(p[3])],
                     n=p[0].shape[0], m=p[2].shape[0]) for p in pairs]
    torch.cuda.synchronize()
    params = dict(corr_dist_threshold=2.0, max_iterations=args.iters, optimizer=0, rotation_epsilon=0.0, transformation_epsilon=0.0, search=1)
    method_of = {"apd": (apd.METHOD_APDGICP, apd.VOXEL_DIRECT1), "gicp": (apd.METHOD_GICP, apd.VOXEL_DIRECT1), "vgicp1": (apd.METHOD_VGICP, apd.VOXEL_DIRECT1),
                 "vgicp7": (apd.METHOD_VGICP, apd.VOXEL_DIRECT7), "vgicp27": (apd.METHOD_VGICP, apd.VOXEL_DIRECT27)}
    for name in args.methods.split(","):
        method, search = method_of[name]
        objs = [gorio.ApdGicp(device=0, **params) for _ in pairs]
        for o in objs:
            o.set_method(method, 1.0, search, apd.VOXEL_ADDITIVE)
        inputs = gorio.DeviceInputs(objs, sources=[([t.data_ptr() for t in r["s"]], r["n"]) for r in resident], targets=[([t.data_ptr() for t in r["t"]], r["m"]) for r in resident])

        def step():
            inputs.apply()
            return sum(r["n_linearize"] for r in gorio.align_batch(objs))

        for _ in range(args.warmup):
            step()
        rates, ms = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lin = 0
            for _ in range(args.steps):
                lin += step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rates.append(lin / dt)
            ms.append(1e3 * dt / args.steps)
        print(json.dumps(dict(workload=args.workload, method=name, unit="linearisations/s", rates=[round(r, 1) for r in rates], ms_per_step=[round(m, 3) for m in ms],
                              pairs=len(pairs), points=n, target_points=int(pairs[0][2].shape[0]), iterations=args.iters, steps=args.steps, warmup=args.warmup)), flush=True)
        del inputs, objs


if __name__ == "__main__":
    main()
