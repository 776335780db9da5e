#!/usr/bin/env python3
"""Development timing of NDTCuda (GORIO_METHOD_NDT_CUDA, P2D and D2D) next to FastVGICP on the same clouds; not wired into bench.py.

Workload: synthetic radar scan pairs of go-rio_amd/synth.py at 5 k x 5 k and 16 k x 16 k points, resolution 1.0, DIRECT7 for the NDT modes
and FastVGICP's default DIRECT1, 64 iterations, the LM shell.  Wall clock around calls that end in a stream synchronisation, after --warmup
untimed calls; every handle has aligned before, so maps (and FastVGICP's covariances) are outside the timed region.  Per size and method:
    linearize   one gorio_apd_linearize (descriptor upload, pair / slot kernel, reduction, one copy back)
    align       one gorio_apd_align; its time over its linearisations is the time per iteration of the shell
    map         the voxel map of the target alone: the parity hook's count-only call on a freshly uploaded cloud (two small read-backs inside)
and the loop-closure shape, N = 16 and 64 candidate sources against one shared target: N single aligns against one gorio_apd_align_batch,
with a check that both give the same bits.  One JSON line; --markdown writes the tables.

    python tools/ndt_cuda_bench.py [--reps 15] [--warmup 3] [--sizes 5000 16000] [--counts 16 64] [--markdown out.md]
"""
import argparse
import ctypes as C
import hashlib
import importlib
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def timed(fn, warmup, reps, before=None):
    for _ in range(warmup):
        if before:
            before()
        res = fn()
    t = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        res = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t, res


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), n=len(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16000])
    ap.add_argument("--counts", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    common = dict(max_iterations=64, search=apd.SEARCH_PRUNED)

    def make(method):
        g = gorio.ApdGicp(device=0, **common)
        if method == "vgicp":
            g.set_method(apd.METHOD_VGICP, 1.0, apd.VOXEL_DIRECT1, apd.VOXEL_ADDITIVE)
        else:
            g.set_ndt_cuda_params(apd.NDT_CUDA_P2D if method == "ndt_p2d" else apd.NDT_CUDA_D2D)
            g.set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT7)
        return g

    def voxel_count(g, method):
        n = C.c_int(0)
        if method == "vgicp":
            rc = g._lib.gorio_apd_get_voxelmap(g._h, None, None, None, None, 0, C.byref(n))
        else:
            rc = g._lib.gorio_apd_ndt_cuda_get_voxels(g._h, 1, 0, C.byref(n), None, None, None, None, None)
        assert rc == 0
        return n.value

    methods = ("ndt_p2d", "ndt_d2d", "vgicp")
    out = {"reps": a.reps, "warmup": a.warmup, "sizes": {}, "batches": {}}
    for n in a.sizes:
        src, _, tgt, _, _ = gorio.synth.scan_pair(n, n, seed=1)
        sources = [gorio.synth.radar_scan(n, seed=101 + q)[0] for q in range(max(a.counts))]
        row = {}
        for method in methods:
            g = make(method)
            g.setInputTarget(tgt)
            g.setInputSource(src)
            t, r = timed(lambda: g.align(), a.warmup, a.reps)
            s = stats(t)
            row[method + " align"] = dict(s, units=int(r["n_linearize"]), unit="linearisations", per_unit_us=1e3 * s["median"] / max(1, r["n_linearize"]), converged=bool(r["converged"]))
            t, _ = timed(lambda: g.linearize(np.eye(4)), a.warmup, a.reps)
            s = stats(t)
            row[method + " linearize"] = dict(s, units=1, unit="call", per_unit_us=1e3 * s["median"])
            if method != "ndt_d2d":  # the map build is the same code for both NDT modes
                if method == "vgicp":
                    g.calculateCovariances()
                    cov = g.getTargetCovariances()
                    before = lambda: (g.setInputTarget(tgt), g.setTargetCovariances(cov))  # noqa: E731 -- the map alone: the covariances are supplied
                else:
                    before = lambda: g.setInputTarget(tgt)  # noqa: E731
                t, nv = timed(lambda: voxel_count(g, method), a.warmup, a.reps, before)
                s = stats(t)
                row[("ndt" if method != "vgicp" else "vgicp") + " map"] = dict(s, units=int(nv), unit="voxels", per_unit_us=1e3 * s["median"] / max(1, nv))
            for count in a.counts:
                objs = []
                for q in range(count):
                    o = make(method)
                    if q == 0:
                        o.setInputTarget(tgt)
                    else:
                        o.setInputTargetShared(objs[0])
                    o.setInputSource(sources[q])
                    objs.append(o)
                ts, rs = timed(lambda: [o.align() for o in objs], a.warmup, a.reps)
                tb, rb = timed(lambda: gorio.align_batch(objs), a.warmup, a.reps)
                bits = [hashlib.sha256(b"".join(r["T"].tobytes() for r in res)).hexdigest() for res in (rs, rb)]
                out["batches"]["%d / %d / %s" % (n, count, method)] = dict(single=stats(ts), batch=stats(tb), linearisations=int(sum(r["n_linearize"] for r in rs)),
                                                                         longest=int(max(r["n_linearize"] for r in rs)), converged=int(sum(r["converged"] for r in rs)),
                                                                         same_bits=bits[0] == bits[1])
                del objs
        out["sizes"][str(n)] = row
    print(json.dumps(out))
    if a.markdown:
        def cell(s):
            return "%.3f (%.3f .. %.3f)" % (s["median"], s["min"], s["max"])
        with open(a.markdown, "w") as f:
            f.write("| points | what | call [ms]: median (min .. max) of %d | units per call | time per unit [us] |\n|---|---|---|---|---|\n" % a.reps)
            for n, row in out["sizes"].items():
                for name, s in row.items():
                    f.write("| %s | %s | %s | %d %s | %.2f |\n" % (n, name, cell(s), s["units"], s["unit"], s["per_unit_us"]))
            f.write("\n| points / N / method | N single aligns [ms] | one batch [ms] | single / batch | linearisations summed (longest) | converged | same bits |\n|---|---|---|---|---|---|---|\n")
            for key, c in out["batches"].items():
                f.write("| %s | %s | %s | %.1f | %d (%d) | %d | %s |\n" % (key, cell(c["single"]), cell(c["batch"]), c["single"]["median"] / c["batch"]["median"], c["linearisations"],
                                                                     c["longest"], c["converged"], c["same_bits"]))


if __name__ == "__main__":
    main()
