#!/usr/bin/env python3
"""Development timing of FastVGICPCuda (GORIO_METHOD_VGICP_CUDA) next to the handle's FastVGICP on the same clouds; not wired into bench.py.

Workload: synthetic radar scan pairs of go-rio_amd/synth.py at 5 k x 5 k and 16 k x 16 k points, resolution 1.0, k = 20, PLANE, the RBF
kernel 0.5 / 3.0, 64 iterations, the LM shell.  Wall clock around calls that end in a stream synchronisation, after --warmup untimed
calls.  Per size, the stages of ONE cloud (the target), each timed through the count-only call of the parity hook after an untimed step
that makes exactly that stage stale:
    fresh k-NN      a freshly uploaded cloud to its kept points: search index, lists, covariance, regularise + compaction
    k-NN + cov      the same with the index already built (the untimed step switches to the RBF mode and back): lists, covariance,
                    regularise + compaction
    RBF             the O(N^2) pass, its fold, regularise + compaction (the untimed step changes the kernel width in a bit the float
                    conversion drops)
    regularise      regularise + compaction alone (the untimed step switches the regularisation and back)
    map             the voxel map of the kept points alone (the untimed step switches the resolution and back)
    FastVGICP cov   gorio_apd_calculate_covariances of the same handle in FastVGICP mode: BOTH clouds, search indices included
then one linearise and one align per method and neighbourhood with everything built, and N single aligns against one
gorio_apd_align_batch on a shared target, with a check that both give the same bits.  One JSON line; --markdown writes the tables.

    python tools/vgicp_cuda_bench.py [--reps 10] [--warmup 2] [--sizes 5000 16000] [--counts 64] [--markdown out.md]
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16000])
    ap.add_argument("--counts", type=int, nargs="+", default=[64])
    ap.add_argument("--markdown", default=None)
    a = ap.parse_args()
    gorio = importlib.import_module("go-rio_amd")
    apd = importlib.import_module("go-rio_amd.apd")
    common = dict(max_iterations=64, search=apd.SEARCH_PRUNED)
    PLANE, MIN_EIG = 3, 1

    def make(method, search):
        g = gorio.ApdGicp(device=0, **common)
        if method == "vgicp":
            g.set_method(apd.METHOD_VGICP, 1.0, search, apd.VOXEL_ADDITIVE)
        else:
            g.set_vgicp_cuda_params(apd.NN_GPU_RBF_KERNEL if method == "vgicp_cuda_rbf" else apd.NN_CPU_PARALLEL_KDTREE, 0.5, 3.0)
            g.set_method(apd.METHOD_VGICP_CUDA, 1.0, search)
        return g

    def kept(g):
        n, k = C.c_int(0), C.c_int(0)
        assert g._lib.gorio_apd_vgicp_cuda_get_points(g._h, 1, 0, C.byref(n), None, C.byref(k), None, None) == 0
        return k.value

    def voxels(g):
        n = C.c_int(0)
        assert g._lib.gorio_apd_vgicp_cuda_get_voxels(g._h, 0, C.byref(n), None, None, None, None) == 0
        return n.value

    out = {"reps": a.reps, "warmup": a.warmup, "sizes": {}, "batches": {}}
    for n in a.sizes:
        src, _, tgt, _, _ = gorio.synth.scan_pair(n, n, seed=1)
        sources = [gorio.synth.radar_scan(n, seed=101 + q)[0] for q in range(max(a.counts))]
        row = {}
        g = make("vgicp_cuda", apd.VOXEL_DIRECT1)
        g.setInputSource(src)

        def stage(name, before, fn=kept, unit="kept points"):
            t, r = timed(lambda: fn(g), a.warmup, a.reps, before)
            s = stats(t)
            row[name] = dict(s, units=int(r), unit=unit, per_unit_us=1e3 * s["median"] / max(1, r))

        stage("fresh k-NN: index + lists + cov + regularise", lambda: g.setInputTarget(tgt))
        stage("k-NN lists + cov + regularise", lambda: (g.set_vgicp_cuda_params(apd.NN_GPU_RBF_KERNEL, 0.5, 3.0), kept(g), g.set_vgicp_cuda_params(apd.NN_CPU_PARALLEL_KDTREE, 0.5, 3.0)))
        g.set_vgicp_cuda_params(apd.NN_GPU_RBF_KERNEL, 0.5, 3.0)
        flip = [0]

        def new_width():
            flip[0] ^= 1
            g.set_vgicp_cuda_params(apd.NN_GPU_RBF_KERNEL, 0.5 + 1e-12 * flip[0], 3.0)  # another double, the same float: the same work again

        stage("RBF cov + regularise", new_width)
        stage("regularise + compaction", lambda: (g.set_params(regularization=MIN_EIG), kept(g), g.set_params(regularization=PLANE)))
        voxels(g)
        stage("map of the kept points", lambda: (g.set_method(apd.METHOD_VGICP_CUDA, 1.001, apd.VOXEL_DIRECT1), voxels(g), g.set_method(apd.METHOD_VGICP_CUDA, 1.0, apd.VOXEL_DIRECT1)),
              voxels, "voxels")
        v = make("vgicp", apd.VOXEL_DIRECT1)
        t, _ = timed(lambda: v.calculateCovariances(), a.warmup, a.reps, lambda: (v.setInputSource(src), v.setInputTarget(tgt)))
        s = stats(t)
        row["FastVGICP calculate_covariances (both clouds, indices included)"] = dict(s, units=2 * n, unit="points", per_unit_us=1e3 * s["median"] / (2 * n))
        del g, v

        for method in ("vgicp_cuda", "vgicp_cuda_rbf", "vgicp"):
            for sname, search in (("DIRECT1", apd.VOXEL_DIRECT1), ("DIRECT7", apd.VOXEL_DIRECT7)):
                g = make(method, search)
                g.setInputTarget(tgt)
                g.setInputSource(src)
                t, r = timed(lambda: g.align(), a.warmup, a.reps)
                s = stats(t)
                row["%s %s align" % (method, sname)] = dict(s, units=int(r["n_linearize"]), unit="linearisations", per_unit_us=1e3 * s["median"] / max(1, r["n_linearize"]),
                                                           converged=bool(r["converged"]))
                t, _ = timed(lambda: g.linearize(np.eye(4)), a.warmup, a.reps)
                s = stats(t)
                row["%s %s linearize" % (method, sname)] = dict(s, units=1, unit="call", per_unit_us=1e3 * s["median"])
                del g
        for method in ("vgicp_cuda", "vgicp"):
            for count in a.counts:
                objs = []
                for q in range(count):
                    o = make(method, apd.VOXEL_DIRECT1)
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
