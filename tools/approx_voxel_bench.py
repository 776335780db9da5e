#!/usr/bin/env python3
"""Development timing of pcl::ApproximateVoxelGrid on the GPU (gorio_prep_approx_voxel_downsample, csrc/apd_approx_voxel.hip) beside the
pcl::VoxelGrid path of the same commit (gorio_prep_voxel_downsample); GPU only (it fails without a device), not wired into bench.py.
There is no time gate: VoxelGrid is the yardstick to report beside, not a threshold.

Clouds (x, y, z; both filters put out coordinates only here, so the calls move the same bytes):
    frame       one 16 384-point radar scan (synth.radar_scan), leaf 0.1
    submap      a 160 000-point assembled map (synth.local_map, 10 scans), leaf 0.1 and leaf 0.5
    one_cell    160 000 points inside ONE cell (leaf 1): one run of n points for the new filter, one voxel of n points for VoxelGrid
Timed per cloud, alternating in one process after a warm-up of every shape, wall clock around calls that end in a stream synchronise:
    approx_host     gorio_prep_approx_voxel_downsample: staging, upload, 8 launches, the 4-byte n_out, download of n_out points
    approx_device   gorio_prep_approx_voxel_downsample_device on columns that already live on the device: the launches and the 4-byte n_out
    voxel_host      gorio_prep_voxel_downsample (upload, bounding box, key sort, centroids, download)
and the submap call (ApdGicp.setInputTargetSubmap, 10 keyframes of 16 384 points, leaf 0.1 and 0.5) with DOWNSAMPLE_VOXELGRID and with
DOWNSAMPLE_APPROX_VOXELGRID.  Figures: median, min and max of --reps repetitions in ms, and the output sizes.  One JSON line.

    python tools/approx_voxel_bench.py [--reps 20] [--warmup 3]
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
gorio = importlib.import_module("go-rio_amd")
apd, prep, synth = gorio.apd, gorio.prep, gorio.synth


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "reps": len(t)}


class DeviceColumns:
    """x, y, z of a cloud and an output of the same size as device columns, through the HIP runtime the library links against."""

    def __init__(self, xyz):
        self.hip = C.CDLL("libamdhip64.so")
        self.n = xyz.shape[0]
        self.ptrs = []
        self.cols = (C.c_void_p * 3)(*[self._dev(np.ascontiguousarray(xyz[:, a])) for a in range(3)])
        self.outs = (C.c_void_p * 3)(*[self._dev(np.zeros(self.n, np.float32)) for _ in range(3)])

    def _dev(self, a):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(a.nbytes, 16))) == 0
        assert self.hip.hipMemcpy(p, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        self.ptrs.append(p)
        return p.value

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0
        for p in self.ptrs:
            self.hip.hipFree(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("approx_voxel_bench.py needs a GPU: there is nothing to time without one")
    lib = gorio.load_library()
    rng = np.random.default_rng(7)
    frame = synth.radar_scan(16384, seed=41)[0]
    submap = synth.local_map(160000, seed=5, n_scans=10)[0]
    one_cell = rng.uniform(0.01, 0.99, (160000, 3)).astype(np.float32)
    shapes = [("frame", frame, 0.1), ("submap", submap, 0.1), ("submap", submap, 0.5), ("one_cell", one_cell, 1.0)]
    dev = {id(c): DeviceColumns(c) for _, c, _ in shapes}

    def approx_device(cloud, leaf):
        d = dev[id(cloud)]
        lf = np.array([leaf] * 3, np.float64)
        m = C.c_int(0)
        rc = lib.gorio_prep_approx_voxel_downsample_device(0, d.cols, 3, d.n, C.c_void_p(lf.ctypes.data), d.outs, d.n, C.byref(m), None)
        assert rc == 0, rc
        return m.value

    keyframes = [synth.radar_scan(16384, seed=600 + k, sensor_pose=synth.gt_transform([0.6 * k, 0.05 * k, 0.0], [0.0, 0.0, 1.2 * k])) for k in range(10)]
    rel = [np.linalg.inv(synth.gt_transform([0.6 * 9, 0.05 * 9, 0.0], [0.0, 0.0, 1.2 * 9])) @ synth.gt_transform([0.6 * k, 0.05 * k, 0.0], [0.0, 0.0, 1.2 * k]) for k in range(10)]
    regs = {}
    for name, method in (("voxelgrid", apd.DOWNSAMPLE_VOXELGRID), ("approx_voxelgrid", apd.DOWNSAMPLE_APPROX_VOXELGRID)):
        regs[name] = gorio.ApdGicp()
        regs[name].setSubmapDownsample(method)

    t = {i: {"approx_host": [], "approx_device": [], "voxel_host": []} for i in range(len(shapes))}
    sizes = {}
    ts = {(leaf, name): [] for leaf in (0.1, 0.5) for name in regs}
    sub_sizes = {}
    for it in range(a.warmup + a.reps):
        for i, (_, cloud, leaf) in enumerate(shapes):
            t0 = time.perf_counter()
            na = len(prep.approx_voxel_downsample(cloud, leaf))
            t1 = time.perf_counter()
            nd = approx_device(cloud, leaf)
            t2 = time.perf_counter()
            nv = len(prep.voxel_downsample(cloud, leaf))
            t3 = time.perf_counter()
            assert na == nd
            sizes[i] = (na, nv)
            if it >= a.warmup:
                for k, v in zip(("approx_host", "approx_device", "voxel_host"), (t1 - t0, t2 - t1, t3 - t2)):
                    t[i][k].append(v * 1e3)
        for leaf in (0.1, 0.5):
            for name, g in regs.items():
                t0 = time.perf_counter()
                n = g.setInputTargetSubmap(keyframes, rel, voxel_leaf=leaf)
                t1 = time.perf_counter()
                sub_sizes[(leaf, name)] = n
                if it >= a.warmup:
                    ts[(leaf, name)].append((t1 - t0) * 1e3)
    out = {"reps": a.reps, "warmup": a.warmup, "filters": [], "submap_calls": []}
    for i, (name, cloud, leaf) in enumerate(shapes):
        row = {"cloud": name, "n": int(cloud.shape[0]), "leaf": leaf, "n_out_approx": sizes[i][0], "n_out_voxel": sizes[i][1]}
        row.update({k: stats(v) for k, v in t[i].items()})
        out["filters"].append(row)
    for (leaf, name), v in ts.items():
        out["submap_calls"].append(dict(method=name, leaf=leaf, keyframes=10, points=sum(len(f[0]) for f in keyframes), n_target=sub_sizes[(leaf, name)], **stats(v)))
    for d in dev.values():
        d.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
