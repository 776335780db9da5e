#!/usr/bin/env python3
"""Development timing of the keyframe store (include/gorio_keyframes.h) against the host entry points it stands beside; GPU only (it
fails without a device), not wired into bench.py.

The frames are what the scan pipeline really puts out for scan_pipeline_restatement.raw_scan with its defaults and a raw message of
--points points (16 384): one message, seen from a sensor that moves 0.2 m and turns 0.01 rad per frame.

(a) one keyframe change of the front end (scan_matching_odometry_nodelet.cpp:586-618) with a ten-frame submap, leaf 0.1.  Before every
    repetition, untimed and the same for both routes: the pipeline runs the frame, the registration takes it as its source
    (setInputSourceFromScan) and aligns against the current keyframe.  Timed:
      host    xyz, label = pipe.output(); reg.setInputTarget(xyz, label); reg.calculateCovariances();
              sub.setInputTargetSubmap(nine older host clouds + this one, poses, 0.1)
      store   id = store.add_from_apd(reg, 0); reg.setInputTargetKeyframe(store, id); reg.calculateCovariances();
              sub.setInputTargetSubmapKeyframes(store, nine older ids + id, poses, 0.1)
(b) loop-closure verification (loop_detector.cpp:391-422) of 8 candidates against a new keyframe, twice in a row -- two new keyframes,
    the same 8 candidates -- with one registration object, per candidate setInputSource, align, getFitnessScore.  Each visit is timed.
      host    reg.setInputTarget(cloud); per candidate reg.setInputSource(cloud)
      store   reg.setInputTargetKeyframe(store, id); per candidate reg.setInputSourceKeyframe(store, id)
    The second visit is where kept covariances and search indices show: the store route finds those of the 8 candidates in place.

The two routes alternate in one process after a warm-up of every shape; every timed region ends in a call that synchronises the stream
(the submap assembly, the fitness score).  Figures: median, min and max of --reps repetitions, wall clock.  Prints one JSON line.

    python tools/keyframe_bench.py [--reps 20] [--warmup 3] [--points 16384]
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
import scan_pipeline_restatement as sr  # noqa: E402  (scenes only)

ANG_VEL = (0.01, -0.02, 0.15)
KW = dict(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)
LEAF = 0.1


def stats(t):
    return {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)), "max_ms": float(np.max(t)), "reps": len(t)}


def pose(k):
    T = np.eye(4)
    c, s = np.cos(0.01 * k), np.sin(0.01 * k)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [0.2 * k, -0.1 * k, 0.0]
    return T


def make_raws(points, count):
    rot = sr.tilt()
    extra = len(sr.raw_scan(200, n_ground=1000, rotation=rot)) - 1000  # what a message carries beside its ground points
    raw = sr.raw_scan(200, n_ground=points - extra, rotation=rot)
    raws = []
    for k in range(count):
        T = pose(k)
        r = raw.copy()
        with np.errstate(invalid="ignore"):  # the message's NaN / Inf points stay what they are
            r[:, :3] = (raw[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        raws.append(r)
    return rot, raws


class Frames:
    """The pipeline and the frames it puts out; run(k) leaves frame k as the pipeline's output."""

    def __init__(self, points, count):
        self.rot, self.raws = make_raws(points, count)
        self.params = gorio.prep.scan_default_params(rotation=self.rot)
        self.pipe = gorio.prep.ScanPipeline(self.params)
        self.rng = np.random.default_rng(7)

    def run(self, k):
        _, nv = self.pipe.load(self.raws[k])
        samples = self.rng.integers(0, nv, (3, self.params.reve.n_ransac_points)).astype(np.uint32)
        r = self.pipe.run(samples, ANG_VEL)
        assert r["status"] == "ok", r
        return r


def keyframe_change(a, fr, clouds, out):
    """(a): clouds[k] = (xyz, intensity, label) of frame k as the pipeline put it out."""
    older = list(range(9))
    new = 10  # aligned against keyframe 9
    rel = [np.linalg.inv(pose(new)) @ pose(k) for k in older + [new]]
    store = gorio.KeyframeStore()
    old_ids = [store.add(clouds[k][0], clouds[k][1], clouds[k][2]) for k in older]
    regs = {r: gorio.ApdGicp(**KW) for r in ("host", "store")}
    subs = {r: gorio.ApdGicp(**KW) for r in ("host", "store")}
    parts = ("take_keyframe", "set_target", "covariances", "submap", "total")
    t = {r: {p: [] for p in parts} for r in regs}
    n_sub = {}
    for i in range(a.warmup + a.reps):
        for route in ("host", "store"):
            reg, sub = regs[route], subs[route]
            reg.setInputTarget(clouds[9][0], clouds[9][2])
            fr.run(new)
            reg.setInputSourceFromScan(fr.pipe)
            reg.align()
            t0 = time.perf_counter()
            if route == "host":
                xyz, _, _, lab = fr.pipe.output()
                t1 = time.perf_counter()
                reg.setInputTarget(xyz, lab)
                t2 = time.perf_counter()
                reg.calculateCovariances()
                t3 = time.perf_counter()
                n_sub[route] = sub.setInputTargetSubmap([(clouds[k][0], clouds[k][2]) for k in older] + [(xyz, lab)], rel, voxel_leaf=LEAF)
            else:
                kid = store.add_from_apd(reg, 0)
                t1 = time.perf_counter()
                reg.setInputTargetKeyframe(store, kid)
                t2 = time.perf_counter()
                reg.calculateCovariances()
                t3 = time.perf_counter()
                n_sub[route] = sub.setInputTargetSubmapKeyframes(store, old_ids + [kid], rel, voxel_leaf=LEAF)
            t4 = time.perf_counter()
            if route == "store":
                reg.clearTarget()
                store.release(kid)
            if i >= a.warmup:
                for p, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
                    t[route][p].append(v * 1e3)
    assert n_sub["host"] == n_sub["store"]
    same = np.array_equal(subs["host"].getTargetPoints()[0].view(np.uint32), subs["store"].getTargetPoints()[0].view(np.uint32))
    out["keyframe_change"] = {r: {p: stats(v) for p, v in t[r].items()} for r in t}
    out["keyframe_change"].update(n_keyframe=int(len(clouds[new][0])), n_submap_in=int(sum(len(clouds[k][0]) for k in older + [new])), n_submap=int(n_sub["host"]), submaps_equal=bool(same))
    store.close()


def loop_verification(a, clouds, out):
    """(b): candidates = frames 0..7, the two new keyframes = frames 9 and 10."""
    cands, news = list(range(8)), (9, 10)
    t = {r: {"visit_1": [], "visit_2": []} for r in ("host", "store")}
    last = {}
    for i in range(a.warmup + a.reps):
        for route in ("host", "store"):
            reg = gorio.ApdGicp(**KW)  # a fresh object and a fresh store: visit 1 finds nothing in place on either route
            store = gorio.KeyframeStore() if route == "store" else None
            ids = {k: store.add(clouds[k][0], clouds[k][1], clouds[k][2]) for k in cands + list(news)} if store else {}
            res = []
            for visit, new in enumerate(news):
                t0 = time.perf_counter()
                if store:
                    reg.setInputTargetKeyframe(store, ids[new])
                else:
                    reg.setInputTarget(clouds[new][0], clouds[new][2])
                for c in cands:
                    if store:
                        reg.setInputSourceKeyframe(store, ids[c])
                    else:
                        reg.setInputSource(clouds[c][0], clouds[c][2])
                    r = reg.align(np.linalg.inv(pose(new)) @ pose(c))
                    res.append((r["T"].tobytes(), reg.getFitnessScore()[0]))
                t1 = time.perf_counter()
                if i >= a.warmup:
                    t[route]["visit_%d" % (visit + 1)].append((t1 - t0) * 1e3)
            last[route] = res
            if store:
                store.close()
    out["loop_verification"] = {r: {p: stats(v) for p, v in t[r].items()} for r in t}
    out["loop_verification"].update(candidates=len(cands), results_equal=bool(last["host"] == last["store"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=16384)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("keyframe_bench.py needs a GPU: there is nothing to time without one")
    fr = Frames(a.points, 11)
    clouds = []
    for k in range(11):
        fr.run(k)
        xyz, inten, _, lab = fr.pipe.output()
        clouds.append((xyz, inten, lab))
    out = {"reps": a.reps, "warmup": a.warmup, "n_raw": int(len(fr.raws[0])), "n_out": [int(len(c[0])) for c in clouds]}
    keyframe_change(a, fr, clouds, out)
    loop_verification(a, clouds, out)
    fr.pipe.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
