"""Scenes of the batched FastGICPMultiPoints tests: the align scenes of gicp_mp_scenes.py, all_empty, and one scene with LONG neighbour
segments (more than 4 096 neighbours of one query, the segments the radius search sorts outside LDS).

dense_64_4200: the 64-point source and 300-point target of id_64_300, with a ball of 4 200 points (radius 0.05 m) added to the target around
source point 20.  Three source points then have the whole ball inside their 0.5 m radius at the first pass and at the last.  A target that
is nothing but such a ball does not serve: every source point then sees the same 4 200 neighbours, the merged distributions are all alike
and the Gauss-Newton steps run away (tried on the CPU: steps of 0.8 m, no convergence).  With the room around the ball the restatement
alone gives (recorded here, tests/test_gicp_mp_batch_restatement.py keeps the record honest):
    passes 5, iterations 4, converged, convergence ratios 10983.6, 285.3, 14.8, 2.87, 0.434 -- none between 0.5 and 2, so float noise
    cannot flip the pass count -- and 3 long segments at the first pose.

The batch's pass counts by the restatement alone: 3, 3, 4, 4, 5, 3, 4, 3 for gicp_mp_scenes.ALIGN_SCENES in order, 1 for all_empty, 5 for
dense_64_4200: four distinct values."""
import functools

import numpy as np

import gicp_mp_restatement as R
import gicp_mp_scenes as M
import icp_scenes as S

f32 = np.float32
DENSE = "dense_64_4200"
DENSE_RECORD = dict(passes=5, iterations=4, converged=True, long_segments=3)
BATCH = M.ALIGN_SCENES + ["all_empty", DENSE]
PASSES = dict(zip(BATCH, [3, 3, 4, 4, 5, 3, 4, 3, 1, 5]))


def ball(n, radius, centre, seed):
    """n points uniform in a ball"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 1.0, (n, 3))
    v *= (radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (v + centre).astype(f32)


@functools.lru_cache(maxsize=None)
def scenes():
    out = dict(M.scenes())
    src = S.source(64, 300)
    tgt = np.concatenate([S.target(300), ball(4200, 0.05, src[20].astype(np.float64), 7)]).astype(f32)
    out[DENSE] = dict(source=src, target=tgt, guess=np.eye(4, dtype=f32), params={})
    return out


def params_of(name):
    p = dict(R.DEFAULTS)
    p.update(scenes()[name]["params"])
    return p


@functools.lru_cache(maxsize=None)
def reference(name):
    sc = scenes()[name]
    return R.align(sc["source"], sc["target"], sc["guess"], **sc["params"])
