"""Scenes of the batched GICP_OMP tests (tests/test_gicp_omp_batch_gpu.py, tests/test_gicp_omp_batch_host_cpp.py), built from the clouds of
tests/gicp_omp_scenes.py.  Every scene runs with max_correspondence_distance = 0.5 (all handles of a batch carry the same parameters) and
is at most 600 points.  Reference runs of the NumPy restatement are computed once per process."""
import functools

import numpy as np

import gicp_omp_restatement as R
import gicp_omp_scenes as S

f32 = np.float32
PARAMS = dict(max_correspondence_distance=0.5)
T_SMALL = S.pose([0.10, -0.06, 0.03], [0.4, -0.3, 1.0])
LOOP_SIZES = (256, 257, 512, 513, 600)  # a full last block, a one-point last block, two and three blocks


@functools.lru_cache(maxsize=None)
def mixed():
    """Handles that end in different rounds and every small shape: (name, scene) in batch order."""
    eye = np.eye(4, dtype=f32)
    s4, t4 = S.few_pairs(4)
    s3, t3 = S.few_pairs(3)
    a300 = S.room(300, 2)
    n20 = S.room(20, 3)
    return (
        ("four_pairs", dict(source=s4, target=t4, guess=eye, params=PARAMS)),
        ("three_pairs", dict(source=s3, target=t3, guess=S.pose([0.001, 0, 0], [0, 0, 0]), params=PARAMS)),
        ("room300", dict(source=a300, target=S.moved(a300, T_SMALL, 24), guess=eye, params=PARAMS)),
        ("identical", dict(source=a300, target=a300.copy(), guess=eye, params=PARAMS)),
        ("k_equals_n", dict(source=n20, target=S.moved(n20, S.pose([0.01, 0.0, 0.0], [0, 0, 0.2]), 22), guess=eye, params=PARAMS)),
    )


@functools.lru_cache(maxsize=None)
def loop_closure():
    """One target, five candidate sources that end on the block boundaries, distinct small guesses: (name, scene) in batch order."""
    a600 = S.room(600, 1)
    tgt = S.moved(a600, T_SMALL, 21)
    out = []
    for i, n in enumerate(LOOP_SIZES):
        guess = S.pose([0.02 - 0.01 * i, 0.01 * (i % 2), -0.01 + 0.005 * i], [0.05 * i, 0.1 - 0.05 * i, -0.3 + 0.1 * i])
        out.append(("loop%d" % n, dict(source=a600[:n].copy(), target=tgt, guess=guess, params=PARAMS)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def all_scenes():
    return dict(mixed() + loop_closure())


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's align of a scene, computed once."""
    sc = all_scenes()[name]
    return S.make(sc).align(sc["guess"])


@functools.lru_cache(maxsize=None)
def is_stable(name):
    """The stability condition of gicp_omp_scenes.is_stable on these scenes: every reduction scaled by (1 +- 1e-9) leaves the counts."""
    sc, r0 = all_scenes()[name], reference(name)
    for s in (1.0 + 1e-9, 1.0 - 1e-9):
        r = S.make(sc, s).align(sc["guess"])
        if (r["nr_iterations"], r["inner_total"], r["converged"]) != (r0["nr_iterations"], r0["inner_total"], r0["converged"]):
            return False
    return True
