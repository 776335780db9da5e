"""CPU tests that pin the oracle on the scenes of index_scenes.py before any GPU comparison depends on it (no GPU).

For every scene at n = 513, 2049 and 4097 the exhaustive C oracle, its kd-tree variant and the dense NumPy restatement must return
the same k-NN lists (k = 20) and the same 1-NN correspondences (queries = the scene moved by half a unit, gate off), indices and
squared distances alike.  The module also asserts, from the reference alone, the properties that make each scene mean something:
how many points lie within the k-th distance (above or below what knn_collect_kernel buffers) and how many queries have their
minimum distance at two or more target points.  Those are conditions on the inputs: a generator that cannot meet one is changed,
not the threshold.
"""
import numpy as np
import pytest

import index_scenes as scenes

SIZES = (513, 2049, 4097)
# An interior point of the integer lattice has 1 + 6 + 12 + 8 = 27 points within its 20th distance (d^2 = 3); a point on a face has
# 23 within d^2 = 4.  The interior of a cube of side s is ((s - 2) / s)^3 of it: 0.42 for the 8^3 lattice of n = 513 and more for every
# larger one.  The variant with duplicates has a lattice of 0.8 n points (0.39 interior at n = 513, with its partial top layer) and
# stacks of eight copies that put every lattice point within d^2 = 2 of a stack over the buffer as well.  A quarter of the queries
# is therefore a floor every lattice here must clear.
KNN_TIE_SHARE = 0.25
# A query half a cell off on every axis is equidistant from the 8 corners of its cell unless the cell sticks out of the lattice:
# ((s - 1) / s)^3 >= 0.66 of the queries for s >= 8, less the partial top layer.
NN_TIE_SHARE = 0.5


def _dense_sqd(q, t):
    d = None
    for a in range(3):  # ((dx*dx) + dy*dy) + dz*dz in float32, as oracle/apd_numpy.py
        diff = q[:, None, a] - t[None, :, a]
        d = diff * diff if d is None else d + diff * diff
    return d


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_scene_is_finite_float32_and_reproducible(name, n):
    xyz = scenes.make(name, n)
    assert xyz.dtype == np.float32 and xyz.shape == (n, 3) and xyz.flags["C_CONTIGUOUS"] and np.isfinite(xyz).all()
    assert np.array_equal(xyz, scenes.make(name, n))
    assert not np.array_equal(xyz, scenes.make(name, n, seed=1)) or name.startswith("lattice")
    if name == "line":
        assert not xyz[:, 1:].any()
    if name == "plane":
        assert np.ptp(xyz[:, 2]) == 0
    if name == "lattice3d_dup":
        n_dup = int(n * scenes.DUP_SHARE)
        base = {tuple(p) for p in xyz[: n - n_dup]}
        assert len(base) == n - n_dup and all(tuple(p) in base for p in xyz[n - n_dup :])  # copies sit behind their originals
    if name == "offset":
        assert np.all(xyz[:, :2] * 128 == np.round(xyz[:, :2] * 128))  # x and y on the 1/128 m grid of floats near 1e5


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_knn_oracle_variants_agree_and_tie_conditions_hold(oracle_apd, name, n):
    from oracle import apd_numpy

    xyz = scenes.make(name, n)
    idx, sqd = oracle_apd.knn_self(xyz, scenes.K)
    idx_kd, sqd_kd = oracle_apd.knn_self(xyz, scenes.K, kdtree=True)
    idx_np, sqd_np = apd_numpy.knn_self(xyz, scenes.K)
    assert np.array_equal(idx, idx_kd) and np.array_equal(sqd, sqd_kd)
    assert np.array_equal(idx, idx_np) and np.array_equal(sqd, sqd_np)
    within = (_dense_sqd(xyz, xyz) <= sqd[:, -1:]).sum(axis=1)  # points within the oracle's k-th distance, per query
    over = within > scenes.TIE_BUFFER
    print(f"{name} n={n}: {over.mean():.3f} of the queries have more than {scenes.TIE_BUFFER} points within d_k (max {within.max()})")
    wide = scenes.within_kth(oracle_apd.knn_self(xyz, 32, kdtree=True)[1])
    assert np.array_equal(wide > scenes.TIE_BUFFER, over)  # the saturating count the GPU tests print tells the same story
    if name in scenes.KNN_TIE_SCENES:
        assert over.mean() >= KNN_TIE_SHARE
    if name in scenes.KNN_SELECT_SCENES:
        assert not over.any()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_nn_oracle_variants_agree_and_tie_conditions_hold(oracle_apd, name, n):
    from oracle import apd_numpy

    tgt = scenes.make(name, n)
    src = scenes.shifted(tgt)
    z_s, z_t = np.zeros((n, 4, 4)), np.zeros((n, 4, 4))
    corr, sqd, _ = oracle_apd.update_correspondences(np.eye(4), src, tgt, z_s, z_t, oracle_apd.default_params())  # gate off (FLT_MAX)
    corr_kd, sqd_kd, _ = oracle_apd.update_correspondences(np.eye(4), src, tgt, z_s, z_t, oracle_apd.default_params(search=1))
    corr_np, sqd_np = apd_numpy.nearest(apd_numpy.transform_f32(np.eye(4), src), tgt)
    assert (corr >= 0).all()
    assert np.array_equal(corr, corr_kd) and np.array_equal(sqd, sqd_kd)
    assert np.array_equal(corr, corr_np) and np.array_equal(sqd, sqd_np)
    at_min = (_dense_sqd(src, tgt) == sqd[:, None]).sum(axis=1)
    print(f"{name} n={n}: {(at_min >= 2).mean():.3f} of the queries have two or more targets at the minimum distance (max {at_min.max()})")
    if name in scenes.NN_TIE_SCENES:
        assert (at_min >= 2).mean() >= NN_TIE_SHARE
        tied = at_min >= 2
        assert np.array_equal(corr[tied], np.argmax(_dense_sqd(src[tied], tgt) == sqd[tied, None], axis=1))  # the lowest index of the tied ones


def test_natural_qpw_rule():
    """the sizes the GPU tests take for 8 / 16 / 32 / 64 queries per wave sit where the rule of run_covariances puts them"""
    assert [scenes.natural_qpw([n]) for n in (2300, 16320, 16384, 32704, 40000, 65472, 70000)] == [8, 8, 16, 16, 32, 32, 64]
    assert scenes.natural_qpw([3000] * 16) == 32 and scenes.natural_qpw([3000] * 14) == 32
