"""CPU tests that pin tests/search_restatement.py, the reference of the GPU search tests: on self queries it returns the indices and
squared distances of the oracle's knn_self bit for bit (tie-free and tie scenes of tests/index_scenes.py), and its radius rule is the
strict d < float32(r * r) on hand-built points exactly at, just inside and just outside the bound.  No GPU."""
import numpy as np
import pytest

import index_scenes as S
import search_restatement as R


@pytest.mark.parametrize("scene", ["radar", "line", "lattice3d", "lattice3d_dup"])
@pytest.mark.parametrize("k", [1, 20])
def test_self_knn_is_the_oracles(oracle_apd, scene, k):
    xyz = S.make(scene, 700)
    idx_o, sqd_o = oracle_apd.knn_self(xyz, k)
    idx, sqd, cnt = R.knn(xyz, None, k)
    assert np.array_equal(idx, idx_o)
    assert np.array_equal(sqd.view(np.uint32), sqd_o.view(np.uint32))
    assert np.array_equal(cnt, np.full(len(xyz), k))
    idx_e, sqd_e, _ = R.knn(xyz, xyz.copy(), k)  # the explicit form of the same queries
    assert np.array_equal(idx_e, idx) and np.array_equal(sqd_e.view(np.uint32), sqd.view(np.uint32))


def test_tie_scenes_do_have_ties():
    xyz = S.make("lattice3d", 700)
    _, sqd, _ = R.knn(xyz, None, 20)
    assert (sqd[:, 1:] == sqd[:, :-1]).any(axis=1).all()  # every lattice point has equal distances inside its list


def test_knn_padding_and_nonfinite_queries():
    xyz = S.make("radar", 5)
    q = np.array([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]], np.float32)
    idx, sqd, cnt = R.knn(xyz, q, 8)
    assert cnt.tolist() == [5, 0, 0]
    assert (idx[0, 5:] == -1).all() and np.isinf(sqd[0, 5:]).all() and (idx[0, :5] >= 0).all()
    assert (idx[1:] == -1).all() and np.isinf(sqd[1:]).all()
    idx0, _, cnt0 = R.knn(np.zeros((0, 3), np.float32), q, 3)
    assert (idx0 == -1).all() and (cnt0 == 0).all()


def test_radius_rule_at_the_bound():
    two = np.float32(2.0)
    inside, outside = np.nextafter(two, np.float32(0)), np.nextafter(two, np.float32(3))
    # index:          0 (at)  1 (inside)  2 (outside)  3 (at, y axis)  4 (the query itself)  5 (inside, same distance as 1)
    xyz = np.array([[two, 0, 0], [inside, 0, 0], [outside, 0, 0], [0, two, 0], [0, 0, 0], [0, 0, -inside]], np.float32)
    assert R.radius_bound(2.0) == np.float32(4.0)
    assert inside * inside < np.float32(4.0) and two * two == np.float32(4.0) and outside * outside > np.float32(4.0)
    offs, idx, sqd = R.radius(xyz, np.zeros((1, 3), np.float32), 2.0)
    assert offs.tolist() == [0, 3] and idx.tolist() == [4, 1, 5]  # ascending (d, index); the points AT the bound are out
    assert np.array_equal(sqd, np.array([0, inside * inside, inside * inside], np.float32))
    assert R.radius(xyz, np.zeros((1, 3), np.float32), 2.0, max_nn=2)[1].tolist() == [4, 1]
    assert R.radius(xyz, np.zeros((1, 3), np.float32), 2.0, max_nn=7)[1].tolist() == [4, 1, 5]
    # the product is taken in double and rounded once; squaring float32(0.7) in float32 gives another bound
    assert R.radius_bound(0.7) == np.float32(np.float64(0.7) * np.float64(0.7)) != np.float32(0.7) * np.float32(0.7)
    offs, idx, _ = R.radius(xyz, np.array([[np.nan, 0, 0], [0, 0, 0]], np.float32), 1.0)
    assert offs.tolist() == [0, 0, 1] and idx.tolist() == [4]


def test_radius_is_the_prefix_of_the_full_order():
    xyz = S.make("lattice3d_dup", 400)
    q = S.shifted(xyz)[:50]
    offs, idx, sqd = R.radius(xyz, q, 1.5)
    d = R.sqdist(q, xyz)
    for i in range(len(q)):
        o = np.lexsort((np.arange(len(xyz)), d[i]))
        m = int((d[i] < R.radius_bound(1.5)).sum())
        assert np.array_equal(idx[offs[i]:offs[i + 1]], o[:m]) and np.array_equal(sqd[offs[i]:offs[i + 1]], d[i, o[:m]])
