"""CPU: the sequential definition of pcl::ApproximateVoxelGrid and its parallel form (tests/approx_voxel_restatement.py) agree bit for
bit, order included, on random clouds, scan-ordered clouds and the edge clouds the GPU test uses."""
import numpy as np
import pytest

import approx_voxel_restatement as R
import approx_voxel_scenes as S
import ndt_scenes

f32 = np.float32


def test_self_test_clouds():
    R.self_test()  # the seven clouds the parallel form was first checked on


CLOUDS, same = S.CLOUDS, S.same


@pytest.mark.parametrize("name", sorted(CLOUDS))
def test_forms_agree(name):
    p, leaf = CLOUDS[name]()
    a, b = R.sequential(p, leaf), R.parallel(p, leaf)
    assert same(a, b)
    assert 1 <= len(a) <= len(p)


def test_expected_counts():
    assert len(R.sequential(S.buckets_512(), 1.0)) == 512
    assert len(R.sequential(S.one_cell(), 1.0)) == 1
    assert len(R.sequential(S.alternating(), 1.0)) == 4096
    ring = S.ring_scan()
    assert ring.shape == (28800, 4) and len(R.sequential(ring, 0.25)) == 4989
    tgt = ndt_scenes.real_pair()[1]
    assert tgt.shape[0] == 5192 and len(R.sequential(tgt, 0.5)) == 2236


def test_only_final_flush_is_in_bucket_order():
    p = S.buckets_512()
    out = R.sequential(p, 1.0)
    b = R.bucket(R.cells(out, 1.0))
    assert np.array_equal(b, np.arange(512))


def test_hash_wraps_in_32_bits():
    assert 300000 * 7171 > 2 ** 31
    c = np.array([[300000, 0, 0], [-300000, 0, 0], [300000, -300000, 300000], [-299999, 300001, -300000]], np.int64)
    got = R.bucket(c)
    for row, g in zip(c, got):
        want = np.array([row[0] * 7171 + row[1] * 3079 + row[2] * 4231], np.int64).astype(np.int32).astype(np.uint32)[0] & 511  # int32 wrap, as the reference behaves
        assert g == want
    # the unwrapped sum gives the same low bits only because 512 divides 2^32: the wrap must not change the bucket
    assert got[0] == (300000 * 7171) % 512
    p = S.hash_wrap()
    cells = R.cells(p, 0.5)
    assert np.abs(cells).min() >= 299990 and (np.abs(cells[:, 0] * 7171) > 2 ** 31).all()


def test_cells_0_and_512_share_bucket_0():
    c = np.array([[0, 0, 0], [512, 0, 0]], np.int64)
    assert R.bucket(c).tolist() == [0, 0]
    p = np.array([[0.5, 0.5, 0.5, 1.0], [512.5, 0.5, 0.5, 2.0], [0.25, 0.5, 0.5, 3.0]], f32)
    out = R.sequential(p, 1.0)
    assert same(out, p)  # each point evicts its predecessor: three single-point outputs in input order
    assert same(R.parallel(p, 1.0), p)


def test_refusals():
    p = S.gaussian(100, 20)
    for bad in (np.nan, np.inf, -np.inf, 1e12):
        q = p.copy()
        q[37, 1] = bad
        with pytest.raises(R.Refused):
            R.sequential(q, 0.1)
        with pytest.raises(R.Refused):
            R.parallel(q, 0.1)
    q = p.copy()
    q[37, 3] = np.nan  # not a coordinate: averaged as given
    a, b = R.sequential(q, 0.5), R.parallel(q, 0.5)
    assert np.isnan(a[:, 3]).sum() == 1 and same(a, b)
