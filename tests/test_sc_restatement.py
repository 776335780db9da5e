"""The Scan Context restatement (tests/sc_restatement.py) against hand-worked cases of the reference's arithmetic and quirks.
No GPU."""
import numpy as np
import pytest

import sc_restatement as sr

F = np.float32


def _point(ring, sector, rng_=56.5):
    """A point in the middle of bin (ring, sector), 1-based, in the sensor frame (x forward, y left)."""
    r = (ring - 0.5) * 2.0
    az = -rng_ + (sector - 0.5) * (2 * rng_ / 20)  # SC azimuth, degrees
    t = np.deg2rad(-az)  # the SC azimuth is minus the usual one
    return [r * np.cos(t), r * np.sin(t), 0.0]


def test_one_point_per_bin():
    xyz, inten, want = [], [], np.zeros((40, 20))
    for ring in range(1, 41):
        for sec in range(1, 21):
            xyz.append(_point(ring, sec))
            v = ring * 100 + sec
            inten.append(v)
            want[ring - 1, sec - 1] = v
    d = sr.make_scancontext(np.array(xyz, F), np.array(inten, F))
    np.testing.assert_array_equal(d, want)
    np.testing.assert_array_equal(sr.ring_key(d), want.mean(axis=1))
    np.testing.assert_allclose(sr.sector_key(d), want.mean(axis=0), rtol=1e-15)


def test_bin_value_is_max_intensity_not_height():
    xyz = np.array([_point(5, 7), _point(5, 7), _point(5, 7)], F)
    xyz[:, 2] = [10.0, -3.0, 0.0]
    d = sr.make_scancontext(xyz, np.array([1.0, 7.5, 2.0], F))
    assert d[4, 6] == 7.5 and np.count_nonzero(d) == 1


def test_ring_edges_and_ceil_boundary():
    # r = 2 m: ceil(2 / 80 * 40) = 1 -> ring 1; just above 2 m -> ring 2; r = 0 -> ceil(0) = 0 -> clamped to 1; r = 80 kept in ring 40
    x = np.array([2.0, np.nextafter(F(2.0), F(3.0)), 1e-3, 80.0, np.nextafter(F(80.0), F(81.0))], F)
    keep, ring, _, _, _ = sr.bin_indices(x, np.zeros_like(x), 56.5)
    assert list(keep) == [True, True, True, True, False]
    assert list(ring[:4]) == [1, 2, 1, 40]
    # sector: azimuth near -56.5 -> 1, near +56.5 -> 20.  Straight ahead, atan2f(x, 0) is float(pi / 2), a little above pi / 2, so the
    # azimuth is +2.5e-6 deg and ceil puts the point in sector 11, not 10
    t = np.deg2rad(np.array([56.4, -56.4, 0.0]))
    keep, _, sec, az, _ = sr.bin_indices((10 * np.cos(t)).astype(F), (10 * np.sin(t)).astype(F), 56.5)
    assert all(keep) and sec[0] == 1 and sec[1] == 20
    assert 0 < az[2] < 1e-5 and sec[2] == 11


def test_azimuth_convention_and_range():
    # SC:185: (atan2f(x, y) - pi/2) in degrees: ahead about 0, left (y > 0) negative, behind out of range
    keep, _, _, az, _ = sr.bin_indices(np.array([10.0, 0.0, -10.0], F), np.array([0.0, 10.0, 0.0], F), 56.5)
    assert abs(az[0]) < 1e-5 and az[1] == F(-90.0)
    assert list(keep) == [True, False, False]


def test_abs_is_the_float_overload():
    """|azimuth| 56.7 deg: the float abs skips the point; int abs would have kept it (include/gorio_sc.h)."""
    t = np.deg2rad(56.7)
    keep, _, _, az, _ = sr.bin_indices(np.array([10 * np.cos(t)], F), np.array([10 * np.sin(t)], F), 56.5)
    assert 56.5 < abs(float(az[0])) < 57.0 and int(abs(float(az[0]))) <= 56.5
    assert not keep[0]


def test_nan_coordinates_land_in_bin_1_1_and_inf_range_is_skipped():
    xyz = np.array([[np.nan, 5.0, 0.0], [5.0, np.nan, 0.0], [np.inf, 1.0, 0.0], [1.0, -np.inf, 0.0], [np.nan, np.inf, 0.0]], F)
    d = sr.make_scancontext(xyz, np.array([3.0, 4.0, 100.0, 100.0, 2.0], F))
    assert d[0, 0] == 4.0 and np.count_nonzero(d) == 1


def test_intensity_at_or_below_start_value_gives_zero_and_nan_never_updates():
    xyz = np.array([_point(3, 3), _point(3, 3), _point(4, 4), _point(6, 6), _point(6, 6)], F)
    d = sr.make_scancontext(xyz, np.array([-1000.0, -5000.0, np.nan, -999.5, np.nan], F))
    assert d[2, 2] == 0.0 and d[3, 3] == 0.0 and d[5, 5] == -999.5
    assert np.count_nonzero(d) == 1
    # negative intensities above -1000 are kept, the maximum wins
    d = sr.make_scancontext(np.array([_point(1, 2)] * 2, F), np.array([-7.0, -3.0], F))
    assert d[0, 1] == -3.0


def test_circshift_direction():
    m = np.arange(2 * 20, dtype=float).reshape(2, 20)
    s = sr.circshift(m, 3)
    np.testing.assert_array_equal(s[:, 3], m[:, 0])  # column c moves to (c + 3) mod 20
    np.testing.assert_array_equal(s[:, 2], m[:, 19])
    np.testing.assert_array_equal(sr.circshift(m, 0), m)


@pytest.mark.parametrize("k", [1, 2, 3, 7, 19])
def test_column_permuted_descriptor_recovers_its_shift(k):
    rng = np.random.default_rng(k)
    d = rng.uniform(0, 10, (40, 20)) * (rng.uniform(size=(40, 20)) < 0.4)
    c = sr.circshift(d, k)  # the candidate is the query shifted by k columns
    dist, shift = sr.distance(d, c)
    assert shift == (20 - k) % 20 and dist == pytest.approx(0.0, abs=1e-15)
    np.testing.assert_array_equal(sr.circshift(c, shift), d)


def test_search_shifts_sorted():
    assert sr.search_shifts(0) == [0, 1, 19]
    assert sr.search_shifts(19) == [0, 18, 19]
    assert sr.search_shifts(7) == [6, 7, 8]


def test_no_effective_column_gives_nan_then_big():
    z = np.zeros((40, 20))
    d = np.zeros((40, 20))
    d[3, 4] = 1.0
    assert np.isnan(sr.dist_direct(z, d))
    assert sr.distance(z, d) == (sr.BIG, 0)


def test_dist_direct_skips_zero_columns():
    a, b = np.zeros((40, 20)), np.zeros((40, 20))
    a[0, 0] = b[0, 0] = 1.0  # cosine 1
    a[0, 1], a[1, 1] = 1.0, 0.0
    b[0, 1], b[1, 1] = 0.0, 1.0  # cosine 0
    a[5, 2] = 1.0  # column 2 empty in b: skipped
    assert sr.dist_direct(a, b) == 0.5


def test_key_distance_grouped_float_order():
    rng = np.random.default_rng(3)
    q = rng.uniform(0, 50, 40).astype(F)
    k = rng.uniform(0, 50, (5, 40)).astype(F)
    got = sr.key_distances(q, k)
    for i in range(5):
        res = F(0)
        for g in range(10):
            d = [F(q[4 * g + j] - k[i, 4 * g + j]) for j in range(4)]
            res = F(res + F(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]))
        assert got[i] == res


def test_knn_fewer_than_three_and_empty():
    q = np.zeros(40, F)
    pos, dist, n = sr.knn(q, np.zeros((0, 40), F))
    assert n == 0 and list(pos) == [0, 0, 0] and dist[0] == 0 and dist[1] == 0 and dist[2] == sr.FLT_MAX
    keys = np.stack([np.full(40, 2.0, F), np.full(40, 1.0, F)])
    pos, dist, n = sr.knn(q, keys)
    assert n == 2 and list(pos) == [1, 0, 0] and list(dist) == [F(40.0), F(160.0), sr.FLT_MAX]
    pos, dist, n = sr.knn(q, keys[:1])
    assert n == 1 and list(pos) == [0, 0, 0] and list(dist) == [F(160.0), F(0.0), sr.FLT_MAX]


def test_knn_ties_go_to_the_lower_position():
    keys = np.stack([np.full(40, 3.0, F), np.full(40, 1.0, F), np.full(40, 1.0, F), np.full(40, 1.0, F)])
    pos, _, _ = sr.knn(np.zeros(40, F), keys)
    assert list(pos) == [1, 2, 3]


class _Db(sr.SCManagerRef):
    """A database of hand-set ring keys: the k-NN sees only ring_keys_f, the SC distance only descs."""

    def __init__(self, keys):
        super().__init__()
        for v in keys:
            d = np.zeros((40, 20))
            d[:, int(v) % 20] = v + 1.0
            self.descs.append(d)
            self.ring_keys.append(sr.ring_key(d))
            self.sector_keys.append(sr.sector_key(d))
            self.ring_keys_f.append(np.full(40, v, F))


def test_early_return_below_ten_keeps_the_counter():
    db = _Db(range(30))
    for q in range(10):
        lid, yaw, md, dg = db.detect(q, list(range(q + 1)))
        assert (lid, yaw, md) == (-1, 0.0, sr.BIG) and dg["early_return"] == 1
    assert db.counter == 0
    db.detect(10, [0])
    assert db.counter == 1


def test_size_t_wrap_keeps_candidates_after_the_query():
    db = _Db(range(40))
    db.detect(20, [0, 5, 10, 11, 15, 25, 39])
    # 20 - c >= 10 for c <= 10; 25 and 39 wrap to huge values and are kept
    assert db.snapshot == [0, 5, 10, 25, 39]


def test_stale_snapshot_maps_through_the_current_candidate_list():
    db = _Db([float(i) for i in range(40)])
    # rebuild at counter 0 from candidates 0..9 (all >= 10 back from 25)
    _, _, _, dg = db.detect(25, list(range(10)))
    assert dg["rebuilt"] == 1 and db.snapshot == list(range(10))
    # query 30 has ring key 30: nearest snapshot entries are keyframes 9, 8, 7 at positions 9, 8, 7
    # the current list is shorter: position 9 and 8 are beyond it (skipped); position 7 names keyframe 17, not 7
    cur = [10, 11, 12, 13, 14, 15, 16, 17]
    _, _, _, dg = db.detect(30, cur)
    assert dg["rebuilt"] == 0 and dg["snapshot_size"] == 10
    assert list(dg["position"]) == [9, 8, 7]
    assert list(dg["keyframe"]) == [-1, -1, 17]
    assert np.isnan(dg["sc_dist"][0]) and not np.isnan(dg["sc_dist"][2])


def test_fewer_than_three_entries_map_position_zero():
    db = _Db([float(i) for i in range(40)])
    lid, yaw, md, dg = db.detect(12, [0, 11])  # snapshot [0]: positions [0, 0, 0], all name keyframe 0
    assert db.snapshot == [0] and dg["n_found"] == 1
    assert list(dg["position"]) == [0, 0, 0] and list(dg["keyframe"]) == [0, 0, 0]
    assert dg["key_dist"][1] == 0 and dg["key_dist"][2] == sr.FLT_MAX


def test_empty_snapshot_evaluates_position_zero_of_the_list():
    db = _Db([float(i) for i in range(40)])
    lid, yaw, md, dg = db.detect(12, [11, 5])  # 12 - 11 < 10, 12 - 5 < 10: empty snapshot
    assert dg["snapshot_size"] == 0 and dg["n_found"] == 0
    assert list(dg["keyframe"]) == [11, 11, 11]  # position 0 of the current list, three times


def test_yaw_is_returned_without_a_loop():
    assert sr.yaw_rad(3, 56.5) == np.float32(np.float64(np.float32(3 * 5.65)) * np.pi / 180.0)
    db = _Db([float(i) for i in range(40)])
    db.thresh = -1.0  # nothing is a loop
    db.descs[0] = sr.circshift(db.descs[12], 2)
    lid, yaw, md, dg = db.detect(12, [0])
    assert lid == -1 and md == pytest.approx(0.0, abs=1e-15)
    assert yaw == sr.yaw_rad(18, 56.5) and yaw != 0


def test_empty_candidate_list_is_refused():
    with pytest.raises(ValueError):
        _Db(range(20)).detect(15, [])
