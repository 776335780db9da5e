"""The NumPy restatement of the scan pipeline's four new stages (tests/scan_pipeline_restatement.py) on closed forms; no GPU."""
import numpy as np

import scan_pipeline_restatement as sr

F = np.float32


def _raw(xyz, power=1.0, doppler=0.0):
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    return np.concatenate([xyz, np.full((len(xyz), 1), power, F), np.full((len(xyz), 1), doppler, F)], 1)


def test_identity_rotation_leaves_the_points_unchanged():
    rng = np.random.default_rng(1)
    raw = _raw(rng.normal(0, 30, (500, 3)))
    idx, cloud = sr.gate_rotate(raw, 0.0, np.eye(3))
    assert np.array_equal(idx, np.arange(500)) and np.array_equal(cloud.view(np.uint32), raw.view(np.uint32))


def test_quarter_turn_is_exact_on_integer_coordinates():
    rng = np.random.default_rng(2)
    p = rng.integers(-1000, 1000, (300, 3)).astype(F)
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    _, cloud = sr.gate_rotate(_raw(p), 0.0, Rz)
    assert np.array_equal(cloud[:, 0], -p[:, 1]) and np.array_equal(cloud[:, 1], p[:, 0]) and np.array_equal(cloud[:, 2], p[:, 2])


def test_gate_drops_low_power_and_non_finite_points_in_order():
    raw = _raw([[1, 2, 3], [4, 5, 6], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [7, 8, 9]])
    raw[1, 3] = 0.0  # power == threshold: the test is >
    idx, cloud = sr.gate_rotate(raw, 0.0, np.eye(3))
    assert idx.tolist() == [0, 5] and np.array_equal(cloud[:, :3], raw[[0, 5], :3])
    idx, cloud = sr.gate_rotate(_raw([[1, 2, 3], [4, 5, 6]], power=0.5), 0.5, np.eye(3))  # every point at the threshold: the scan is empty
    assert len(idx) == 0 and cloud.shape == (0, 5)
    idx, _ = sr.gate_rotate(_raw([[1, 2, 3]], power=-3.0), 0.0, np.eye(3))
    assert len(idx) == 0


def test_dynamic_selection_keeps_the_inliers_and_nothing_after_a_failed_estimate():
    m = np.array([1, 0, 0, 1, 1, 0], bool)
    assert sr.dynamic_select(m).tolist() == [0, 3, 4]
    assert len(sr.dynamic_select(m, success=False)) == 0


def test_deskew_with_zero_angular_velocity_is_the_identity_bit_for_bit():
    rng = np.random.default_rng(3)
    p = rng.normal(0, 40, (777, 3)).astype(F)
    out = sr.deskew(p, (0.0, 0.0, 0.0), 0.1)
    assert np.array_equal(out.view(np.uint32), p.view(np.uint32))


def test_deskew_about_z_is_the_exact_rotation_to_first_order():
    """With u = delta_t / 2 w and a = |w| delta_t, the UNIT quaternion (1, -u) / sqrt(1 + |u|^2) rotates by 2 atan(a / 2) = a - a^3 / 12 + ...
    about the IMU axis.  The reference feeds Eigen's unit-quaternion formula v + 2 w' (q' x v) + 2 q' x (q' x v) the unnormalised inverse
    q' = (1, -u) / (1 + |u|^2) instead: its first-order term carries 1 / (1 + |u|^2)^2 where the unit quaternion has 1 / (1 + |u|^2), an error
    of |u|^2 * 2 |u| |v| = a^3 / 4 |v|; the second-order term's error is of fourth order, a^4 / 8 |v|.  So the result agrees with the exact
    rotation by a to first (indeed second) order: within (a^3 / 4 + a^3 / 12 + a^4 / 8) |v| plus float rounding."""
    rng = np.random.default_rng(4)
    n = 1000
    p = rng.uniform(-50, 50, (n, 3)).astype(F)
    wz, period = 0.2, 0.1
    out = sr.deskew(p, (0.0, 0.0, wz), period).astype(np.float64)
    a = wz * period * np.arange(n) / n  # the deskew undoes the scan's own rotation: +ang_vel * delta_t
    c, s = np.cos(a), np.sin(a)
    exact = np.stack([c * p[:, 0] - s * p[:, 1], s * p[:, 0] + c * p[:, 1], p[:, 2].astype(np.float64)], 1)
    r = np.linalg.norm(p.astype(np.float64), axis=1)
    # float rounding: about ten operations on values up to |v|
    assert np.all(np.linalg.norm(out - exact, axis=1) <= 16 * np.finfo(F).eps * r + (a ** 3 / 4 + a ** 3 / 12 + a ** 4 / 8) * r + 1e-12)
    big = a > 0.015
    assert np.all(np.linalg.norm(out - exact, axis=1)[big] < 1e-3 * (a * r)[big])  # far below the first-order term itself
    assert np.linalg.norm(out - p, axis=1).max() > 0.5  # and it does rotate: 0.02 rad at 70 m


def test_distance_filter_is_strict_at_all_four_thresholds():
    pts = np.array([[1.0, 0, 0], [100.0, 0, 0], [3.0, 4.0, 20.0], [3.0, 4.0, -5.0], [3.0, 4.0, 0.0], [0, 0, 1.0000001], [99.99999, 0, 0], [3, 4, 19.999998], [3, 4, -4.9999995]], F)
    k = sr.distance_mask(pts, 1.0, 100.0, -5.0, 20.0)
    assert k.tolist() == [False, False, False, False, True, True, True, True, True]


def test_callback_reports_an_all_low_power_scan_as_empty():
    res = sr.callback(_raw(np.ones((50, 3)), power=0.0), sr.default_params(), [], None, None)
    assert res["status"] == "empty" and res["stage"] == 0 and len(res["stages"]["gate"][0]) == 0


def test_chain_seeds_keep_their_patchwork_margin(oracle_apd):
    """The seeds tests/test_scan_pipeline_gpu.py compares exactly: the restatement alone must sit clear of every Patchwork++ decision
    threshold (the guard of tests/test_ground_chain_gpu.py), so a near-tie cannot be mistaken for a bug there."""
    import patchwork_restatement as pr

    for seed, dor, method in sr.CHAIN_CASES:
        raw, p, samples = sr.chain_inputs(seed, dor, method, oracle_apd)
        assert 9000 < len(raw) < 12000
        res = sr.callback(raw, p, samples, sr.CHAIN_ANG_VEL, oracle_apd, pr.Patchworkpp())
        assert res["status"] == "ok" and res["margin"] > 1e-4, (seed, dor, method, res["margin"])
        assert res["n_out"] > 1000 and res["n_clusters"] >= 1 and 0 < res["n_ground"] < res["n_out"]
        assert len(res["stages"]["gate"][0]) < len(raw) and len(res["stages"]["outlier"][0]) < len(res["stages"]["distance"][0]) < res["n_gated"]
    pw = pr.Patchworkpp()
    for seed in sr.SEQUENCE_SEEDS:
        raw, p, samples = sr.chain_inputs(seed, False, sr.OUTLIER_STATISTICAL, oracle_apd, n_ground=sr.SEQUENCE_N_GROUND)
        res = sr.callback(raw, p, samples, sr.CHAIN_ANG_VEL, oracle_apd, pw)
        assert res["status"] == "ok" and res["margin"] > 1e-4, (seed, res["margin"])
