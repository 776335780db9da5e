"""CPU checks of the Patchwork++ restatement (tests/patchwork_restatement.py) and of the ground binding's surface."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import ground_scenes as gs
import patchwork_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_noiseless_plane_all_ground_and_normal_recovered():
    n_true = np.array([0.02, -0.03, 1.0])
    n_true /= np.linalg.norm(n_true)
    xyz, inten = gs.plane_scan(1, normal=n_true, d=0.7)
    for id in (0, 1):
        out = pr.Patchworkpp().estimate_ground(xyz, inten, id=id)
        assert len(out["ground"]) == len(xyz) and len(out["nonground"]) == 0
        f = out["final"]
        assert np.allclose(f["normal"], n_true, atol=1e-4) and abs(float(f["d"]) - 0.7) < 1e-3


def test_vertical_wall_is_not_upright():
    rng = np.random.default_rng(2)
    m = 400
    xyz = np.stack([np.full(m, 3.0) + rng.normal(0, 0.01, m), rng.uniform(0.5, 2.5, m), rng.uniform(-0.7, 2.0, m)], 1).astype(np.float32)
    out = pr.Patchworkpp().estimate_ground(xyz, np.full(m, 0.5, np.float32), id=1)
    fitted = [p for p in out["patches"] if "fits" in p]
    assert len(fitted) == 1 and fitted[0]["decision"] == 1  # GORIO_GROUND_NOT_UPRIGHT
    assert fitted[0]["uprightness"] < 0.5 and len(out["ground"]) == 0


def test_erase_skips_the_point_after_each_erased_point():
    xyz = np.array([[0, 0, -3], [0, 0, -3], [0, 0, -3], [0, 0, 0], [0, 0, -3], [0, 0, -3]], np.float32)
    kept, dists = pr.erase_under_ground(range(6), xyz, np.array([0, 0, 1], np.float32), np.float32(0.5))
    # 0 erased, 1 (moved to slot 0) never tested, 2 erased, 3 never tested, 4 erased, 5 never tested: all six lie 2.5 m under
    # the plane, three survive
    assert kept == [1, 3, 5] and len(dists) == 3


def test_single_ring0_elevation_sets_sensor_height_to_zero():
    ref = pr.Patchworkpp()
    ref.set_state([0.0] * 4, [0.0] * 4, 0.7)
    ref.elevation_thr[0] = 10.0  # every upright ring-0 patch is "not elevated"
    xyz, inten = gs.plane_scan(3, n=400, r_max=3.0)  # one ring-0 patch sector only
    keep = (xyz[:, 0] > 0) & (xyz[:, 1] > 0)
    out = ref.estimate_ground(xyz[keep], inten[keep], id=0)
    assert sum(1 for p in out["patches"] if p["concentric_idx"] == 0 and "fits" in p) == 1
    assert len(ref.upd_elev[0]) == 1 and ref.sensor_height == 0.0 and ref.elevation_thr[0] == 0.0


def test_flatness_update_breaks_at_first_short_ring():
    ref = pr.Patchworkpp()
    ref.set_state([0.0] * 4, [1.0, 2.0, 3.0, 4.0], 0.7, update_flatness=[[0.1], [0.2, 0.3], [0.4, 0.5], []])
    ref.estimate_ground(np.zeros((1, 3), np.float32) + 100, np.ones(1, np.float32), id=0)
    assert ref.flatness_thr == [1.0, 2.0, 3.0, 4.0]


def test_lm_iterations_and_termination_are_reported():
    xyz, inten = gs.scan(4)
    out = pr.Patchworkpp().estimate_ground(xyz, inten, id=1)
    its = [(q["iters"], q["term"]) for p in out["patches"] if "fits" in p for q in p["fits"]]
    assert its and all(1 <= i <= pr.MAX_LM_ITER and t in pr.TERM and t != 0 for i, t in its)
    assert sum(1 for i, t in its if t == 4) >= len(its) // 2  # the scale of (n, d) is free: most solves run to the cap
    assert out["final"]["iters"] >= 1
    out0 = pr.Patchworkpp().estimate_ground(xyz, inten, id=0)
    assert all(q["iters"] == 0 for p in out0["patches"] if "fits" in p for q in p["fits"])


def test_analytic_jacobian_matches_complex_step():
    rng = np.random.default_rng(5)
    P = rng.uniform(-10, 10, (20, 3)).astype(np.float32)
    P[:, 2] = -0.7 + rng.normal(0, 0.05, 20)
    Cm = pr.range_covariance(P)
    x = np.array([0.05, -0.02, 0.98, 0.71])
    _, J = pr.plane_residuals(x, P.astype(np.float64), Cm)
    for k in range(4):
        xc = x.astype(complex)
        xc[k] += 1e-30j
        p0, p1, p2 = (P[:, i].astype(np.float64) for i in range(3))
        a = ((xc[0] * p0 + xc[1] * p1) + xc[2] * p2) + xc[3]
        q = (xc[0] * xc[0] + xc[1] * xc[1]) + xc[2] * xc[2]
        cn = [(Cm[:, 0] * xc[0] + Cm[:, 1] * xc[1]) + Cm[:, 2] * xc[2], (Cm[:, 1] * xc[0] + Cm[:, 3] * xc[1]) + Cm[:, 4] * xc[2],
              (Cm[:, 2] * xc[0] + Cm[:, 4] * xc[1]) + Cm[:, 5] * xc[2]]
        w = (xc[0] * cn[0] + xc[1] * cn[1]) + xc[2] * cn[2]
        r = (a / np.sqrt(q)) ** 2 / w
        np.testing.assert_allclose(J[:, k], r.imag / 1e-30, rtol=1e-9, atol=1e-9 * np.abs(J).max())


def test_scale_freedom_of_the_cost():
    P = gs.plane_scan(6, n=50)[0]
    Cm = pr.range_covariance(P)
    x = np.array([0.01, 0.02, 0.99, 0.7])
    r1 = pr.plane_residuals(x, P.astype(np.float64), Cm, jac=False)
    r2 = pr.plane_residuals(2 * x, P.astype(np.float64), Cm, jac=False)
    np.testing.assert_allclose(r2, r1 / 4, rtol=1e-12)


def test_svd3_against_numpy():
    rng = np.random.default_rng(7)
    for _ in range(50):
        A = rng.normal(size=(3, 3)).astype(np.float32)
        cov = (A @ A.T).astype(np.float32)
        sv, u = pr.svd3(cov)
        ref = np.linalg.svd(cov.astype(np.float64), compute_uv=False)
        np.testing.assert_allclose(sv, ref, rtol=1e-4, atol=1e-5 * ref[0])
        assert abs(abs(float(np.dot(u, np.linalg.svd(cov.astype(np.float64))[0][:, 2]))) - 1) < 1e-3
    sv, u = pr.svd3(np.zeros((3, 3), np.float32))
    assert list(u) == [0, 0, 1]  # Eigen's U of a zero matrix is the identity


def test_moments_are_sequential_float():
    rng = np.random.default_rng(8)
    P = rng.uniform(-30, 30, (1000, 3)).astype(np.float32)
    mean, cov = pr.moments(P, None, None)
    acc = [np.float32(0)] * 9
    for x, y, z in P:
        for k, v in enumerate([x * x, x * y, x * z, y * y, y * z, z * z, x, y, z]):
            acc[k] = np.float32(acc[k] + v)
    assert mean[0] == acc[6] / np.float32(1000) and cov[2, 2] == acc[5] / np.float32(1000) - (acc[8] / np.float32(1000)) ** 2


def test_sequence_exercises_adaptive_state():
    ref = pr.Patchworkpp()
    decisions, heights = set(), []
    for xyz, inten in gs.sequence(3, frames=12):
        out = ref.estimate_ground(xyz, inten, id=0)
        decisions |= {p["decision"] for p in out["patches"]}
        heights.append(ref.sensor_height)
        assert 0 < len(out["ground"]) and len(out["ground"]) + len(out["nonground"]) <= len(xyz)
    assert {0, 2, 4} <= decisions and len(set(heights)) > 1


def test_rvpf_refused_by_restatement():
    with pytest.raises(ValueError):
        pr.Patchworkpp(enable_RVPF=True)


def test_parameters_that_allow_an_empty_seed_set_are_refused():
    for bad in (dict(num_lpr=0), dict(num_lpr=-1), dict(th_seeds=0.0), dict(th_seeds=-0.5), dict(th_seeds=float("nan"))):
        with pytest.raises(ValueError, match="seeds"):
            pr.Patchworkpp(**bad)
    pr.Patchworkpp(num_lpr=1, th_seeds=1e-3)
    # why: with num_lpr = 0 the LPR height is 0 (PWP:646), and a patch lifted above th_seeds has no seeds.  The reference would fit it
    # with the previous patch's pc_mean_ / cov_; patch_chain (and the kernels) start every patch from zeros.
    ref = pr.Patchworkpp()
    ref.p["num_lpr"] = 0
    xyz, _ = gs.scan(9, n_ground=400, extras=False)
    P = xyz[np.argsort(xyz[:, 2], kind="stable")] + np.array([0, 0, 2.0], np.float32)
    fits, _, _ = ref.patch_chain(1, P, pr.range_covariance(P), 0)
    assert fits[0]["m"] == 0 and not fits[0]["mean"].any() and not fits[0]["cov"].any()
    ref.p["num_lpr"] = 1  # the lowest point is its own LPR and lies below it + th_seeds
    assert ref.patch_chain(1, P, pr.range_covariance(P), 0)[0][0]["m"] >= 1
    assert ref.patch_chain(0, P - np.array([0, 0, 9.0], np.float32), pr.range_covariance(P), 0)[0][0]["m"] == len(P)  # all below the zone-0 margin


def test_binding_refuses_empty_seed_parameters_before_it_looks_for_a_device(gorio):
    for bad in (dict(num_lpr=0), dict(th_seeds=0.0), dict(th_seeds=-1.0)):
        with pytest.raises(gorio.GorioError, match="no seeds") as e:
            gorio.ground.GroundSegmenter(**bad)
        assert "gorio error -1" in str(e.value)


def test_binding_covers_header(gorio):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gorio_ground.h")).read(), flags=re.S)
    assert sorted(gorio.ground.GROUND_SYMBOLS) == sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))


def test_default_params_match_reference(gorio):
    p = gorio.ground.default_params()
    ref = pr.default_params()
    for k in ("num_iter", "num_lpr", "num_min_pts", "sensor_height", "th_seeds", "th_dist", "min_range", "max_range", "uprightness_thr",
              "adaptive_seed_selection_margin", "RNR_ver_angle_thr", "RNR_intensity_thr", "max_flatness_storage", "max_elevation_storage"):
        assert getattr(p, k) == ref[k], k
    assert list(p.num_sectors_each_zone) == [3, 1, 1, 3] and list(p.num_rings_each_zone) == [4, 4, 2, 2]
    assert (p.enable_RNR, p.enable_RVPF, p.enable_TGR) == (1, 0, 1)


def test_no_device_refused(gorio):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(gorio.GorioError) as e:
        gorio.ground.GroundSegmenter()
    assert "gorio error -2" in str(e.value)
