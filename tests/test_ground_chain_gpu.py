"""The preprocessing nodelet's chain with ground segmentation in place (PREP:502-568): distance filter -> StatisticalOutlierRemoval ->
Patchwork++ -> full_scan = ground + nonground -> DBSCAN labels -> APD-GICP, on the GPU and through the CPU restatements."""
import numpy as np
import pytest

import ground_scenes as gs
import patchwork_restatement as pr

pytestmark = pytest.mark.gpu


def _pose(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    T = np.eye(4)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = t
    return T


def test_chain_with_ground_segmentation_matches_restatements(gpu, gorio, oracle_apd, pose_err):
    xyz, inten = gs.scan(93, n_ground=7000)
    rng = np.random.default_rng(94)
    T_gt = _pose(0.02, (0.3, -0.1, 0.0))
    picks = [rng.random(len(xyz)) < 0.75, rng.random(len(xyz)) < 0.75]
    seg, ref = gorio.ground.GroundSegmenter(), pr.Patchworkpp()
    made = []
    for k, pick in enumerate(picks):
        p, i = xyz[pick], inten[pick]
        if k == 1:
            p = (p.astype(np.float64) @ T_gt[:3, :3].T + T_gt[:3, 3]).astype(np.float32)
        d = np.linalg.norm(p.astype(np.float64), axis=1)
        keep = (d > 0.5) & (d < 100.0)  # distance_filter
        p, i = p[keep], i[keep]
        k_g = gorio.prep.statistical_outlier_mask(p, 20, 1.0)
        k_o, _ = oracle_apd.statistical_outlier_mask(p, 20, 1.0)
        assert np.array_equal(k_g, k_o)
        p, i = np.ascontiguousarray(p[k_g]), i[k_g]
        g, ng = seg.estimate(p, i, id=1)
        out = ref.estimate_ground(p, i, id=1)
        assert out["margin"] > 1e-4
        assert np.array_equal(g, out["ground"]) and np.array_equal(ng, out["nonground"])
        full = np.ascontiguousarray(p[np.concatenate([g, ng])])  # PREP:519
        l_g, nc = gorio.prep.dbscan_labels(full)
        l_o, nc_o = oracle_apd.dbscan_labels(full)
        assert nc == nc_o and np.array_equal(l_g, l_o)
        made.append((full, l_g))
    (a, la), (b, lb) = made
    assert len(a) > 3000 and la.max() >= 1
    p = oracle_apd.launch_params()
    ro = oracle_apd.align(np.eye(4), a, la, b, lb, oracle_apd.calculate_covariances(a, p), oracle_apd.calculate_covariances(b, p), p)
    gi = gorio.ApdGicp(corr_dist_threshold=2.0, transformation_epsilon=0.1, search=1)
    gi.setInputTarget(b, lb)
    gi.setInputSource(a, la)
    r = gi.align()
    te, re = pose_err(ro["T"], r["T"])
    assert te < 1e-4 and re < 1e-4 and r["converged"] == ro["converged"]
