"""Patchwork++ ground segmentation on the MI355X (include/gorio_ground.h) against the NumPy restatement
(tests/patchwork_restatement.py)."""
import os

import numpy as np
import pytest

import ground_scenes as gs
from ground_checks import _compare_frame, _state_equal
import patchwork_restatement as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def G(gorio, gpu):
    return gorio.ground


def _real(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", "real_lidar_pair.npz"))[name]
    return d[:, :3].astype(np.float32), d[:, 3].astype(np.float32)


@pytest.mark.parametrize("id", [0, 1])
@pytest.mark.parametrize("scene", ["scan", "sparse", "real_a0", "real_b1", "large"])
def test_single_scan_matches_restatement(G, scene, id):
    h = 0.7
    if scene == "scan":
        xyz, inten = gs.scan(11)
    elif scene == "sparse":
        xyz, inten = gs.sparse_far_scan(12)
    elif scene == "large":
        xyz, inten = gs.large_scan(13)
    else:
        xyz, inten = _real({"real_a0": "a_0", "real_b1": "b_1"}[scene])
        h = 2.3
    seg = G.GroundSegmenter(sensor_height=h)
    ref = pr.Patchworkpp(sensor_height=h)
    g, ng = seg.estimate(xyz, inten, id=id)
    out = ref.estimate_ground(xyz, inten, id=id)
    assert out["margin"] > 1e-4, out["margin"]
    _compare_frame(seg, out, xyz, id)
    np.testing.assert_array_equal(g, out["ground"])
    np.testing.assert_array_equal(ng, out["nonground"])
    _state_equal(seg, ref)
    if scene == "large":
        assert max(p["n_points"] for p in seg.diagnostics()["patches"]) > 8192  # the global-memory sort ran


@pytest.mark.parametrize("id", [0, 1])
def test_sequence_state_after_every_frame(G, id):
    seg, ref = G.GroundSegmenter(), pr.Patchworkpp()
    decisions = set()
    for xyz, inten in gs.sequence(3, frames=24):
        g, ng = seg.estimate(xyz, inten, id=id)
        out = ref.estimate_ground(xyz, inten, id=id)
        assert out["margin"] > 1e-4
        np.testing.assert_array_equal(g, out["ground"])
        np.testing.assert_array_equal(ng, out["nonground"])
        _state_equal(seg, ref)
        decisions |= {p["decision"] for p in out["patches"]}
    assert {4, 5, 6} & decisions  # A-GLE and TGR acted


def test_set_state_then_estimate(G):
    xyz, inten = gs.scan(21)
    st = dict(elevation_thr=[-0.5, -0.45, -0.4, -0.4], flatness_thr=[0.002, 0.003, 0.004, 0.005], sensor_height=0.68,
              update_elevation=[[-0.7, -0.69], [-0.6], [], [-0.5, -0.52, -0.51]], update_flatness=[[0.001, 0.002], [0.003], [], [0.004, 0.0041, 0.0039]])
    seg, ref = G.GroundSegmenter(), pr.Patchworkpp()
    seg.set_state(**st)
    ref.set_state(**st)
    _state_equal(seg, ref)
    g, ng = seg.estimate(xyz, inten)
    out = ref.estimate_ground(xyz, inten)
    np.testing.assert_array_equal(g, out["ground"])
    np.testing.assert_array_equal(ng, out["nonground"])
    _state_equal(seg, ref)


@pytest.mark.parametrize("id", [0, 1])
def test_batch_is_bitwise_single(G, id):
    scenes = [gs.scan(31 + k) for k in range(3)] + [gs.sparse_far_scan(40)]
    singles = []
    for xyz, inten in scenes:
        s = G.GroundSegmenter()
        singles.append((s.estimate(xyz, inten, id=id), s.get_state(), s.diagnostics()))
    segs = [G.GroundSegmenter() for _ in scenes]
    outs = G.estimate_batch(segs, scenes, id=id)
    for s, (g, ng), ((g1, ng1), st1, dg1) in zip(segs, outs, singles):
        np.testing.assert_array_equal(g, g1)
        np.testing.assert_array_equal(ng, ng1)
        dg = s.diagnostics()
        np.testing.assert_array_equal(dg["frame"]["final_normal"], dg1["frame"]["final_normal"])
        assert dg["frame"]["final_d"] == dg1["frame"]["final_d"]
        for a, b in zip(dg["patches"], dg1["patches"]):
            np.testing.assert_array_equal(a["normal"], b["normal"])
            np.testing.assert_array_equal(a["lm_iterations"], b["lm_iterations"])
        assert s.get_state()["sensor_height"] == st1["sensor_height"]


def test_errors(G, gorio):
    import ctypes as C

    p = G.default_params()
    p.enable_RVPF = 1
    with pytest.raises(gorio.GorioError, match="RVPF"):
        G.GroundSegmenter(params=p)
    seg = G.GroundSegmenter()
    with pytest.raises(gorio.GorioError):
        seg.estimate(np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
    lib = gorio.load_library()
    ng, no = C.c_int(), C.c_int()
    assert lib.gorio_ground_estimate(seg.h, None, None, 10, 16, 1, None, C.byref(ng), C.byref(no)) == -1
    xyz, inten = gs.scan(5)
    with pytest.raises(gorio.GorioError, match="twice"):
        G.estimate_batch([seg, seg], [(xyz, inten), (xyz, inten)])
    bad = xyz.copy()
    bad[3, 2] = np.nan
    with pytest.raises(gorio.GorioError, match="non-finite"):
        seg.estimate(bad, inten)
    with pytest.raises(gorio.GorioError):
        seg.estimate(xyz, inten, id=2)

