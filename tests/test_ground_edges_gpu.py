"""Patchwork++ ground segmentation on the MI355X at its size, geometry and parameter edges: every scene of
tests/ground_edge_scenes.py through GroundSegmenter and through the NumPy restatement (tests/patchwork_restatement.py), compared as
tests/test_ground_gpu.py compares them.  tests/test_ground_edge_scenes.py pins, on the CPU, what each scene holds and its margin."""
import numpy as np
import pytest

import ground_edge_scenes as es
import patchwork_restatement as pr
from ground_checks import _compare_frame, _state_equal

pytestmark = pytest.mark.gpu
SCENES = es.single_scenes()
CASES = [(name, id) for name in SCENES for id in (0, 1) if id == 0 or name not in es.ID0_ONLY]
_REF = {}


@pytest.fixture(scope="module")
def G(gorio, gpu):
    return gorio.ground


def _ref(name, id):
    """The restatement's output for a scene on a fresh object, and that object; computed once."""
    if (name, id) not in _REF:
        xyz, inten, ov = SCENES[name]
        ref = pr.Patchworkpp(**ov)
        _REF[name, id] = (ref.estimate_ground(xyz, inten, id=id), ref)
    return _REF[name, id]


def _check_single(seg, g, ng, name, id):
    xyz = SCENES[name][0]
    out, ref = _ref(name, id)
    if id == 1:
        assert out["margin"] > 1e-4, out["margin"]
    _compare_frame(seg, out, xyz, id)
    np.testing.assert_array_equal(g, out["ground"])
    np.testing.assert_array_equal(ng, out["nonground"])
    _state_equal(seg, ref)


@pytest.mark.parametrize("name,id", CASES)
def test_edge_scene_matches_restatement(G, name, id):
    xyz, inten, ov = SCENES[name]
    seg = G.GroundSegmenter(**ov)
    g, ng = seg.estimate(xyz, inten, id=id)
    _check_single(seg, g, ng, name, id)
    dg = seg.diagnostics()
    if name.startswith("ties_"):  # the tie rule itself: (z, input index), -0 with +0
        fitted = 0
        for p in dg["patches"]:
            if p["n_fits"]:
                idx = dg["patch_order"][p["segment_offset"]:p["segment_offset"] + p["n_points"]]
                members = np.sort(idx)
                np.testing.assert_array_equal(idx, members[np.lexsort((members, xyz[members, 2]))])
                fitted += 1
        assert fitted >= 10
    if name.startswith("exact_counts"):
        n = [p["n_points"] for p in dg["patches"]]
        assert sorted(c for c in n if c > 8192) == [8193, 8194, 16385] and 8192 in n and 8191 in n  # three patches sorted in the global scratch
    if name == "grid_512":
        assert dg["frame"]["n_patches"] == 512 and all(p["n_fits"] == (9 if p["n_points"] else 0) for p in dg["patches"])


@pytest.mark.parametrize("id", [0, 1])
@pytest.mark.parametrize("name", sorted(es.SWITCHES))
def test_switch_sequence_matches_restatement(G, name, id):
    frames, ov = es.switches()[name]
    seg, ref = G.GroundSegmenter(**ov), pr.Patchworkpp(**ov)
    for xyz, inten in frames:
        g, ng = seg.estimate(xyz, inten, id=id)
        out = ref.estimate_ground(xyz, inten, id=id)
        if id == 1:
            assert out["margin"] > 1e-4, out["margin"]
        _compare_frame(seg, out, xyz, id)
        np.testing.assert_array_equal(g, out["ground"])
        np.testing.assert_array_equal(ng, out["nonground"])
        _state_equal(seg, ref)


def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("id", [0, 1])
def test_mixed_batch(G, id):
    """Five handles with different grids and fit counts in one launch; the global-sort patches are in scans 1 and 4, so the later
    scans' key and patch offsets count what the earlier ones used."""
    names = ["grid_4", "exact_counts", "ladder_n1", "grid_512", "exact_counts_b"]
    segs = [G.GroundSegmenter(**SCENES[k][2]) for k in names]
    outs = G.estimate_batch(segs, [SCENES[k][:2] for k in names], id=id)
    for k, s, (g, ng) in zip(names, segs, outs):
        _check_single(s, g, ng, k, id)
        one = G.GroundSegmenter(**SCENES[k][2])
        g1, ng1 = one.estimate(*SCENES[k][:2], id=id)
        _same([g, ng], [g1, ng1])
        _same(s.diagnostics(), one.diagnostics())
        _same(s.get_state(), one.get_state())


def test_parameter_errors(G, gorio):
    xyz, inten = SCENES["ladder_n1025"][:2]
    seg, ref = G.GroundSegmenter(), pr.Patchworkpp()
    bad = [(dict(num_sectors_each_zone=[32, 32, 32, 1], num_rings_each_zone=[4, 4, 4, 129]), "512"),  # 513 patches
           (dict(num_iter=0), "num_iter"), (dict(num_iter=9), "num_iter"), (dict(num_min_pts=0), "num_min_pts"),
           (dict(num_lpr=0), "no seeds"), (dict(th_seeds=0.0), "no seeds"), (dict(th_seeds=-0.1), "no seeds")]
    for ov, text in bad:
        with pytest.raises(gorio.GorioError, match=text) as e:
            G.GroundSegmenter(**ov)
        assert "gorio error -1" in str(e.value)
        g, ng = seg.estimate(xyz, inten, id=0)  # the handle made before still works, frame after frame
        out = ref.estimate_ground(xyz, inten, id=0)
        _compare_frame(seg, out, xyz, 0)
        np.testing.assert_array_equal(g, out["ground"])
        np.testing.assert_array_equal(ng, out["nonground"])
        _state_equal(seg, ref)
    G.GroundSegmenter(num_sectors_each_zone=[32, 32, 32, 1], num_rings_each_zone=[4, 4, 4, 128], num_iter=8, num_min_pts=1, num_lpr=1, th_seeds=1e-3)  # 512: the edge
    for ov in (dict(num_lpr=0), dict(th_seeds=0.0)):
        with pytest.raises(ValueError):
            pr.Patchworkpp(**ov)
