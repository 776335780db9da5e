"""CPU checks that every scene of tests/ground_edge_scenes.py has the property it is named for, through the restatement alone
(tests/patchwork_restatement.py), and the margin of every scene the GPU tests run with id = 1."""
import functools

import numpy as np
import pytest

import ground_edge_scenes as es
import patchwork_restatement as pr

SCENES = es.single_scenes()
MAX = np.finfo(np.float64).max


@functools.lru_cache(maxsize=None)
def _run(name, id):
    xyz, inten, ov = SCENES[name]
    return pr.Patchworkpp(**ov).estimate_ground(xyz, inten, id=id)


# radii 1, nextafter(1), 2.53125, 7.125, 13.25, 25.5, 50, nextafter(50); per radius (r, +0), (r, -0), (0, r), (-r, +0), (-r, -0), (0, -r);
# then the origin; then (a, a), (-a, a), (-a, -a), (a, -a) for a = 2, 5, 10, 20.  r == min_range is outside, r == max_range is in the
# last ring, (r, +-0) is in the LAST sector (theta = 2 pi), (-r, -0) and (-r, +0) share a sector, a point on a sector boundary
# belongs to the sector that starts there.
BOUNDARY_LABELS = {
    (4, 4, 4, 4): [-1, -1, -1, -1, -1, -1, 3, 3, 1, 2, 2, 3, 7, 7, 5, 6, 6, 7, 19, 19, 17, 18, 18, 19, 35, 35, 33, 34, 34, 35, 43, 43, 41, 42, 42, 43,
                   47, 47, 45, 46, 46, 47, -1, -1, -1, -1, -1, -1, -2, 4, 5, 6, 7, 12, 13, 14, 15, 32, 33, 34, 35, 40, 41, 42, 43],
    (3, 1, 1, 3): [-1, -1, -1, -1, -1, -1, 2, 2, 0, 1, 1, 2, 5, 5, 3, 4, 4, 5, 12, 12, 12, 12, 12, 12, 16, 16, 16, 16, 16, 16, 20, 20, 18, 19, 19, 20,
                   23, 23, 21, 22, 22, 23, -1, -1, -1, -1, -1, -1, -2, 3, 4, 4, 5, 9, 10, 10, 11, 16, 16, 16, 16, 18, 19, 19, 20],
}


@pytest.mark.parametrize("sectors", list(BOUNDARY_LABELS))
def test_boundary_labels(sectors):
    geo = es.geometry()
    assert es.boundary_radii(geo) == [1.0, float(np.nextafter(np.float32(1), np.float32(2))), 2.53125, 7.125, 13.25, 25.5, 50.0,
                                      float(np.nextafter(np.float32(50), np.float32(60)))]
    sp, _ = es.boundary_special(sectors)
    assert np.signbit(sp[1, 1]) and not np.signbit(sp[0, 1]) and np.signbit(sp[4, 1]) and sp[1, 1] == 0  # the -0.0 survive the float cast
    out = _run("boundary_%d%d%d%d" % sectors, 0)
    assert [int(v) for v in out["labels"][-len(sp):]] == BOUNDARY_LABELS[sectors]
    assert sum("fits" in p for p in out["patches"]) >= 12 and len(out["ground"]) > 2000  # the patches around them still fit planes


def test_rnr_threshold_labels():
    # intensity below / at / above float32(0.1): float32(0.1) > 0.1, so only the lower neighbour is noise; z below / at / above -1.5;
    # two floats on each side of -15 degrees
    out = _run("rnr", 0)
    assert [int(v) for v in out["labels"][-10:]] == [-2, 3, 3, -2, 0, 0, -2, -2, 12, 12]
    sp, si = es.rnr_special()
    assert float(si[1]) > 0.1 > float(si[0]) and sp[4, 2] == np.float32(-1.5)
    assert np.all(np.diff(sp[6:10, 2].view(np.int32)) == -1)  # four adjacent negative floats, rising


def test_size_ladder():
    L = es.size_ladder()
    assert [len(L["n%d" % k][0]) for k in es.LADDER] == [1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025]
    assert np.array_equal(L["n1025"][0][:17], L["n17"][0])
    out = _run("ladder_outside", 0)
    assert np.all(out["labels"] == -1) and len(out["ground"]) == 0 and out["final"]["m"] == 0
    out = _run("ladder_noise", 0)
    assert np.all(out["labels"] == -2) and len(out["ground"]) == 0 and out["final"]["m"] == 0
    assert all(p["n_points"] == 0 for p in out["patches"])
    assert len(out["nonground"]) == 150  # all 300 lie more than 1 m under z = 0, the plane of the zero moments: every second is erased
    out = _run("ladder_n1025", 0)
    assert sum("fits" in p for p in out["patches"]) == 15 and out["final"]["m"] == 717


def test_exact_patch_counts():
    want = {0: 255, 1: 8193, 2: 9, 4: 256, 6: 16385, 9: 10, 11: 8191, 13: 257, 16: 8192, 21: 8194}
    for name in ("exact_counts", "exact_counts_b"):
        out = _run(name, 0)
        assert len(SCENES[name][0]) == 49942
        assert {q: p["n_points"] for q, p in enumerate(out["patches"]) if p["n_points"]} == want
        big = [q for q, p in enumerate(out["patches"]) if p["n_points"] > 8192]
        assert big == [1, 6, 21]  # 8192 itself still sorts in LDS
        between = [out["patches"][q] for q in range(big[0] + 1, big[1])]
        assert any(0 < p["n_points"] < 10 and "fits" not in p for p in between) and any(p["n_points"] == 256 and "fits" in p for p in between)
        assert [p["n_points"] for p in out["patches"] if "fits" in p] == [255, 8193, 256, 16385, 10, 8191, 257, 8192, 8194]
        order = out["patch_order"][:8]
        assert not np.array_equal(order, np.sort(order))  # shuffled input
    out = _run("exact_selected", 0)
    fitted = {q: [f["m"] for f in p["fits"]] for q, p in enumerate(out["patches"]) if "fits" in p}
    assert fitted == {1: [255] * 5, 5: [256] * 5, 14: [257] * 5}
    assert {q: out["patches"][q]["n_points"] for q in fitted} == {1: 355, 5: 356, 14: 357}


def _tie_groups(out, xyz, q):
    p = out["patches"][q]
    idx = out["patch_order"][p["segment_offset"]:p["segment_offset"] + p["n_points"]]
    return idx, xyz[idx, 2]


def test_z_ties():
    for k in "abcde":
        xyz = SCENES["ties_" + k][0]
        out = _run("ties_" + k, 0)
        for q, p in enumerate(out["patches"]):
            if "fits" in p:
                idx, z = _tie_groups(out, xyz, q)
                assert np.array_equal(idx, idx[np.lexsort((idx, z))])
    xyz = SCENES["ties_a"][0]
    out = _run("ties_a", 0)
    assert np.all(xyz[:, 2] * 16 == np.round(xyz[:, 2] * 16))
    for q, p in enumerate(out["patches"]):
        if "fits" in p:
            assert len(np.unique(_tie_groups(out, xyz, q)[1])) < p["n_points"] // 2  # most points tie with another
    xyz = SCENES["ties_b"][0]
    out = _run("ties_b", 0)
    idx, z = _tie_groups(out, xyz, es.TIE_PATCH)
    zero = idx[z == 0]
    neg = np.signbit(xyz[zero, 2])
    assert len(zero) == 40 and neg.sum() == 20 and np.all(np.diff(zero) > 0)  # +0 and -0 are one tie group, in input order
    assert np.sum(neg[1:] != neg[:-1]) > 10  # and interleaved in it
    out = _run("ties_c", 0)
    assert np.all(SCENES["ties_c"][0][:, 2] == np.float32(-0.7))
    for p in out["patches"]:
        if "fits" in p:
            f = p["fits"][-1]
            # the float sums of m <= 1200 equal terms 0.49 round, so zz is not exactly 0 but at most m x 2^-24 x 0.49 x 2 < 1e-4 of noise
            assert f["m"] <= 1200 and abs(f["cov"][2, 2]) < 1e-4 and f["sv"][2] < 1e-4 < f["sv"][1]
    out = _run("ties_d", 0)
    p = out["patches"][es.LINE_PATCH]
    f = p["fits"][-1]
    assert p["n_points"] == 16 and f["sv"][0] > 0 and f["sv"][1] == 0 and f["sv"][2] == 0
    assert p["line_variable"] == MAX and p["decision"] == 6  # a TGR candidate, rejected by its line variable
    out = _run("ties_e", 0)
    p = out["patches"][es.LINE_PATCH]
    idx, z = _tie_groups(out, SCENES["ties_e"][0], es.LINE_PATCH)
    assert p["n_points"] == 12 >= 10 and "fits" in p and len(np.unique(SCENES["ties_e"][0][idx], axis=0)) == 1
    assert np.array_equal(idx, np.arange(500, 512))


def test_elevated_only_patch():
    xyz = SCENES["elevated"][0]
    for id in (0, 1):
        out = _run("elevated", id)
        p = out["patches"][es.ELEVATED_PATCH]
        m = [f["m"] for f in p["fits"]]
        assert p["n_points"] == 60 and m[0] > 0 and m[1:] == [0, 0, 0, 0] and p["n_ground"] == 0
        for f in p["fits"][1:]:  # the empty fits keep the patch's own first moments
            assert np.array_equal(f["mean"], p["fits"][0]["mean"]) and np.array_equal(f["cov"], p["fits"][0]["cov"])
            assert f["iters"] == 0
    idx, z = _tie_groups(out, xyz, es.ELEVATED_PATCH)
    assert float(z[0]) >= -0.7 + 0.5 > float(np.nextafter(z[0], np.float32(-1)))


def test_under_ground_run():
    xyz, _, _ = SCENES["under_run"]
    out = _run("under_run", 0)
    assert np.all(out["labels"][:es.UNDER_RUN + 1] == -1) and not np.any(out["labels"] == -2)
    assert np.all(xyz[:es.UNDER_RUN, 2] == -5) and xyz[es.UNDER_RUN, 2] == 1
    # 0, 2, 4 erased; 1, 3, 5 slide into the erased slots and are never tested although they lie as deep; 6 is tested and kept
    assert list(out["nonground"][:4]) == [1, 3, 5, 6]
    assert not {0, 2, 4} & set(out["nonground"].tolist())


def test_grids():
    out = _run("grid_512", 0)
    assert len(out["patches"]) == 512
    counts = np.bincount([p["n_points"] for p in out["patches"]])
    assert counts[0] > 50 and counts[1] > 50 and counts[2] > 25
    assert all(("fits" in p) == (p["n_points"] > 0) and (p["n_points"] == 0 or len(p["fits"]) == 9) for p in out["patches"])
    assert max(q for q, p in enumerate(out["patches"]) if "fits" in p) > 500  # the last columns of the count table are in use
    out = _run("grid_4", 0)
    assert len(out["patches"]) == 4 and all("fits" in p for p in out["patches"])


@functools.lru_cache(maxsize=None)
def _run_switch(name, id):
    frames, ov = es.switches()[name]
    ref = pr.Patchworkpp(**ov)
    outs, lens = [], []
    for xyz, inten in frames:
        outs.append(ref.estimate_ground(xyz, inten, id=id))
        lens.append(([len(v) for v in ref.upd_elev], [len(v) for v in ref.upd_flat]))
    return outs, lens


def test_switches_act():
    assert sorted(es.switches()) == ["iter_1", "lpr_1", "rnr_off", "storage_0", "storage_3", "tgr_off"]
    assert all(len(fr) == 8 for fr, _ in es.switches().values())
    outs, lens = _run_switch("tgr_off", 0)
    assert 6 in {p["decision"] for o in outs for p in o["patches"]} and 5 not in {p["decision"] for o in outs for p in o["patches"]}
    assert max(max(e) for e, _ in lens) > 3  # untrimmed, the lists outgrow 3 ...
    outs, lens = _run_switch("storage_3", 0)
    assert lens[-1] == ([3, 3, 3, 3], [3, 3, 3, 3])  # ... and the trim cuts them
    outs, lens = _run_switch("storage_0", 0)
    assert lens[-1][0] == [0, 0, 0, 0]
    outs, _ = _run_switch("rnr_off", 0)
    assert not any(np.any(o["labels"] == -2) for o in outs)
    outs, _ = _run_switch("tgr_off", 0)
    assert all(np.any(o["labels"] == -2) for o in outs)  # the same frames do hold RNR noise
    outs, _ = _run_switch("iter_1", 0)
    assert {len(p["fits"]) for o in outs for p in o["patches"] if "fits" in p} == {2}


# The smallest distance of a quantity that decides on the LM plane to its threshold (estimate_ground's "margin"), id = 1, as computed
# here.  The GPU tests require > 1e-4 of every scene they run with id = 1; the seeds in tests/ground_edge_scenes.py were chosen for it.
MARGINS = {
    "boundary_4444": 0.222855, "boundary_3113": 0.103295, "rnr": 0.074528,
    "ladder_n15": 0.21236, "ladder_n16": 0.21236, "ladder_n17": 0.21236, "ladder_n63": 0.094538, "ladder_n64": 0.094538, "ladder_n65": 0.094538,
    "ladder_n1023": 0.131081, "ladder_n1024": 0.131081, "ladder_n1025": 0.131081,
    "exact_counts": 0.499855, "exact_counts_b": 0.499938, "exact_selected": 0.499979, "ties_a": 0.235949, "ties_b": 0.250404,
    "elevated": 0.0908208, "under_run": 0.499983, "grid_512": 0.00722253, "grid_4": 0.117929,
}
SWITCH_MARGINS = {"rnr_off": 0.000169665, "tgr_off": 0.000169665, "iter_1": 0.000169665, "lpr_1": 0.000313759, "storage_3": 0.000169665,
                  "storage_0": 0.000169665}


def test_every_scene_is_listed():
    assert sorted(MARGINS) == sorted(set(SCENES) - set(es.ID0_ONLY))
    assert sorted(es.ID0_ONLY) == ["ladder_n1", "ladder_n2", "ladder_noise", "ladder_outside", "ties_c", "ties_d", "ties_e"]
    assert sorted(SWITCH_MARGINS) == sorted(es.SWITCHES)


@pytest.mark.parametrize("name", sorted(MARGINS))
def test_margin_of_id1_scene(name):
    m = _run(name, 1)["margin"]
    assert m > 1e-4
    assert m == pytest.approx(MARGINS[name], rel=1e-3)


@pytest.mark.parametrize("name", sorted(SWITCH_MARGINS))
def test_margin_of_id1_sequence(name):
    m = min(o["margin"] for o in _run_switch(name, 1)[0])
    assert m > 1e-4
    assert m == pytest.approx(SWITCH_MARGINS[name], rel=1e-3)
