"""Batched ICP aligns on the GPU (gorio_apd_icp_align_batch, go-rio_amd/csrc/apd_icp.hip) on the six batch scenes of tests/icp_scenes.py:
mixed sizes and ICP parameters, ending at different iterations, two members on one shared target, one target from a keyframe, one member
ending with fewer than 3 pairs.  Gates: every handle ends bit for bit where its own align() on a fresh handle ends (pose, counts, diag
values, correspondences), in both search modes; against the restatement the gate of test_icp_gpu.check_align; rounds = the longest
member's passes and at most 3 launches per round without reciprocal correspondences."""
import importlib

import numpy as np
import pytest

import icp_scenes as S
from test_icp_gpu import assert_same_bits, check_align, handle, scene_handle, state_of

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SEARCHES = [apd.SEARCH_BRUTE_FORCE, apd.SEARCH_PRUNED]

_single = {}


def single(gorio, gpu, name, search):
    """The state after align() on a fresh handle with the scene's own uploads, computed once per (scene, search)."""
    if (name, search) not in _single:
        g = scene_handle(gorio, gpu, name, search)
        _single[(name, search)] = state_of(g, g.align(S.scenes()[name]["guess"]))
    return _single[(name, search)]


def guesses(names):
    return np.stack([S.scenes()[n]["guess"] for n in names])


def run_batch(gorio, objs, names):
    res = gorio.icp_align_batch(objs, guesses(names))
    return res, [state_of(g, r) for g, r in zip(objs, res)]


@pytest.mark.parametrize("search", SEARCHES)
def test_mixed_batch(gorio, gpu, search):
    names = S.batch()
    sc = S.scenes()
    store = gorio.KeyframeStore(device=gpu)
    objs = []
    for name in names:
        if name == "batch_513_recip":  # the target of batch_257, shared
            g = handle(gorio, gpu, sc[name]["params"], search, sc[name]["source"])
            g.setInputTargetShared(objs[0])
        elif name == "batch_256_relmse":  # its target from a keyframe
            g = handle(gorio, gpu, sc[name]["params"], search, sc[name]["source"])
            g.setInputTargetKeyframe(store, store.add(sc[name]["target"]))
        else:
            g = scene_handle(gorio, gpu, name, search)
        objs.append(g)
    res, states = run_batch(gorio, objs, names)
    for name, st in zip(names, states):
        assert_same_bits(st, single(gorio, gpu, name, search), name)
        check_align(name, st)
    two = states[names.index("batch_two_pairs")]  # ends at its first pass while the others go on
    assert not two["converged"] and two["nr_iterations"] == 0 and two["diag"]["state"] == 5 and two["diag"]["pairs"] == 2
    assert len({st["nr_iterations"] for st in states}) >= 4
    diag = res[0]["batch_diag"]
    print("mixed batch: %d rounds, %d launches; one by one %d round trips" % (diag["rounds"], diag["launches"], sum(st["n_linearize"] for st in states)))
    assert diag["rounds"] == max(st["n_linearize"] for st in states) == max(st["nr_iterations"] for st in states)
    # one member asks for reciprocal correspondences: its rounds add one launch each
    recip_rounds = states[names.index("batch_513_recip")]["n_linearize"]
    assert diag["launches"] <= 3 * diag["rounds"] + recip_rounds
    # a second batch on the same handles gives the same bits
    _, states2 = run_batch(gorio, objs, names)
    for st, st2 in zip(states, states2):
        assert_same_bits(st2, st, "second batch")


@pytest.mark.parametrize("search", SEARCHES)
def test_launch_budget_without_reciprocal_and_order(gorio, gpu, search):
    names = [n for n in S.batch() if n != "batch_513_recip"][::-1]
    objs = [scene_handle(gorio, gpu, n, search) for n in names]
    res, states = run_batch(gorio, objs, names)
    for name, st in zip(names, states):
        assert_same_bits(st, single(gorio, gpu, name, search), "reversed " + name)
    diag = res[0]["batch_diag"]
    assert diag["rounds"] == max(st["nr_iterations"] for st in states)
    assert diag["launches"] <= 3 * diag["rounds"]
    # a batch of one
    name = "batch_513_roteps"
    g = scene_handle(gorio, gpu, name, search)
    r = gorio.icp_align_batch([g], guesses([name]))
    assert_same_bits(state_of(g, r[0]), single(gorio, gpu, name, search), "batch of one")
    assert r[0]["batch_diag"] == dict(rounds=r[0]["nr_iterations"], launches=3 * r[0]["nr_iterations"])


def test_one_member_in_state_5_leaves_the_others_alone(gorio, gpu):
    search = apd.SEARCH_PRUNED
    names = ["batch_257", "batch_3"]
    with_two = ["batch_two_pairs"] + names
    a = [scene_handle(gorio, gpu, n, search) for n in names]
    b = [scene_handle(gorio, gpu, n, search) for n in with_two]
    _, sa = run_batch(gorio, a, names)
    _, sb = run_batch(gorio, b, with_two)
    for n, x, y in zip(names, sa, sb[1:]):
        assert_same_bits(y, x, n)
    assert sb[0]["diag"]["state"] == 5 and not sb[0]["converged"]
    assert "fewer than 3 correspondences" in b[0]._lib.gorio_apd_last_error(b[0]._h).decode()


def test_refusals_change_nothing(gorio, gpu):
    search = apd.SEARCH_BRUTE_FORCE
    sc = S.scenes()
    n1, n2 = "batch_257", "batch_256_relmse"
    g, g2 = scene_handle(gorio, gpu, n1, search), scene_handle(gorio, gpu, n2, search)
    before = [state_of(g, g.align(sc[n1]["guess"])), state_of(g2, g2.align(sc[n2]["guess"]))]
    plain = gorio.ApdGicp(device=gpu, max_iterations=60, transformation_epsilon=1e-5, corr_dist_threshold=1.0, search=search)
    plain.setInputTarget(sc[n1]["target"])
    plain.setInputSource(sc[n1]["source"])
    other_thr = handle(gorio, gpu, dict(sc[n1]["params"], max_correspondence_distance=0.6), search, sc[n1]["source"], sc[n1]["target"])
    no_source = handle(gorio, gpu, sc[n1]["params"], search, None, sc[n1]["target"])
    cases = [([g, g2, g], INVALID, "handle 2"), ([g, plain, g2], STATE, "handle 1"), ([g, g2, other_thr], INVALID, "handle 2"), ([g, no_source, g2], STATE, "handle 1")]
    for objs, code, where in cases:
        with pytest.raises(gorio.GorioError) as e:
            gorio.icp_align_batch(objs)
        assert e.value.code == code and where in str(e.value), (code, where, str(e.value))
        for h, st in ((g, before[0]), (g2, before[1])):
            corr, sqd = h.getCorrespondences()
            assert h.icp_diag() == st["diag"] and np.array_equal(corr, st["corr"]) and sqd.tobytes() == st["sqd"].tobytes(), where
    assert plain.get_method()["method"] == apd.METHOD_APDGICP
    assert_same_bits(state_of(g, g.align(sc[n1]["guess"])), before[0], "after the refusals")
