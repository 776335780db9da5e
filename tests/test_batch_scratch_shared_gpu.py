"""The lock-step batched aligns keep their round table, partials and sums in ONE scratch of the handle that leads the batch
(gorio_apd::RoundScratch, go-rio_amd/csrc/apd_batch_rounds.hip), whatever the method.  One lead handle on the 257-point and a second handle
on the 3-point ICP batch scene run an ICP batch, then -- switched with set_method, on the same clouds -- a GICP_OMP batch, then the ICP
batch again.  Gates: every member of every batch ends bit for bit where a fresh handle's own align() in that method ends, the third batch
equals the first, and each batch_diag read after a batch of its own method is the one a fresh lead handle reports.  The pruned search
gives the 3-point member a padding workgroup (nwg 2, nblk 1).  The 3-point source carries covariances of its own (setSourceCovariances):
a cloud smaller than k_correspondences cannot estimate any, and with them GICP_OMP takes it and ends at its first update with fewer than
4 pairs while the 257-point member goes on."""
import ctypes as C
import importlib

import numpy as np
import pytest

import icp_scenes as S
import test_gicp_omp_batch_gpu as O
import test_icp_gpu as I

pytestmark = pytest.mark.gpu
apd = importlib.import_module("go-rio_amd.apd")
NAMES = ["batch_257", "batch_3"]
SEARCH = apd.SEARCH_PRUNED


def to_icp(g, name):
    p = S.scenes()[name]["params"]
    g.set_method(apd.METHOD_ICP)
    g.set_icp_params(p.get("use_reciprocal", False), p.get("euclidean_fitness_epsilon", -np.finfo(np.float64).max), p.get("transformation_rotation_epsilon", 0.0))


def fresh(gorio, gpu, name, method):
    g = I.scene_handle(gorio, gpu, name, SEARCH)
    if name == "batch_3":
        g.setSourceCovariances(np.tile(np.eye(4), (3, 1, 1)))
    if method == apd.METHOD_GICP_OMP:
        g.set_method(method)
    return g


def test_icp_then_gicp_omp_then_icp_on_one_lead(gorio, gpu):
    sc = S.scenes()
    guesses = np.stack([sc[n]["guess"] for n in NAMES])
    batch = {apd.METHOD_ICP: gorio.icp_align_batch, apd.METHOD_GICP_OMP: gorio.gicp_omp_align_batch}
    mod = {apd.METHOD_ICP: I, apd.METHOD_GICP_OMP: O}
    want, want_diag = {}, {}
    for method in batch:  # a fresh handle's own align() per member, and the batch_diag of a fresh lead
        singles = [fresh(gorio, gpu, n, method) for n in NAMES]
        want[method] = [mod[method].state_of(g, g.align(sc[n]["guess"])) for g, n in zip(singles, NAMES)]
        want_diag[method] = batch[method]([fresh(gorio, gpu, n, method) for n in NAMES], guesses)[0]["batch_diag"]
    assert not want[apd.METHOD_GICP_OMP][1]["converged"] and want[apd.METHOD_GICP_OMP][0]["n_linearize"] > 0  # the members end rounds apart

    objs = [fresh(gorio, gpu, n, apd.METHOD_ICP) for n in NAMES]
    seen = []
    for step, method in enumerate([apd.METHOD_ICP, apd.METHOD_GICP_OMP, apd.METHOD_ICP]):
        for g, n in zip(objs, NAMES):
            g.set_method(method) if method == apd.METHOD_GICP_OMP else to_icp(g, n)
        res = batch[method](objs, guesses)
        states = [mod[method].state_of(g, r) for g, r in zip(objs, res)]
        for n, st, w in zip(NAMES, states, want[method]):
            mod[method].assert_same_bits(st, w, "batch %d, %s" % (step, n))
        assert [r["batch_diag"] for r in res] == [want_diag[method]] * len(objs), step
        seen.append(states)
    for n, a, b in zip(NAMES, seen[0], seen[2]):
        I.assert_same_bits(b, a, "third batch against the first, " + n)
    # the GICP_OMP counters of the lead outlive the ICP batch it led afterwards
    rounds, launches = C.c_int(-1), C.c_int(-1)
    assert objs[0]._lib.gorio_apd_gicp_omp_batch_diag(objs[0]._h, C.byref(rounds), C.byref(launches)) == 0
    assert dict(rounds=rounds.value, launches=launches.value) == want_diag[apd.METHOD_GICP_OMP]
