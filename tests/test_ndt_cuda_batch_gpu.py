"""gorio_apd_align_batch over GORIO_METHOD_NDT_CUDA handles: a batch returns the single aligns' bits; differing settings are refused."""
import importlib

import numpy as np
import pytest

import ndt_cuda_restatement as nr

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu
F = np.float32


def handles(gorio, gpu, count, mode, opt):
    """`count` handles of ragged sizes: every handle its own sub-sampling of the scene pair and its own guess"""
    src, tgt, _ = nr.scene_pair(4096)
    rng = np.random.default_rng(count)
    out, guesses = [], []
    for q in range(count):
        ns, nt = 700 + 211 * q, 4096 - 97 * q
        g = gorio.ApdGicp(device=gpu, optimizer=opt)
        g.set_ndt_cuda_params(mode)
        g.set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT7)
        g.setInputSource(src[rng.permutation(4096)[:ns]])
        g.setInputTarget(tgt[:nt])
        out.append(g)
        guesses.append(nr.known_transform(0.02 * (q % 5), -0.01 * (q % 3), 0.0, 0.004 * (q % 4), 0.0))
    return out, np.array(guesses, F)


@pytest.mark.parametrize("count,mode,opt", [(3, nr.D2D, apd.OPT_LEVENBERG_MARQUARDT), (3, nr.P2D, apd.OPT_GAUSS_NEWTON), (17, nr.P2D, apd.OPT_LEVENBERG_MARQUARDT),
                                            (17, nr.D2D, apd.OPT_GAUSS_NEWTON)])
def test_batch_equals_single_aligns(gorio, gpu, count, mode, opt):
    hs, guesses = handles(gorio, gpu, count, mode, opt)
    batch = gorio.align_batch(hs, guesses)
    pairs = [h.ndt_cuda_pairs() for h in hs]
    for q, h in enumerate(hs):
        one = h.align(guesses[q])
        assert one["T"].tobytes() == batch[q]["T"].tobytes() and one["H"].tobytes() == batch[q]["H"].tobytes(), q
        assert (one["converged"], one["nr_iterations"], one["n_linearize"]) == (batch[q]["converged"], batch[q]["nr_iterations"], batch[q]["n_linearize"])
        assert np.array_equal(h.ndt_cuda_pairs(), pairs[q])
    assert len({b["n_linearize"] for b in batch}) > 1 or count == 3  # ragged work: the pairs do not all end together


def test_batch_with_differing_settings_is_refused(gorio, gpu):
    hs, guesses = handles(gorio, gpu, 3, nr.D2D, apd.OPT_LEVENBERG_MARQUARDT)
    before = gorio.align_batch(hs, guesses)
    for change in ("mode", "resolution", "search", "method"):
        if change == "mode":
            hs[1].set_ndt_cuda_params(nr.P2D)
        elif change == "resolution":
            hs[1].set_method(apd.METHOD_NDT_CUDA, 2.0, apd.VOXEL_DIRECT7)
        elif change == "search":
            hs[1].set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT27)
        else:
            hs[1].set_method(apd.METHOD_VGICP, 1.0, apd.VOXEL_DIRECT7)
        with pytest.raises(gorio.GorioError) as e:
            gorio.align_batch(hs, guesses)
        assert e.value.code == -1, change
        hs[1].set_ndt_cuda_params(nr.D2D)
        hs[1].set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT7)
    after = gorio.align_batch(hs, guesses)  # a refused batch changed nothing
    for a, b in zip(before, after):
        assert a["T"].tobytes() == b["T"].tobytes()
