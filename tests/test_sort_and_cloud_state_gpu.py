"""The tiled key sort where it changes shape, reached through its two single-array callers, and the state of a cloud whose points are
replaced.

Sort sizes (keys are padded to a power of two of at least one 4096-key tile): 1 = one partly filled tile, 4095, 4096 = exactly one tile,
4097 = two tiles, the first size with a stage through global memory, 8193 = four tiles, the first with two merge sizes.

  * submap assembly (gorio_apd_set_target_submap with a voxel grid) against oracle_apd.submap_assemble, bit for bit;
  * the FastVGICP voxel map (gorio_apd_get_voxelmap) against the restatement's, by the comparison of test_vgicp_map_slots_linearize;
  * new points make a cloud's covariances, search index and k-NN lists stale whichever setter brings them: the lists are refused and
    the next align equals the align of a fresh handle, bit for bit.
"""
import ctypes as C
import importlib

import numpy as np
import pytest

import gicp_restatement as gr
import gicp_scenes as gs
from test_gicp_variants_gpu import check_map

synth = importlib.import_module("go-rio_amd.synth")
apd = importlib.import_module("go-rio_amd.apd")

pytestmark = pytest.mark.gpu

N_BAD = 37  # non-finite points of the first keyframe


@pytest.fixture(scope="module")
def scan():
    return synth.radar_scan(8193, seed=911)


@pytest.mark.parametrize("m", [1, 4095, 4096, 4097, 8193])
def test_submap_voxel_sort_sizes(gpu, gorio, oracle_apd, scan, m):
    """m finite points in two keyframes; the first one also carries N_BAD non-finite points, which the staging drops: the second frame's
    staged offset differs from its offset in the input."""
    xyz, lab = scan
    a = m // 2  # finite points of the first frame (none for m = 1)
    x0 = np.empty((a + N_BAD, 3), np.float32)
    l0 = np.zeros(a + N_BAD, np.float32)
    bad = np.zeros(a + N_BAD, bool)
    bad[np.linspace(0, a + N_BAD - 1, N_BAD).astype(int)] = True
    x0[~bad], l0[~bad] = xyz[:a], lab[:a]
    x0[bad] = xyz[:N_BAD]
    x0[bad, np.arange(N_BAD) % 3] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(N_BAD) % 3]
    frames = [(x0, l0), (xyz[a:m].copy(), lab[a:m].copy())]
    rel = [synth.gt_transform([0.4, -0.1, 0.02], [0.02, -0.01, 0.3]), np.eye(4)]
    xo, lo = oracle_apd.submap_assemble(frames, rel, 0.3)
    assert 0 < xo.shape[0] <= m and (m < 4095 or xo.shape[0] < m)  # the voxel grid ran: it merged points
    g = gorio.ApdGicp()
    assert g.setInputTargetSubmap(frames, rel, voxel_leaf=0.3) == xo.shape[0]
    xg, lg = g.getTargetPoints()
    assert np.array_equal(xg, xo) and np.array_equal(lg, lo)


@pytest.mark.parametrize("n", [4096, 4097])
def test_voxelmap_sort_sizes(gpu, gorio, oracle_apd, n):
    _, _, tx, tl, _ = gs.c1_pair(64, n)
    ct = oracle_apd.calculate_covariances(tx, oracle_apd.launch_params())
    g = gorio.ApdGicp()
    g.set_method(apd.METHOD_VGICP, 1.0)
    g.setInputTarget(tx, tl)
    g.setTargetCovariances(ct)
    check_map(g.getVoxelMap(), gr.VoxelMap(tx, ct, 1.0))


def test_replaced_points_leave_nothing_stale(gpu, gorio):
    kw = dict(corr_dist_threshold=2.0, transformation_epsilon=0.05, keep_knn_indices=1, search=1)
    hip = C.CDLL("libamdhip64.so")  # the runtime the library itself is linked against
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a, np.float32)
        ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(ptr), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(ptr, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice
        bufs.append(ptr)
        return ptr.value

    def cols(sx, sl):
        return [dev(sx[:, 0]), dev(sx[:, 1]), dev(sx[:, 2]), dev(sl)]

    def result(h):
        r = h.align()
        r["corr"], r["sqd"] = h.getCorrespondences()
        return r

    sx, sl, tx, tl, _ = synth.scan_pair(600, 600, seed=930)
    g = gorio.ApdGicp(**kw)
    g.setInputTarget(tx, tl)
    g.setInputSource(sx, sl)
    g.calculateCovariances()
    setters = {
        "setInputSource": lambda x, l: g.setInputSource(x, l),
        "device": lambda x, l: g.setInputSourceDevice(*cols(x, l), len(x)),
        "batch": lambda x, l: gorio.DeviceInputs([g], sources=[(cols(x, l), len(x))]).apply(),
    }
    for q, (name, replace) in enumerate(setters.items()):
        assert g.getKnnIndices(0).shape == (600, g.params.k_correspondences)  # lists of the current covariances are held
        nx, nl = synth.radar_scan(600, seed=931 + q)  # as many points as before: no size check can tell the clouds apart
        replace(nx, nl)
        with pytest.raises(gorio.GorioError) as e:
            g.getKnnIndices(0)
        assert e.value.code == -3, name  # GORIO_ERR_STATE
        fresh = gorio.ApdGicp(**kw)
        fresh.setInputTarget(tx, tl)
        fresh.setInputSource(nx, nl)
        got, ref = result(g), result(fresh)
        assert got["n_linearize"] >= 2, name
        for key in ref:
            assert np.array_equal(got[key], ref[key]), (name, key)
    for ptr in bufs:
        hip.hipFree(ptr)
