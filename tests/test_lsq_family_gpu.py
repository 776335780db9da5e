"""One handle walked through every registration method of gorio_apd_set_method and back, against fresh handles.

The five Gauss-Newton / LM methods (APD-GICP, FastGICP, FastVGICP, NDTCuda, FastVGICPCuda) share one host pipeline and one
method-switch transition; the other three (ICP, GICP_OMP, FastGICPMultiPoints) leave state of their own on the handle.  Whatever a
method left behind must not reach the next one: after every step the walked handle returns what a fresh handle, set to that method
from the start, returns for the same calls -- T, H, b and the errors bit for bit, the counters equal.

GICP_OMP is not part of the walk: it estimates covariances by a rule of its own (GO:50-122) but registers with whatever covariances the
clouds already hold, so a handle that reaches it from another method aligns with that method's covariances and differs from a fresh one
(255 points: nr_iterations 4 and n_linearize 229 against 5 and 277).  That is how the library behaves today; this test pins the rest.
"""
import importlib

import numpy as np
import pytest

import gicp_scenes as gs
import ndt_cuda_restatement as nr

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu

GUESS = nr.known_transform(0.02, -0.01, 0, 0.004, 0)
GN, LM = 0, 1


def _ndt_cuda(g):
    g.set_ndt_cuda_params(apd.NDT_CUDA_D2D)
    g.set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT7)


def _vgicp_cuda(g):
    g.set_vgicp_cuda_params(apd.NN_CPU_PARALLEL_KDTREE)
    g.set_method(apd.METHOD_VGICP_CUDA, 1.0, apd.VOXEL_DIRECT7)


# (name, how a handle is set to the method, member of the Gauss-Newton / LM family)
WALK = [
    ("apd", lambda g: g.set_method(apd.METHOD_APDGICP), True),
    ("ndt_cuda", _ndt_cuda, True),
    ("vgicp_cuda", _vgicp_cuda, True),
    ("vgicp", lambda g: g.set_method(apd.METHOD_VGICP, 1.0, apd.VOXEL_DIRECT7, apd.VOXEL_ADDITIVE), True),
    ("gicp", lambda g: g.set_method(apd.METHOD_GICP), True),
    ("icp", lambda g: g.set_method(apd.METHOD_ICP), False),
    ("gicp_mp", lambda g: g.set_method(apd.METHOD_GICP_MP), False),
    ("apd_again", lambda g: g.set_method(apd.METHOD_APDGICP), True),
]


def _handle(gorio, src, tgt):
    g = gorio.ApdGicp()
    g.setInputTarget(tgt)
    g.setInputSource(src)
    return g


def _align(g, optimizer):
    g.set_params(optimizer=optimizer)
    r = g.align(GUESS)
    return r["T"].tobytes(), r["H"].tobytes(), r["converged"], r["nr_iterations"], r["n_linearize"]


def _steps(g, lsq):
    """The calls of one method, as (step name, comparable result) in call order."""
    if not lsq:
        yield "align", _align(g, GN)
        return
    err, H, b = g.linearize(gs.parity_pose())
    yield "linearize", (np.float64(err).tobytes(), H.tobytes(), b.tobytes())
    yield "compute_error", np.float64(g.compute_error(nr.known_transform())).tobytes()
    yield "align GN", _align(g, GN)
    yield "align LM", _align(g, LM)


@pytest.fixture(scope="module")
def scene():
    src, tgt, _ = nr.scene_pair(4096)
    return src, tgt


@pytest.mark.parametrize("n", [255, 256, 257, 1500])  # one block of partials, its boundary on both sides, several blocks
def test_walked_handle_equals_fresh_handles(gpu, gorio, scene, n):
    src, tgt = scene
    src = np.ascontiguousarray(src[np.random.default_rng(n).permutation(src.shape[0])[:n]])
    walked = _handle(gorio, src, tgt)
    for name, configure, lsq in WALK:
        configure(walked)
        fresh = _handle(gorio, src, tgt)
        configure(fresh)
        for (step, got), (_, want) in zip(_steps(walked, lsq), _steps(fresh, lsq)):
            assert got == want, "%s, %s: the walked handle differs from a fresh one" % (name, step)
