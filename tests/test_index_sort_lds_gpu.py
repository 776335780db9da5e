"""The search index when the Morton keys of a cloud are made and sorted by one workgroup inside LDS (bbox_morton_sort_kernel, clouds of at
most LDS_SORT_MAX points) and when a call mixes such clouds with bigger ones, which keep the tiled sort through global memory.

The index is read back through gorio_apd_debug_get_index and compared with the NumPy restatement of tests/test_index_build_structure.py
(imported, not copied): the whole permutation, tie-break included, and every tile, super-tile and block box must be EQUAL.  The sorted keys
are unique -- (Morton code << 31) | point index -- so the LDS sort has exactly one right answer, whatever the geometry does to the codes:

  uniform     random positions in a box
  planar      z constant
  identical   every point the same (one Morton code; the sort is decided by the index bits alone)
  pairs       every point occurs exactly twice
  collide     64 cells of the Morton grid hold all the points, which differ inside a cell (equal codes, different positions)

Sizes: around the tile (32), the kd chunk (2048), the sort tile of the old path (4096), the limit of the LDS sort and the limit + 1, which
takes the old path (with its 64-point source on the new one: already a mixed call); one batched call with a limit-sized cloud, a limit + 1
cloud and a 33-point cloud.  For three sizes the 1-NN and the 20-NN results of the pruned searches equal the brute-force ones bit for bit.
"""
import importlib

import numpy as np
import pytest

import test_index_build_structure as ibs

synth = importlib.import_module("go-rio_amd.synth")
LDS_SORT_MAX = 16384  # kLdsSortMax (apd_index.hip)
SIZES = (1, 31, 32, 33, 2047, 2048, 2049, 4097, LDS_SORT_MAX, LDS_SORT_MAX + 1)
GEOMETRIES = ("planar", "identical", "pairs", "collide")
CASES = [("uniform", n) for n in SIZES] + [(kind, n) for kind in GEOMETRIES for n in (33, 4097, LDS_SORT_MAX)]
SEARCH_SIZES = (33, 4097, LDS_SORT_MAX)


def make(kind, n, seed=11):
    rng = np.random.default_rng(seed + 7 * n)
    xyz = rng.uniform(-40.0, 40.0, (n, 3)).astype(np.float32) * np.array([1.0, 0.6, 0.1], np.float32)
    if kind == "planar":
        xyz[:, 2] = np.float32(1.25)
    elif kind == "identical":
        xyz[:] = xyz[0]
    elif kind == "pairs":
        half = (n + 1) // 2
        xyz[half:] = xyz[: n - half]
        xyz = xyz[rng.permutation(n)]
    elif kind == "collide":
        # the box is 80 m wide -> cells of 80 / 2047 m; 64 cell corners, every point within a quarter of a cell of one of them
        cell = np.float32(80.0 / 2047.0)
        corners = (rng.integers(8, 2040, (64, 3)).astype(np.float32) + np.float32(0.25)) * cell - np.float32(40.0)
        xyz = corners[rng.integers(0, 64, n)] + rng.uniform(0.0, 0.25, (n, 3)).astype(np.float32) * cell
        if n >= 2:  # two points pin the bounding box, and with it the cell size
            xyz[0], xyz[1] = np.float32(-40.0), np.float32(40.0)
    return np.ascontiguousarray(xyz, np.float32)


def check_index(ix, xyz, chunk=2048):
    """permutation and boxes of an index read back against the restatement"""
    n = len(xyz)
    n_spad = -(-n // 512) * 512
    assert (ix["n"], ix["n_spad"], ix["kd_chunk"]) == (n, n_spad, chunk)
    orig_r, _, _ = ibs.restate(xyz, chunk)
    orig = ix["orig"]
    assert np.array_equal(orig, orig_r), (n, int((orig != orig_r).sum()))
    want_pts = np.full((n_spad, 3), np.float32(1e30), np.float32)
    want_pts[:n] = xyz[orig[:n]]
    for a, name in enumerate(("sx", "sy", "sz")):
        assert np.array_equal(ix[name], want_pts[:, a]), name
    assert np.array_equal(ix["s4"][:, :3], want_pts) and np.array_equal(ix["s4"][:, 3].view(np.int32), orig)
    for name, group in (("tbox", 32), ("sbox", 512), ("bbox", 32768)):
        assert ix[name].shape == (-(-n_spad // group), 8), name
        assert np.array_equal(ix[name], ibs.boxes_of(ix, group)), name


def test_collide_input_collides():
    """the restatement alone (no GPU): the `collide` input has many points per Morton code, the `identical` one a single code"""
    for kind, most in (("collide", 66), ("identical", 1)):
        xyz = make(kind, 4097)
        lo, hi = xyz.min(axis=0), xyz.max(axis=0)
        ext = np.float32(max(np.float32(1e-6), (hi - lo).max()))
        q = np.minimum(np.maximum((xyz - lo) / ext * np.float32(2047.0), np.float32(0.0)), np.float32(2047.0)).astype(np.uint32)
        cells = len(np.unique(q, axis=0))
        assert cells <= most, (kind, cells)
        assert len(np.unique(xyz, axis=0)) == (1 if kind == "identical" else len(xyz))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", CASES)
def test_index_of_one_cloud(gpu, gorio, kind, n):
    xyz = make(kind, n)
    src = np.ascontiguousarray(xyz[: min(n, 64)])
    g = gorio.ApdGicp(search=1)
    g.setInputTarget(xyz, None)
    g.setInputSource(src, None)
    g.setSourceCovariances(np.tile(np.eye(4), (len(src), 1, 1)))  # only the index build and one search run
    g.setTargetCovariances(np.tile(np.eye(4), (n, 1, 1)))
    g.linearize(np.eye(4))
    check_index(g.debugGetIndex(1), xyz)
    check_index(g.debugGetIndex(0), src)
    print(f"[lds sort] {kind} n={n}: target on the {'LDS' if n <= LDS_SORT_MAX else 'tiled'} sort, source ({len(src)}) on the LDS sort")


@pytest.mark.gpu
def test_mixed_batch(gpu, gorio):
    """one index call over a limit-sized cloud, a limit + 1 cloud and a 33-point cloud (and a second limit-sized one): each is routed by its
    own size, and each index is the restatement's"""
    clouds = [(make("uniform", 33, seed=3), make("uniform", LDS_SORT_MAX, seed=4)), (make("collide", LDS_SORT_MAX, seed=5), make("uniform", LDS_SORT_MAX + 1, seed=6))]
    objs = []
    for sx, tx in clouds:
        g = gorio.ApdGicp(search=1, max_iterations=1)
        g.setInputTarget(tx, None)
        g.setInputSource(sx, None)
        objs.append(g)
    gorio.align_batch(objs)
    for g, (sx, tx) in zip(objs, clouds):
        check_index(g.debugGetIndex(0), sx)
        check_index(g.debugGetIndex(1), tx)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SEARCH_SIZES)
def test_searches_equal_brute_force(gpu, gorio, n):
    """20-NN lists of the cloud and the 1-NN of a moved ragged part of it: pruned (through the index) against brute force (search=0), bit for bit"""
    xyz = make("uniform", n)
    src = np.ascontiguousarray(xyz[: max(n - 37, 20)])
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0.01, -0.01, 0.02])
    T[:3, 3] = [0.2, -0.05, 0.01]
    got = {}
    for search in (1, 0):
        g = gorio.ApdGicp(keep_knn_indices=1, search=search)
        g.setInputTarget(xyz, None)
        g.setInputSource(src, None)
        g.calculateCovariances()
        g.linearize(T)
        got[search] = (g.getKnnIndices(1), g.getKnnIndices(0)) + tuple(g.getCorrespondences())
    for a, b, what in zip(got[1], got[0], ("20-NN target", "20-NN source", "1-NN index", "1-NN squared distance")):
        assert np.array_equal(a, b), (n, what)
    assert (got[0][2] >= 0).sum() >= len(src) // 2  # the gate (class default: off) rejects nothing: a real comparison
