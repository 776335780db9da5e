"""GPU tests of the list work of the K = 20 selection path (knn_kth_kernel's tiered insertion, knn_collect_kernel's comparator network,
the listed redo pass knn_redo_kernel): every k-NN list and covariance must be, bit for bit, what the brute-force path (search=0) gives on
the same cloud, and must meet the CPU oracle under the gates of the existing k-NN tests (lists bit-exact, covariances to 1e-9;
test_apd_gpu.py::test_knn_other_k, test_index_boundaries_gpu.py).

Sizes 1, 19, 20, 21, 63, 64, 65, 255, 256, 257, 5000 on uniform random points, a planar cloud, a cloud in which every point appears
twice and a cloud of identical points.  A cloud with fewer points than k_correspondences is refused (GORIO_ERR_INVALID: undefined in the
reference), which is asserted; n = 1 and 19 then run with k = n, the largest the library takes, through the same K = 20 kernels -- their
20th distance is +inf, the padding of the search index lies at or below it, and the wave is redone: the redo pass is expected there.
(Before this test existed the tile walk of such a wave also took tiles past the end of the index: wrong neighbours or an illegal
access; the walks now stop at n_tiles.)  From n = 20 on a random cloud has no ties and the redo pass must do no group
(gorio_apd_debug_knn_redo_groups).

The redo path is forced by a 3-d integer lattice (27 points within the 20th distance d^2 = 3 of an interior point, more than the 24 the
buffer holds) at n = 257 and 5000.  The boundary of the buffer is hit exactly: a query with 19 distinct nearer points and 5 (24 keys:
stays in the sort) or 6 (25 keys: flagged) points at exactly its 20th distance.  Stale marks: a lattice and then a random cloud on one
handle.  One batched call over clouds of 64, 257 and 5000 points against the single calls.

Covariances against the oracle: PLANE regularisation rebuilds the matrix from eigenvectors, whose error grows with 1 / (relative
eigenvalue gap); as in test_index_boundaries_gpu.py points with a gap below 1e-4 are compared by their lists only, and the degenerate
clouds (planar, doubled, identical, lattice, fewer than 20 points) use regularisation NONE, where every point is compared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 20
CAP = K + 4  # keys knn_collect_kernel buffers per query
COV_ATOL = 1e-9  # the gate of test_apd_gpu.py::test_knn_other_k
COV_MIN_GAP = 1e-4  # test_index_boundaries_gpu.py
SIZES = (1, 19, 20, 21, 63, 64, 65, 255, 256, 257, 5000)
KINDS = ("uniform", "planar", "doubled", "identical")


def cloud(kind, n, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + KINDS.index(kind) if kind in KINDS else seed)
    if kind == "uniform":
        xyz = rng.uniform(-10.0, 10.0, (n, 3))
    elif kind == "planar":
        xyz = np.concatenate([rng.uniform(-10.0, 10.0, (n, 2)), np.full((n, 1), 0.5)], axis=1)
    elif kind == "doubled":
        half = rng.uniform(-10.0, 10.0, ((n + 1) // 2, 3))
        xyz = np.concatenate([half, half])[:n]
    elif kind == "identical":
        xyz = np.tile([1.5, -2.25, 0.75], (n, 1))
    elif kind == "lattice":
        side = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
        xyz = g[rng.permutation(n)]
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(xyz, dtype=np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run(gorio, xyz, search, k, reg, handle=None):
    g = handle or gorio.ApdGicp(keep_knn_indices=1, search=search, regularization=reg, k_correspondences=k)
    g.setInputSource(xyz, None)
    g.calculateCovariances()
    return g, g.getKnnIndices(0), g.getSourceCovariances()


_ORACLE = {}


def oracle_of(oracle_apd, key, xyz, k, reg):
    """the oracle's lists and covariances of a cloud, computed once per module"""
    if key not in _ORACLE:
        idx, _ = oracle_apd.knn_self(xyz, k)
        cov = oracle_apd.calculate_covariances(xyz, oracle_apd.launch_params(k_correspondences=k, regularization=reg))
        raw = cov if reg == oracle_apd.REG_NONE else oracle_apd.covariances_from_knn(xyz, idx, oracle_apd.REG_NONE)
        _ORACLE[key] = (idx, cov, raw)
    return _ORACLE[key]


def check(gorio, oracle_apd, key, xyz, reg, want_redo=None):
    """pruned against brute force as raw bits, both against the oracle; returns the redo groups of the pruned call"""
    n = len(xyz)
    k = min(K, n)
    gp, idx_p, cov_p = run(gorio, xyz, 1, k, reg)
    redo = gp.debugKnnRedoGroups()
    _, idx_b, cov_b = run(gorio, xyz, 0, k, reg)
    print(f"{key}: n={n} k={k} redo groups={redo}")
    assert np.array_equal(idx_p, idx_b), key
    assert np.array_equal(bits(cov_p), bits(cov_b)), key
    idx_o, cov_o, raw = oracle_of(oracle_apd, key, xyz, k, reg)
    assert np.array_equal(idx_p, idx_o), key
    err = np.abs(cov_p - cov_o).reshape(n, -1).max(axis=1)
    if reg == oracle_apd.REG_NONE:
        ok = np.ones(n, bool)
    else:
        w = np.linalg.eigvalsh(raw[:, :3, :3])
        ok = np.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1]) >= COV_MIN_GAP * np.maximum(w[:, 2], 1e-300)
        assert ok.mean() >= 0.9, (key, ok.mean())
    assert np.all(err[ok] <= COV_ATOL), (key, float(err[ok].max()))
    if want_redo is not None:
        assert want_redo(redo), (key, redo)
    return redo


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_and_geometries(gpu, gorio, oracle_apd, kind, n):
    xyz = cloud(kind, n)
    reg = oracle_apd.REG_PLANE if kind == "uniform" and n >= K else oracle_apd.REG_NONE
    want = None
    if kind == "uniform":
        want = (lambda r: r == 0) if n >= K else (lambda r: r == 1)  # no ties: nothing to redo; below K the 20th distance is +inf (docstring)
    elif kind == "identical" and n > CAP:
        want = lambda r: r == (n + 63) // 64  # every query has all n points at its 20th distance 0: every group is redone
    check(gorio, oracle_apd, (kind, n), xyz, reg, want)


@pytest.mark.parametrize("n", [1, 19])
def test_fewer_points_than_k_is_refused(gpu, gorio, n):
    g = gorio.ApdGicp(keep_knn_indices=1, search=1, k_correspondences=K)
    g.setInputSource(cloud("uniform", n), None)
    with pytest.raises(gorio.GorioError):
        g.calculateCovariances()


@pytest.mark.parametrize("n", [257, 5000])
def test_lattice_forces_the_redo_pass(gpu, gorio, oracle_apd, n):
    xyz = cloud("lattice", n, seed=3)
    wide = oracle_apd.knn_self(xyz, 32)[1]
    over = (wide <= wide[:, K - 1 : K]).sum(axis=1) > CAP  # queries with more than CAP points within their 20th distance
    assert over.any()
    check(gorio, oracle_apd, ("lattice", n), xyz, oracle_apd.REG_NONE, lambda r: 1 <= r <= (n + 63) // 64)


def boundary_cloud(ties):
    """query 0 at the origin, 18 points at distinct distances below 0.3, `ties` points at distance exactly 1 (the 20th distance), and 250
    far random points: 1 + 18 + ties keys at or below the origin's 20th distance, and no other query has a tie"""
    rng = np.random.default_rng(5)
    near = rng.normal(size=(18, 3))
    near *= (np.linspace(0.05, 0.3, 18) / np.linalg.norm(near, axis=1))[:, None]
    unit = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], float)[:ties]
    far = rng.uniform(50.0, 60.0, (250, 3))
    return np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), near, unit, far]), dtype=np.float32)


@pytest.mark.parametrize("ties,flagged", [(5, 0), (6, 1)])
def test_boundary_of_the_buffer(gpu, gorio, oracle_apd, ties, flagged):
    xyz = boundary_cloud(ties)
    wide = oracle_apd.knn_self(xyz, 32)[1]
    within = (wide <= wide[:, K - 1 : K]).sum(axis=1)
    assert within[0] == 19 + ties and within.max() == 19 + ties and (within[1:] == K).all()  # 24 or 25 keys for the origin, 20 elsewhere
    check(gorio, oracle_apd, ("boundary", ties), xyz, oracle_apd.REG_NONE, lambda r: r == flagged)


@pytest.mark.parametrize("n", [257, 5000])
def test_marks_of_an_earlier_cloud_do_not_leak(gpu, gorio, oracle_apd, n):
    """a lattice (every group marked) and then a random cloud on ONE handle: the second result is a fresh handle's, and nothing is redone"""
    reg = oracle_apd.REG_PLANE
    g, _, _ = run(gorio, cloud("lattice", 5000, seed=3), 1, K, reg)
    assert g.debugKnnRedoGroups() >= 1
    xyz = cloud("uniform", n, seed=9)
    _, idx, cov = run(gorio, xyz, 1, K, reg, handle=g)
    assert g.debugKnnRedoGroups() == 0
    _, idx_f, cov_f = run(gorio, xyz, 1, K, reg)
    assert np.array_equal(idx, idx_f) and np.array_equal(bits(cov), bits(cov_f))
    assert np.array_equal(idx, oracle_apd.knn_self(xyz, K)[0])


def test_batched_call_equals_the_single_calls(gpu, gorio, oracle_apd):
    """one covariance call over clouds of 64, 257 and 5000 points (align_batch estimates every cloud of its pairs in one call); the 5000-point
    cloud is a lattice, so the call lists groups of a job other than the first"""
    reg = oracle_apd.REG_NONE
    tgt_a = cloud("uniform", 257, seed=11)
    src_a = np.ascontiguousarray(tgt_a[:64])
    lat = cloud("lattice", 5000, seed=3)
    objs = []
    for sx, tx in ((src_a, tgt_a), (lat, lat)):
        g = gorio.ApdGicp(keep_knn_indices=1, search=1, regularization=reg, corr_dist_threshold=2.0, max_iterations=1)
        g.setInputTarget(tx, None)
        g.setInputSource(sx, None)
        objs.append(g)
    gorio.align_batch(objs)
    assert objs[0].debugKnnRedoGroups() >= 2  # both lattice clouds
    for g, (sx, tx) in zip(objs, ((src_a, tgt_a), (lat, lat))):
        for which, xyz in ((0, sx), (1, tx)):
            _, idx_s, cov_s = run(gorio, xyz, 1, K, reg)
            cov = g.getSourceCovariances() if which == 0 else g.getTargetCovariances()
            assert np.array_equal(g.getKnnIndices(which), idx_s), (len(xyz), which)
            assert np.array_equal(bits(cov), bits(cov_s)), (len(xyz), which)
