"""GPU tests of the spatial index (Morton sort, kd_refine_kernel, the three box levels) and of the three search families built on it
-- knn_kth_kernel + knn_collect_kernel with the knn_pruned_kernel fallback, nn_search_pruned_kernel with nn_plan_kernel, and the
brute-force kernels -- at the sizes and geometries where an index goes wrong.  EVERY comparison here is against the CPU oracle
(oracle.apd: the exhaustive scan up to 40 000 points, its kd-tree variant above; tests/test_index_scenes.py pins the two to each other
and to the NumPy restatement on these scenes).  Indices and squared distances must be bit-exact, ties on the lowest index.

  a  size sweep: n - 1 / n / n + 1 around the tile (32), the wave (64), the super tile and padding (512), the kd chunk (2048), the sort
     tile and big kd chunk (4096), the block (32 768) and the small / big switch (131 072), single cloud, pruned and brute force:
     k-NN lists, covariances, and the 1-NN of a moved ragged copy with the gate at 2 m and off.
  b  every queries-per-wave value of the selection kernels: at the sizes that select it, in two batches (16 clouds: renumbered onto
     XCDs; 14 clouds: not), and forced through GORIO_KNN_QPW on a tie scene and a control.
  c  the scenes of index_scenes.py at 16 384 and 40 000 points, as a cloud and as the target of its copy moved by half a unit; the
     1 000 000-point map and two dense blobs of 1 000 000 points, pruned only (the slow test of this module).
  d  seeded and planned searches: 8 fixed Gauss-Newton iterations on hard geometry, then the correspondences at the final pose.

Every test prints what it covered.  Every 1-NN test asserts a floor on the ORACLE's accepted correspondences (the GPU's equal them
bit for bit), so a gate that rejects everything cannot pass silently.

Wall time on one MI355X, same visit, each module as its own pytest run: this module 13.2 s (92 tests; pytest reports 11.95 s, most
of it scene generation and the oracle on the host; the two 1 000 000-point cases take 2.5 s and 1.4 s), tests/test_c5_gpu.py 3.6 s
(pytest: 2.36 s).  At 3.7 times the C5 module nothing was trimmed.
"""
import ctypes
import importlib

import numpy as np
import pytest

import index_scenes as scenes

synth = importlib.import_module("go-rio_amd.synth")
pytestmark = pytest.mark.gpu

KD_ABOVE = 40000  # the exhaustive oracle up to here, its kd-tree variant above
COV_ATOL = 1e-9  # the gate of test_apd_gpu.py::test_knn_other_k
# PLANE regularisation rebuilds the covariance from its eigenvectors, whose error grows with 1 / (relative gap of the eigenvalues):
# test_apd_gpu.py::test_covariances_match_oracle allows 1e-13 / gap, which meets COV_ATOL for gap >= 1e-4.  Points below that are
# locally rank-deficient (an outlier whose 19 neighbours are one far-away blob, three collinear returns) and are compared by their
# lists only; every scene that is not rank-deficient as a whole must keep at least this share of its points in the comparison.
COV_MIN_GAP = 1e-4
COV_MIN_SHARE = 0.9
GATE = 2.0  # corr_dist_threshold of the launch files; None = the class default FLT_MAX (gate off)


def _pose():  # the pose of test_apd_gpu.py
    T = np.eye(4)
    T[:3, :3] = synth.rpy_to_matrix([0.1, -0.1, 1.0])
    T[:3, 3] = [0.2, -0.05, 0.01]
    return T


def oracle_knn(oracle_apd, xyz):
    return oracle_apd.knn_self(xyz, scenes.K, kdtree=len(xyz) > KD_ABOVE)


def oracle_nn(oracle_apd, T, src, tgt, gate):
    kw = {} if gate is None else dict(corr_dist_threshold=gate)
    p = oracle_apd.default_params(search=1 if len(tgt) > KD_ABOVE else 0, **kw)
    corr, sqd, _ = oracle_apd.update_correspondences(T, src, tgt, np.zeros((len(src), 4, 4)), np.zeros((len(tgt), 4, 4)), p)
    return corr, sqd


def same_nn(got, want):
    """correspondences (the -1 rejections included) and the squared distances of the accepted ones, bit for bit (the pruned search
    does not look for the distance of a rejected point)"""
    (corr, sqd), (corr_o, sqd_o) = got, want
    return np.array_equal(corr, corr_o) and np.array_equal(sqd[corr_o >= 0], sqd_o[corr_o >= 0])


def first_difference(a, b):
    bad = np.flatnonzero((np.asarray(a) != np.asarray(b)).reshape(len(a), -1).any(axis=1))
    return f"{len(bad)} rows differ, first {bad[0]}: got {np.asarray(a)[bad[0]]} want {np.asarray(b)[bad[0]]}" if len(bad) else "equal"


def tie_share(oracle_apd, xyz):
    """share of the queries with more than TIE_BUFFER points within their k-th distance: those leave the selection kernels for the
    insertion kernel"""
    wide = oracle_apd.knn_self(xyz, 32, kdtree=True)[1] if len(xyz) >= 32 else None
    return float("nan") if wide is None else float((scenes.within_kth(wide) > scenes.TIE_BUFFER).mean())


def check_cloud(gorio, oracle_apd, name, xyz, searches=(1, 0), tag="", qpw=None):
    """k-NN lists of one cloud on its own (one covariance call over one cloud: the queries per wave follow from its size alone) against
    the oracle; covariances where the scene has well-defined ones."""
    idx_o, _ = oracle_knn(oracle_apd, xyz)
    deficient = name in scenes.RANK_DEFICIENT
    reg = oracle_apd.REG_NONE if deficient else oracle_apd.REG_PLANE
    for search in searches:
        g = gorio.ApdGicp(keep_knn_indices=1, search=search, regularization=reg)
        g.setInputSource(xyz, None)
        g.calculateCovariances()
        idx = g.getKnnIndices(0)
        assert np.array_equal(idx, idx_o), (name, len(xyz), search, first_difference(idx, idx_o))
        if not deficient:
            cov_o = oracle_apd.covariances_from_knn(xyz, idx_o, reg)
            w = np.linalg.eigvalsh(oracle_apd.covariances_from_knn(xyz, idx_o, oracle_apd.REG_NONE)[:, :3, :3])
            ok = np.minimum(w[:, 1] - w[:, 0], w[:, 2] - w[:, 1]) >= COV_MIN_GAP * np.maximum(w[:, 2], 1e-300)
            assert ok.mean() >= COV_MIN_SHARE, (name, len(xyz), ok.mean())
            err = np.abs(g.getSourceCovariances() - cov_o).reshape(len(xyz), -1).max(axis=1)
            assert np.all(err[ok] <= COV_ATOL), (name, len(xyz), search, float(err[ok].max()))
    print(f"[{tag}] k-NN {name} n={len(xyz)} qpw={qpw or scenes.natural_qpw([len(xyz)])} searches={searches} tie share={tie_share(oracle_apd, xyz):.3f}"
          + ("" if deficient else f" covariances compared on {ok.mean():.3f} of the points"))
    return idx_o


def check_pair(gorio, oracle_apd, name, src, tgt, T, gates=(GATE, None), searches=(1, 0), floor=0.5, inject=True, tag=""):
    """1-NN of src (moved by T) in tgt against the oracle, for every gate and search.  floor: the share of the source the ORACLE must
    accept at the 2 m gate (with the gate off it accepts everything)."""
    eye_s, eye_t = np.tile(np.eye(4), (len(src), 1, 1)), np.tile(np.eye(4), (len(tgt), 1, 1))
    for gate in gates:
        want = oracle_nn(oracle_apd, T, src, tgt, gate)
        accepted = int((want[0] >= 0).sum())
        assert accepted >= (floor * len(src) if gate is not None else len(src)), (name, gate, accepted, len(src))
        for search in searches:
            kw = {} if gate is None else dict(corr_dist_threshold=gate)
            g = gorio.ApdGicp(keep_knn_indices=1, search=search, regularization=oracle_apd.REG_NONE if name in scenes.RANK_DEFICIENT else oracle_apd.REG_PLANE, **kw)
            g.setInputTarget(tgt, None)
            g.setInputSource(src, None)
            if inject:  # only the searches run
                g.setSourceCovariances(eye_s)
                g.setTargetCovariances(eye_t)
            g.linearize(T)
            got = g.getCorrespondences()
            assert same_nn(got, want), (name, len(src), len(tgt), gate, search, first_difference(got[0], want[0]))
            if not inject:  # the covariance call of the pair covered both clouds: the target's lists once more, under that call's grid
                assert np.array_equal(g.getKnnIndices(1), oracle_knn(oracle_apd, tgt)[0]), (name, len(tgt), search)
        print(f"[{tag}] 1-NN {name} {len(src)} x {len(tgt)} gate={gate} searches={searches} accepted={accepted}")


# ------------------------------------------------------------------------------------------------------------------ a: size sweep

SWEEP = (20, 31, 32, 33, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 32767, 32768, 32769, 131071, 131072, 131073)
SWEEP_CASES = [("radar", n) for n in SWEEP] + [(s, n) for s in ("lattice3d", "cluster_outliers") for n in SWEEP if n <= 4097]


@pytest.mark.parametrize("name,n", SWEEP_CASES)
def test_a_size_sweep(gpu, gorio, oracle_apd, name, n):
    """One cloud of n points: k-NN lists (and covariances) pruned and brute force; then the same cloud as the target of a ragged part of
    itself (n - 37 points, at least 20) moved by _pose(), gate 2 m and off.  At the 131 07x sizes identity covariances are injected
    for the 1-NN part so that only the searches run; below, the pair's own covariance call checks the target's lists a second time."""
    xyz = scenes.make(name, n)
    check_cloud(gorio, oracle_apd, name, xyz, tag="a")
    src = np.ascontiguousarray(xyz[: max(n - 37, 20)])
    # radar returns reach 120 m, where _pose() (1 degree of yaw, 0.2 m) moves a point by 2.3 m: at least half of every scan lies within
    # the 100 m where the move stays below the gate; the lattices (side <= 17) and the 1 cm cluster move by less than 1 m altogether
    check_pair(gorio, oracle_apd, name, src, xyz, _pose(), inject=n > 100000, tag="a")


# --------------------------------------------------------------------------------------------------------- b: queries per wave

@pytest.mark.parametrize("name,n,qpw", [("radar", 2300, 8), ("radar", 16384, 16), ("radar", 40000, 32), ("radar", 70000, 64), ("lattice3d_dup", 70000, 64)])
def test_b_natural_qpw(gpu, gorio, oracle_apd, name, n, qpw):
    """the sizes at which run_covariances picks 8 / 16 / 32 / 64 queries per wave by itself (pruned: the selection kernels)"""
    assert scenes.natural_qpw([n]) == qpw
    check_cloud(gorio, oracle_apd, name, scenes.make(name, n, seed=2), searches=(1,), tag=f"b natural {qpw}")


@pytest.mark.parametrize("pairs", [8, 7])
def test_b_batches(gpu, gorio, oracle_apd, pairs):
    """A batch of 8 pairs of about 3 000 points is one covariance call over 16 clouds, whose workgroups are renumbered so that a cloud
    runs on one XCD (xcd_grid_pos, apd_device.h); 7 pairs (14 clouds) keep the plain numbering.  Ragged sizes, a tie scene among them:
    every cloud's lists against the oracle."""
    clouds = []
    for q in range(pairs):
        name = "lattice3d_dup" if q % 4 == 1 else "radar"
        clouds.append((scenes.make(name, 2800 + 211 * q, seed=10 + q), scenes.make(name, 3300 - 173 * q, seed=30 + q)))
    objs = []
    for sx, tx in clouds:
        g = gorio.ApdGicp(keep_knn_indices=1, search=1, regularization=oracle_apd.REG_NONE, corr_dist_threshold=GATE, max_iterations=1)
        g.setInputTarget(tx, None)
        g.setInputSource(sx, None)
        objs.append(g)
    gorio.align_batch(objs)
    for q, (g, (sx, tx)) in enumerate(zip(objs, clouds)):
        for which, xyz in ((0, sx), (1, tx)):
            idx_o, _ = oracle_knn(oracle_apd, xyz)
            idx = g.getKnnIndices(which)
            assert np.array_equal(idx, idx_o), (q, which, first_difference(idx, idx_o))
            cov = g.getSourceCovariances() if which == 0 else g.getTargetCovariances()
            assert np.allclose(cov, oracle_apd.covariances_from_knn(xyz, idx_o, oracle_apd.REG_NONE), rtol=0, atol=COV_ATOL)
    sizes = [len(c) for pr in clouds for c in pr]
    print(f"[b batch] {2 * pairs} clouds of {min(sizes)} .. {max(sizes)} points, qpw={scenes.natural_qpw(sizes)}, XCD renumbering={'yes' if 2 * pairs >= 16 and 2 * pairs % 8 == 0 else 'no'}")


@pytest.mark.parametrize("qpw", [8, 16, 32, 64])
@pytest.mark.parametrize("name", ["lattice3d_dup", "radar"])
def test_b_forced_qpw(gpu, gorio, oracle_apd, monkeypatch, name, qpw):
    """Every queries-per-wave value forced on one small cloud through GORIO_KNN_QPW (read by run_covariances at every call).  On the tie
    scene more than half of the queries overflow the selection buffer, so every wave raises its redo flag: with 8 queries per wave
    eight waves share one flag (the case of test_apd_gpu.py::test_knn_select_kernel_falls_back_on_massive_ties), with 64 each wave has
    its own.  The lists must not depend on the value."""
    monkeypatch.setenv("GORIO_KNN_QPW", str(qpw))
    libc = ctypes.CDLL(None)
    libc.getenv.restype = ctypes.c_char_p
    assert libc.getenv(b"GORIO_KNN_QPW") == str(qpw).encode()  # the C environment the library reads, not only os.environ
    xyz = scenes.make(name, 2300, seed=3)
    if name in scenes.KNN_TIE_SCENES:
        assert tie_share(oracle_apd, xyz) > 0.5
    check_cloud(gorio, oracle_apd, name, xyz, searches=(1,), tag="b forced", qpw=qpw)


# ------------------------------------------------------------------------------------------------------ c: hard geometry at scale

@pytest.mark.parametrize("n", [16384, 40000])
@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_c_scene(gpu, gorio, oracle_apd, name, n):
    """every scene as a cloud (k-NN lists) and as the target of its copy moved by half a unit (1-NN; a move of 0.87 m: the 2 m gate
    accepts every point, which the floor asserts), pruned and brute force"""
    xyz = scenes.make(name, n)
    check_cloud(gorio, oracle_apd, name, xyz, tag="c")
    check_pair(gorio, oracle_apd, name, scenes.shifted(xyz), xyz, np.eye(4), floor=1.0, tag="c")


@pytest.mark.parametrize("name", ["radar", "two_clusters"])
def test_c_million_points_slow(gpu, gorio, oracle_apd, name):
    """THE SLOW TEST of this module: 1 000 000 points, pruned only -- the k-NN lists of the big map (kd_refine_kernel<4096>, 64 queries
    per wave, 31 blocks of 32 768 points) against the kd-tree oracle, and the 1-NN of a 16 384-point scan in it.  `radar` is the C5 map of
    tests/test_c5_gpu.py (61 accumulated radar scans), whose k-NN lists no other test looks at."""
    n = 1_000_000
    tgt = synth.local_map(n, seed=synth.BASE_SEED + 77, n_scans=n // 16384)[0] if name == "radar" else scenes.make(name, n)
    src = np.ascontiguousarray(tgt[:16384] if name == "radar" else scenes.shifted(tgt[:16384]))
    T = _pose() if name == "radar" else np.eye(4)
    idx_o, _ = oracle_knn(oracle_apd, tgt)
    g = gorio.ApdGicp(keep_knn_indices=1, search=1, corr_dist_threshold=GATE)
    g.setInputTarget(tgt, None)
    g.setInputSource(src, None)
    g.calculateCovariances()
    idx = g.getKnnIndices(1)
    assert np.array_equal(idx, idx_o), (name, first_difference(idx, idx_o))
    assert np.array_equal(g.getKnnIndices(0), oracle_knn(oracle_apd, src)[0])
    for gate in (GATE, None):
        g.set_params(corr_dist_threshold=GATE if gate is not None else float(np.finfo(np.float32).max))
        g.linearize(T)
        want = oracle_nn(oracle_apd, T, src, tgt, gate)
        accepted = int((want[0] >= 0).sum())
        assert accepted >= (len(src) // 2 if gate is not None else len(src))  # the scan is part of the map, moved by less than the gate within 100 m
        got = g.getCorrespondences()
        assert same_nn(got, want), (name, gate, first_difference(got[0], want[0]))
        print(f"[c slow] 1-NN {name} {len(src)} x {n} gate={gate} accepted={accepted}")
    print(f"[c slow] k-NN {name} n={n} qpw={scenes.natural_qpw([n, len(src)])} tie share={tie_share(oracle_apd, tgt):.3f}")


# -------------------------------------------------------------------------------------- d: seeded and planned searches in an align

@pytest.mark.parametrize("name,n_src,n_tgt", [("lattice3d_dup", 16384, 40000), ("lattice3d", 16384, 40000), ("cluster_outliers", 16384, 40000),
                                              ("two_clusters", 16384, 40000), ("lattice3d_dup", 16384, 140000)])
def test_d_align_searches(gpu, gorio, oracle_apd, name, n_src, n_tgt):
    """Eight fixed Gauss-Newton iterations (optimizer 0, zero epsilons, as test_apd_gpu.py::
    test_seeded_and_planned_searches_keep_ties_on_the_lowest_index): the unseeded search, the seeded one and the planned ones all run
    on hard geometry; 16 384 x 140 000 crosses the `big` switch of the plan budget and the splits.  What is new is the ORACLE at the
    final pose; the run without the plan and the brute-force run (poses, H and counters bit-equal) only localise a failure."""
    tgt = scenes.make(name, n_tgt)
    # the source is part of the target, half a unit off: its last points by index and its far corner, where the Morton order and the
    # last tile end -- on the lattices the final pose lays every source point back on its original, so a target point the index lost
    # or a tie that went to a duplicate shows in the correspondences
    far = np.argsort(tgt.astype(np.float64).sum(axis=1), kind="stable")[-(n_src // 2) :]
    src = scenes.shifted(tgt[np.unique(np.concatenate([far, np.arange(n_tgt - n_src // 2, n_tgt)]))])
    kw = dict(corr_dist_threshold=GATE, max_iterations=8, optimizer=0, rotation_epsilon=0.0, transformation_epsilon=0.0)
    res = {}
    for key, search, plan in (("planned", 1, True), ("unplanned", 1, False), ("brute", 0, True)):
        g = gorio.ApdGicp(search=search, **kw)
        g.setInputTarget(tgt, None)
        g.setInputSource(src, None)
        g.debugSetSchedule(plan_search=plan)
        r = g.align()
        g.linearize(r["T"].astype(np.float64))
        res[key] = (r, g.getCorrespondences())
    r0, got = res["planned"]
    assert r0["n_linearize"] == 8 and np.isfinite(r0["T"]).all()
    want = oracle_nn(oracle_apd, r0["T"].astype(np.float64), src, tgt, GATE)
    accepted = int((want[0] >= 0).sum())
    print(f"[d] {name} {len(src)} x {n_tgt}: accepted={accepted} at the final pose, translation {np.linalg.norm(r0['T'][:3, 3]):.3f} m")
    # the source starts 0.87 m from its own originals, inside the gate, and Gauss-Newton only pulls it closer
    assert accepted >= len(src) // 2
    assert same_nn(got, want), (name, first_difference(got[0], want[0]))
    for key in ("unplanned", "brute"):
        r, c = res[key]
        assert np.array_equal(r["T"], r0["T"]) and np.array_equal(r["H"], r0["H"]), key
        assert (r["n_linearize"], r["nr_iterations"], r["converged"]) == (r0["n_linearize"], r0["nr_iterations"], r0["converged"]), key
        assert same_nn(c, want), (name, key, first_difference(c[0], want[0]))
