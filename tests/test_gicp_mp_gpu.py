"""fast_gicp::FastGICPMultiPoints on the GPU (GORIO_METHOD_GICP_MP) against tests/gicp_mp_restatement.py: covariances, the neighbour CSR (bit-exact),
one pass, aligns, lifecycle and hand-offs.

Tolerances.  The CSR is compared for equality and the pose by the project's 1e-4 m / 1e-4 rad gate.  For the float covariances and the
one-pass quantities the yardstick is the restatement itself: SPREAD[q] is the largest deviation between its float32 form and its float64
twin over all cases (gicp_mp_scenes.measured_spreads, relative to the quantity's largest magnitude), measured on the CPU and recorded here
rounded up (tests/test_gicp_mp_restatement.py keeps the record honest); the GPU may differ from the float32 form by at most FACTOR times
that -- legal float evaluation orders of the same formulas, such as the eigen-solver standing in for the SVD, give deviations of that
size and not more."""
import importlib

import numpy as np
import pytest

import gicp_mp_restatement as R
import gicp_mp_scenes as M
import icp_scenes as S
import search_restatement as sr

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu
INVALID, STATE, UNSUPPORTED = -1, -3, -5
SPREAD = dict(cov=5.8e-7, mean_B=4.8e-8, cov_B=1.4e-7, H=7.3e-7, g=1.6e-6)  # measured: 5.71e-7, 4.76e-8, 1.35e-7, 7.20e-7, 1.58e-6
FACTOR = 4.0


def within(got, want, q):
    dev = M.rel(got, want)
    print("%s: deviation %.3g of the scale, bound %.3g" % (q, dev, FACTOR * SPREAD[q]))
    return dev <= FACTOR * SPREAD[q]


def new(gorio, p=None, **over):
    p = dict(R.DEFAULTS if p is None else p)
    p.update(over)
    g = gorio.ApdGicp()
    g.set_params(k_correspondences=p["k_correspondences"], regularization=p["regularization"], max_iterations=p["max_iterations"], rotation_epsilon=p["rotation_epsilon"],
                 transformation_epsilon=p["transformation_epsilon"])
    g.set_gicp_mp_params(p["neighbor_search_radius"])
    g.set_method(apd.METHOD_GICP_MP)
    return g


def loaded(gorio, name):
    sc = M.scenes()[name]
    g = new(gorio, M.params_of(name))
    g.setInputTarget(sc["target"])
    g.setInputSource(sc["source"])
    return g, sc


# ------------------------------------------------------------------------------------------------ covariances

@pytest.mark.parametrize("cloud", list(M.cov_clouds()))
def test_covariances_of_both_clouds_and_all_rules(gorio, gpu, cloud):
    pts = M.cov_clouds()[cloud]
    other = M.cov_clouds()["room_256"]
    for which in (0, 1):
        g = new(gorio)
        g.setInputSource(pts if which == 0 else other)
        g.setInputTarget(pts if which == 1 else other)
        for reg in (R.MIN_EIG, R.NORMALIZED_MIN_EIG, R.PLANE, R.FROBENIUS):
            g.set_params(regularization=reg)
            got = g.gicp_mp_covariances(which)
            assert got.shape == (pts.shape[0], 6) and within(got, R.covariances(pts, 20, reg), "cov"), (which, reg)


def test_covariance_refusals(gorio, gpu):
    g = new(gorio)
    g.setInputSource(S.room(19, 5))
    g.setInputTarget(S.room(40, 6))
    with pytest.raises(apd.GorioError) as e:
        g.gicp_mp_covariances(0)
    assert e.value.code == INVALID  # n = 19 < k
    assert g.gicp_mp_covariances(1).shape == (40, 6)
    with pytest.raises(apd.GorioError) as e:
        g.align()
    assert e.value.code == INVALID
    g.setInputSource(S.room(20, 5))
    g.set_params(regularization=R.NONE)
    for call in (lambda: g.gicp_mp_covariances(1), g.align, g.gicp_mp_pass):
        with pytest.raises(apd.GorioError) as e:
            call()
        assert e.value.code == UNSUPPORTED


# ------------------------------------------------------------------------------------------------ the neighbour CSR

def csr_equal(g, tgt, q, radius):
    offs, idx, sqd = g.gicp_mp_neighbors()
    eo, ei, es = sr.radius(tgt, q, radius)
    return np.array_equal(offs, eo) and np.array_equal(idx, ei) and idx.dtype == np.int32 and sqd.tobytes() == es.tobytes()


@pytest.mark.parametrize("m", [300, 2000])
@pytest.mark.parametrize("radius", [0.5, 0.25])
def test_csr_is_bit_exact(gorio, gpu, m, radius):
    tgt = S.target(m)
    g = new(gorio, k_correspondences=1, neighbor_search_radius=radius)  # k = 1: a source of one point is a legal cloud
    g.setInputTarget(tgt)
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        src = S.source(n, m)
        g.setInputSource(src)
        r = g.gicp_mp_pass(M.G1)
        q = R.transform_points_f32(M.G1, src)
        eo = sr.radius(tgt, q, radius)[0]
        assert csr_equal(g, tgt, q, radius), n
        assert r["total"] == eo[-1] and r["used"] == int((np.diff(eo) > 0).sum())


def test_csr_with_empty_segments_inside_a_block(gorio, gpu):
    g, sc = loaded(gorio, "far_points_257")
    r = g.gicp_mp_pass(sc["guess"])
    assert csr_equal(g, sc["target"], R.transform_points_f32(sc["guess"], sc["source"]), 0.5)
    offs = g.gicp_mp_neighbors()[0]
    lens = np.diff(offs)
    assert (lens[100:120] == 0).all() and (lens[:100] > 0).all() and (lens[120:] > 0).all() and r["used"] == 257
    assert not g.gicp_mp_merged()["used"][100:120].any()
    for drop in (lambda: g.setInputSource(sc["source"]), lambda: g.set_gicp_mp_params(0.4), g.swapSourceAndTarget):  # the pass dies with what it was made from
        g.gicp_mp_pass(sc["guess"])
        g.gicp_mp_neighbors()
        drop()
        for hook in (g.gicp_mp_neighbors, g.gicp_mp_merged):
            with pytest.raises(apd.GorioError) as e:
                hook()
            assert e.value.code == STATE


def test_neighbour_at_exactly_the_bound_is_excluded(gorio, gpu):
    tgt = S.target(300)
    f = np.float32
    # a target point whose x + 0.5 is exact in float32: the query at that spot is at squared distance exactly 0.25 = float(0.5 * 0.5)
    # ... and which still has other target points within the radius
    def spot(i):
        return (tgt[i] + np.array([0.5, 0.0, 0.0], f)).astype(f)

    j = next(i for i in range(300) if f(f(tgt[i, 0] + f(0.5)) - tgt[i, 0]) == f(0.5) and sr.radius(tgt, spot(i)[None], 0.5)[0][1] >= 3)
    src = S.source(65, 300).copy()
    src[33] = spot(j)
    assert sr.sqdist(src[33:34], tgt[j:j + 1])[0, 0] == sr.radius_bound(0.5)
    g = new(gorio)
    g.setInputTarget(tgt)
    g.setInputSource(src)
    g.gicp_mp_pass(np.eye(4, dtype=f))  # trans of the identity moves no bit
    assert csr_equal(g, tgt, src, 0.5)
    offs, idx, _ = g.gicp_mp_neighbors()
    seg = idx[offs[33]:offs[34]]
    assert seg.size > 0 and j not in seg


# ------------------------------------------------------------------------------------------------ one pass

@pytest.mark.parametrize("name", [c[0] for c in M.pass_cases()])
def test_one_pass(gorio, gpu, name):
    g, sc = loaded(gorio, name)
    p = M.params_of(name)
    r = g.gicp_mp_pass(sc["guess"])
    P = M.pass_reference(name)
    assert csr_equal(g, sc["target"], P.q, p["neighbor_search_radius"])
    assert r["used"] == P.n_used and r["total"] == P.offsets[-1]
    mg = g.gicp_mp_merged()
    assert np.array_equal(mg["used"], P.used)
    if P.n_used == 0:
        assert not r["H"].any() and not r["g"].any()
        return
    assert within(mg["mean_B"], P.mean_B, "mean_B") and within(mg["cov_B"], P.cov_B, "cov_B")
    assert within(r["H"], P.H, "H") and within(r["g"], P.g, "g")
    assert np.array_equal(r["H"], r["H"].T)


# ------------------------------------------------------------------------------------------------ aligns

@pytest.mark.parametrize("name", M.ALIGN_SCENES)
def test_align(gorio, gpu, name):
    g, sc = loaded(gorio, name)
    ref = M.reference(name)
    a = g.align(sc["guess"])
    assert a["converged"] == ref["converged"] and a["nr_iterations"] == ref["iterations"] and a["n_linearize"] == ref["passes"]
    dt, dr = S.pose_error(a["T"], ref["T"])
    print("pose deviation %.3g m %.3g rad" % (dt, dr))
    assert dt < 1e-4 and dr < 1e-4
    assert within(a["H"], ref["H"], "H")
    b = g.align(sc["guess"])
    assert a["T"].tobytes() == b["T"].tobytes() and a["H"].tobytes() == b["H"].tobytes() and b["nr_iterations"] == a["nr_iterations"]
    d = g.gicp_mp_diag()
    assert d["passes"] == ref["passes"] and d["used"] == ref["used"][-1]
    score, inl = g.getFitnessScore(a["T"])  # the scores and transform_source work on the clouds, not on the method
    assert np.isfinite(score) and 0.0 <= inl <= 1.0
    assert np.array_equal(g.transformSource(a["T"]), R.transform_points_f32(a["T"], sc["source"]))


def test_all_empty_ends_unconverged_at_the_guess(gorio, gpu):
    g, sc = loaded(gorio, "all_empty")
    ref = M.reference("all_empty")
    a = g.align(sc["guess"])
    assert not a["converged"] and a["nr_iterations"] == 0 and a["n_linearize"] == 1
    assert a["T"].tobytes() == ref["T"].tobytes() and not a["H"].any()
    assert g.gicp_mp_diag()["used"] == 0 and g.gicp_mp_neighbors()[1].size == 0


# ------------------------------------------------------------------------------------------------ nothing else changed

def test_switching_back_returns_a_fresh_handles_bits_and_batches_refuse(gorio, gpu):
    src, tgt = S.source(257, 2000), S.target(2000)

    def fresh():
        o = gorio.ApdGicp()
        o.setInputTarget(tgt)
        o.setInputSource(src)
        return o

    a = fresh()
    ra = a.align(M.G1)
    b = fresh()
    b.set_method(apd.METHOD_GICP_MP)
    rb = b.align(M.G1)
    assert rb["T"].tobytes() != ra["T"].tobytes()  # another algorithm
    corr_a = a.getCorrespondences()
    nb = b.gicp_mp_neighbors()
    for objs in ([a, b], [b, a], [b]):
        with pytest.raises(apd.GorioError) as e:
            apd.align_batch(objs, np.stack([M.G1] * len(objs)))
        assert e.value.code == UNSUPPORTED
    for call in (apd.icp_align_batch, apd.gicp_omp_align_batch):
        with pytest.raises(apd.GorioError) as e:
            call([b], np.stack([M.G1]))
        assert e.value.code == STATE
    assert all(np.array_equal(x, y) for x, y in zip(corr_a, a.getCorrespondences()))
    assert all(np.array_equal(x, y) for x, y in zip(nb, b.gicp_mp_neighbors()))
    b.set_method(apd.METHOD_APDGICP)
    with pytest.raises(apd.GorioError) as e:
        b.gicp_mp_neighbors()  # the switch dropped the pass
    assert e.value.code == STATE
    rc = b.align(M.G1)
    assert rc["T"].tobytes() == ra["T"].tobytes() and rc["H"].tobytes() == ra["H"].tobytes() and rc["nr_iterations"] == ra["nr_iterations"]


# ------------------------------------------------------------------------------------------------ hand-offs

def test_shared_target_and_keyframe_source_give_the_same_bits(gorio, gpu):
    kf = importlib.import_module("go-rio_amd.keyframes")
    g, sc = loaded(gorio, "guess_256_300")
    want = g.align(sc["guess"])
    store = kf.KeyframeStore()
    kid = store.add(sc["source"])
    before = store.counters()
    o = new(gorio, M.params_of("guess_256_300"))
    o.setInputTargetShared(g)
    o.setInputSourceKeyframe(store, kid)
    got = o.align(sc["guess"])
    assert got["T"].tobytes() == want["T"].tobytes() and got["H"].tobytes() == want["H"].tobytes() and got["nr_iterations"] == want["nr_iterations"]
    assert store.counters() == before and before["point_uploads"] == 1  # no extra point upload
    assert np.array_equal(o.gicp_mp_covariances(1), g.gicp_mp_covariances(1))
    # the covariance rule is one more "regularization" for a shared cloud: a sharer with another rule or k is refused
    p = new(gorio, M.params_of("guess_256_300"), regularization=R.FROBENIUS)
    with pytest.raises(apd.GorioError) as e:
        p.setInputTargetShared(g)
    assert e.value.code == INVALID
    o.set_params(k_correspondences=10)
    with pytest.raises(apd.GorioError) as e:
        o.align(sc["guess"])
    assert e.value.code == INVALID
    store.close()
