"""GPU tests of the k-NN and radius queries of include/gorio_search.h.  Every comparison is EXACT equality -- indices, float bits of
the squared distances, counts, offsets -- with the NumPy restatement tests/search_restatement.py, which test_search_restatement.py
pins against the oracle on the CPU.

Cloud sizes are the ones at which the index changes shape (tile = 32 points, group = 64 tiles, kd chunk = 2048 points); query counts
straddle the 64-lane wave; k covers the list's ends and k > n.  Scenes: uniform, a lattice with multiplicities (massive ties), all
points identical, collinear.  Queries: the cloud's own points (NULL form and explicit), jittered points, points 10^3 box diameters
outside, tile-box corners, and a NaN and an Inf query inside an otherwise finite wave."""
import ctypes as C

import numpy as np
import pytest

import index_scenes as S
import search_restatement as R

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 31, 32, 33, 2047, 2048, 2049, 4097]
NQS = [1, 63, 64, 65, 257]
KS = [1, 5, 20, 32]


# ------------------------------------------------------------------------------------------------ scenes and queries
def uniform(n, seed):
    return np.random.default_rng(seed).uniform(-20.0, 20.0, (n, 3)).astype(np.float32)


def lattice_mult(n, seed):
    """integer lattice points, each present about three times: every distance is shared by many pairs and by exact duplicates"""
    rng = np.random.default_rng(seed)
    m = max(1, n // 3)
    side = 1
    while side ** 3 < m:
        side += 1
    i = np.arange(n) % m
    pts = np.stack([i % side, (i // side) % side, i // (side * side)], axis=1).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(n)])


def identical(n, seed):
    return np.tile(np.array([[1.5, -2.25, 0.75]], np.float32), (n, 1))


SCENES = dict(uniform=uniform, lattice=lattice_mult, identical=identical, collinear=S.line)


def jittered(xyz, nq, seed, sigma=0.3):
    rng = np.random.default_rng(seed)
    return (xyz[rng.integers(0, len(xyz), nq)] + rng.normal(0.0, sigma, (nq, 3))).astype(np.float32)


def far_outside(xyz, nq, seed):
    """10^3 box diameters away from the cloud, in random directions"""
    rng = np.random.default_rng(seed)
    diam = max(float(np.linalg.norm(xyz.max(axis=0) - xyz.min(axis=0))), 1.0)
    v = rng.normal(0.0, 1.0, (nq, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (xyz.mean(axis=0) + 1.0e3 * diam * v).astype(np.float32)


def with_nonfinite(q):
    """one NaN and one Inf query inside an otherwise finite wave (positions 3 and 40 of the first 64 when there are that many)"""
    q = q.copy()
    q[min(3, len(q) - 1), 1] = np.nan
    if len(q) > 1:
        q[min(40, len(q) - 2), 0] = np.inf
    return q


def cut(ref32, k):
    """the k-NN result for k from the one for 32: the first k columns, counts capped (the same order, a prefix of it)"""
    idx, sqd, cnt = ref32
    return idx[:, :k], sqd[:, :k], np.minimum(cnt, k)


def same(got, want):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.nonzero(np.atleast_1d(g != w).reshape(len(g), -1).any(axis=1))[0] if g.size else []
        assert len(bad) == 0, f"{len(bad)} rows differ, first {bad[:5]}"


def same_csr(s, counts, total, want):
    offs_w, idx_w, sqd_w = want
    assert total == int(offs_w[-1]) and np.array_equal(counts, np.diff(offs_w))
    offs, idx, sqd = s.radius_get(total)
    assert np.array_equal(offs, offs_w) and np.array_equal(idx, idx_w) and np.array_equal(sqd.view(np.uint32), sqd_w.view(np.uint32))


class Hip:
    """device arrays through the HIP runtime the library links against"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.ptrs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        self.ptrs.append(p)
        return p.value

    def dev(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            assert self.hip.hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1) == 0
        return p

    def host(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipDeviceSynchronize() == 0  # the library's stream does not synchronise with the null stream
        if out.nbytes:
            assert self.hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(p), C.c_size_t(out.nbytes), 2) == 0
        return out

    def free(self):
        assert self.hip.hipDeviceSynchronize() == 0
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.fixture()
def hip():
    h = Hip()
    yield h
    h.free()


# ------------------------------------------------------------------------------------------------ k-NN
@pytest.mark.parametrize("n", SIZES)
def test_knn_at_cloud_sizes(gpu, gorio, n):
    xyz = uniform(n, 10 + n)
    s = gorio.Search()
    s.set_cloud(xyz)
    assert s.cloud_size() == n
    base = xyz if n else np.zeros((1, 3), np.float32)
    for nq in NQS:
        q = with_nonfinite(jittered(base, nq, 100 + nq, sigma=1.0)) if nq >= 63 else jittered(base, nq, 100 + nq, sigma=1.0)
        ref = R.knn(xyz, q, 32)
        for k in KS:
            same(s.knn(q, k), cut(ref, k))
    ref = R.knn(xyz, None, 32)  # the cloud's own points: NULL form and explicit form
    for k in (1, 5, 32):
        same(s.knn(None, k), cut(ref, k))
        same(s.knn(xyz.copy(), k), cut(ref, k))
    if n:
        assert (s.knn(None, 1)[1] == 0).all()  # a point is its own first neighbour (or a lower-index duplicate is)
    s.close()


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_knn_scenes_and_query_kinds(gpu, gorio, scene):
    n, nq = 2049, 257
    xyz = SCENES[scene](n, 7)
    reg = gorio.ApdGicp(search=1)
    reg.setInputTarget(xyz, np.zeros(n, np.float32))
    s = gorio.Search()
    s.set_cloud_from_apd(reg, 1)  # the owner's index: its tile boxes give the corner queries
    tb = reg.debugGetIndex(1)["tbox"]
    tb = tb[np.isfinite(tb).all(axis=1)]
    corners = np.concatenate([tb[:, 0:3], tb[:, 4:7], np.stack([tb[:, 0], tb[:, 5], tb[:, 2]], axis=1)]).astype(np.float32)
    kinds = dict(own=xyz[:nq].copy(), jitter=with_nonfinite(jittered(xyz, nq, 3)), far=far_outside(xyz, 65, 4), corners=corners[:nq],
                 mixed=with_nonfinite(np.concatenate([far_outside(xyz, 20, 5), jittered(xyz, 100, 6), corners[:9]])))
    for name, q in kinds.items():
        ref = R.knn(xyz, q, 32)
        for k in (1, 20, 32):
            same(s.knn(q, k), cut(ref, k))
    ref = R.knn(xyz, None, 32)
    for k in (1, 20, 32):
        same(s.knn(None, k), cut(ref, k))
    s.close()


def test_knn_device_form_equals_host_form(gpu, gorio, hip):
    n, nq, k = 4097, 257, 20
    xyz = lattice_mult(n, 3)
    q = with_nonfinite(jittered(xyz, nq, 8))
    s = gorio.Search()
    s.set_cloud_device(hip.dev(xyz[:, 0].copy()), hip.dev(xyz[:, 1].copy()), hip.dev(xyz[:, 2].copy()), n)
    assert s.counters() == dict(point_uploads=0, index_builds=1, result_downloads=0)
    want = s.knn(q, k)
    same(want, R.knn(xyz, q, k))
    d_idx, d_sqd, d_cnt = hip.alloc(4 * nq * k), hip.alloc(4 * nq * k), hip.alloc(4 * nq)
    before = s.counters()["result_downloads"]
    q5 = np.zeros((nq, 5), np.float32)  # a strided query array: 20 bytes between queries
    q5[:, :3] = q
    s.knn_device(hip.dev(q5), nq, 20, k, d_idx, d_sqd, d_cnt)
    same((hip.host(d_idx, (nq, k), np.int32), hip.host(d_sqd, (nq, k), np.float32), hip.host(d_cnt, (nq,), np.int32)), want)
    assert s.counters()["result_downloads"] == before
    d_idx, d_sqd = hip.alloc(4 * n * k), hip.alloc(4 * n * k)  # self queries, no counts asked for
    s.knn_device(None, n, 12, k, d_idx, d_sqd, None)
    same((hip.host(d_idx, (n, k), np.int32), hip.host(d_sqd, (n, k), np.float32)), R.knn(xyz, None, k)[:2])
    cnt, total = s.radius(q, 1.5)
    cnt_d, total_d = s.radius_device(hip.dev(q5), nq, 20, 1.5)
    assert total == total_d and np.array_equal(cnt, cnt_d)
    same_csr(s, cnt_d, total_d, R.radius(xyz, q, 1.5))
    s.close()


# ------------------------------------------------------------------------------------------------ radius
@pytest.mark.parametrize("n", SIZES)
def test_radius_at_cloud_sizes(gpu, gorio, n):
    xyz = uniform(n, 20 + n)
    s = gorio.Search()
    s.set_cloud(xyz)
    base = xyz if n else np.zeros((1, 3), np.float32)
    for nq in (1, 65, 257):
        q = with_nonfinite(jittered(base, nq, 200 + nq, sigma=1.0)) if nq > 1 else jittered(base, nq, 200 + nq, sigma=1.0)
        for r, max_nn in ((1.0e-3, 0), (3.4, 0), (3.4, 1), (3.4, 7)):  # nothing; about 10 neighbours at n = 4097; the same, cut
            cnt, total = s.radius(q, r, max_nn)
            same_csr(s, cnt, total, R.radius(xyz, q, r, max_nn))
    cnt, total = s.radius(None, 3.4, 7)  # the cloud's own points
    same_csr(s, cnt, total, R.radius(xyz, None, 3.4, 7))
    s.close()


@pytest.mark.parametrize("scene", ["lattice", "identical", "collinear"])
def test_radius_tie_scenes(gpu, gorio, scene):
    n = 2049
    xyz = SCENES[scene](n, 9)
    s = gorio.Search()
    s.set_cloud(xyz)
    q = with_nonfinite(np.concatenate([jittered(xyz, 150, 1, sigma=0.05), xyz[:60], far_outside(xyz, 5, 2)]))
    for r, max_nn in ((1.0, 0), (1.5, 7), (2.0, 0)):  # on the lattice d = 1 and d = 4 are distances of many pairs: the strict rule decides
        cnt, total = s.radius(q, r, max_nn)
        same_csr(s, cnt, total, R.radius(xyz, q, r, max_nn))
    s.close()


def test_radius_whole_cloud_takes_the_long_path(gpu, gorio):
    """3 queries that catch all 9000 points: every segment exceeds what the LDS sort takes (4096 keys)."""
    n = 9000
    xyz = lattice_mult(n, 5)
    s = gorio.Search()
    s.set_cloud(xyz)
    q = np.array([[3.2, 4.1, 5.3], [0.0, 0.0, 0.0], [7.0, 7.0, 7.5]], np.float32)
    for max_nn in (0, 7, 5000):
        cnt, total = s.radius(q, 1.0e3, max_nn)
        assert total == (3 * n if max_nn == 0 else 3 * max_nn)
        same_csr(s, cnt, total, R.radius(xyz, q, 1.0e3, max_nn))
    # capacity: one entry short is refused and nothing is written; the result is still there afterwards
    cnt, total = s.radius(q, 1.0e3, 0)
    offs = np.full(4, -1, np.int64)
    idx = np.full(total, -5, np.int32)
    sqd = np.full(total, -5.0, np.float32)
    rc = s.lib.gorio_search_radius_get(s.h, C.c_void_p(offs.ctypes.data), C.c_void_p(idx.ctypes.data), C.c_void_p(sqd.ctypes.data), C.c_longlong(total - 1))
    assert rc == -1 and (offs == -1).all() and (idx == -5).all() and (sqd == -5.0).all()
    same_csr(s, cnt, total, R.radius(xyz, q, 1.0e3, 0))
    s.close()


def test_radius_long_and_short_segments_in_one_call(gpu, gorio):
    """Two blobs of 5000 and 9000 points and a sparse background: one call holds long segments of two slot sizes (8192 and 16384 keys
    for the tiled sort), segments the LDS sort takes, and empty ones."""
    rng = np.random.default_rng(11)
    blob_a = rng.normal(0.0, 0.2, (5000, 3)) + np.array([5.0, 5.0, 0.0])
    blob_b = rng.normal(0.0, 0.2, (9000, 3)) + np.array([-40.0, 30.0, 2.0])
    xyz = np.concatenate([blob_a, blob_b, rng.uniform(-60.0, 60.0, (3000, 3))]).astype(np.float32)
    xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))])
    near_a = (blob_a[:20] + rng.normal(0.0, 0.3, (20, 3))).astype(np.float32)
    near_b = (blob_b[:20] + rng.normal(0.0, 0.3, (20, 3))).astype(np.float32)
    q = with_nonfinite(np.concatenate([near_a, rng.uniform(-60.0, 60.0, (60, 3)).astype(np.float32), near_b]))
    s = gorio.Search()
    s.set_cloud(xyz)
    want = R.radius(xyz, q, 3.0)
    lens = np.diff(want[0])
    assert ((lens > 4096) & (lens <= 8192)).any() and (lens > 8192).any() and ((lens > 0) & (lens <= 4096)).any() and (lens == 0).any()
    cnt, total = s.radius(q, 3.0)
    same_csr(s, cnt, total, want)
    cnt, total = s.radius(q, 3.0, 7)
    want7 = R.radius(xyz, q, 3.0, 7)
    same_csr(s, cnt, total, want7)
    # a refused call and a new cloud leave the result held as it was: it stays until the next radius call
    with pytest.raises(gorio.GorioError):
        s.radius(q, -1.0)
    s.set_cloud(xyz[:100])
    offs, idx, sqd = s.radius_get(total)
    assert np.array_equal(offs, want7[0]) and np.array_equal(idx, want7[1]) and np.array_equal(sqd.view(np.uint32), want7[2].view(np.uint32))
    s.close()


# ------------------------------------------------------------------------------------------------ the cloud: refusals, sharing
def test_nonfinite_cloud_is_refused_and_the_held_cloud_stays(gpu, gorio, hip):
    xyz = uniform(500, 1)
    q = jittered(xyz, 65, 2)
    s = gorio.Search()
    s.set_cloud(xyz)
    want = R.knn(xyz, q, 5)
    bad = uniform(300, 2)
    bad[77, 2] = np.nan
    with pytest.raises(gorio.GorioError) as e:
        s.set_cloud(bad)
    assert e.value.code == -1 and "not finite" in str(e.value)
    same(s.knn(q, 5), want)
    bad[77, 2] = np.inf
    with pytest.raises(gorio.GorioError) as e:
        s.set_cloud_device(hip.dev(bad[:, 0].copy()), hip.dev(bad[:, 1].copy()), hip.dev(bad[:, 2].copy()), 300)
    assert e.value.code == -1
    assert s.cloud_size() == 500
    same(s.knn(q, 5), want)
    idx = np.zeros((10, 5), np.int32)  # NULL queries stand for the cloud: nq must be its size
    assert s.lib.gorio_search_knn(s.h, None, 10, 12, 5, C.c_void_p(idx.ctypes.data), C.c_void_p(idx.ctypes.data), None) == -1
    s.close()


def test_shared_from_registration(gpu, gorio):
    sx, sl, tx, tl, _ = gorio.synth.scan_pair(2048, 2048, seed=5)
    q = with_nonfinite(jittered(tx, 257, 3))
    par = dict(search=1, corr_dist_threshold=2.0, transformation_epsilon=0.1)
    alone = gorio.ApdGicp(**par)
    alone.setInputTarget(tx, tl)
    alone.setInputSource(sx, sl)
    ra = alone.align()
    owner = gorio.ApdGicp(**par)
    owner.setInputTarget(tx, tl)
    owner.setInputSource(sx, sl)
    s = gorio.Search()
    s.set_cloud_from_apd(owner, 1)  # before the owner's first align: the index is built now, through the owner
    assert s.cloud_size() == len(tx)
    up = gorio.Search()
    up.set_cloud(tx)
    assert up.counters() == dict(point_uploads=1, index_builds=1, result_downloads=0)
    same(s.knn(q, 20), up.knn(q, 20))
    same(s.knn(q, 20), R.knn(tx, q, 20))
    cnt, total = s.radius(q, 1.0, 7)
    same_csr(s, cnt, total, R.radius(tx, q, 1.0, 7))
    c = s.counters()
    assert (c["point_uploads"], c["index_builds"]) == (0, 0)
    assert owner.debugGetIndex(1)["n"] == len(tx)  # the owner finds its index built
    ro = owner.align()  # bit for bit what it is without the sharer
    assert np.array_equal(ro["T"].view(np.uint32), ra["T"].view(np.uint32)) and ro["n_linearize"] == ra["n_linearize"]
    # the owner moves on: the search handle keeps the old cloud
    owner.setInputTarget(sx, sl)
    same(s.knn(q, 20), R.knn(tx, q, 20))
    # the sharer moves on: the owner's cloud is untouched
    s2 = gorio.Search()
    s2.set_cloud_from_apd(owner, 0)
    s2.set_cloud(tx[:100])
    same(s2.knn(q, 5), R.knn(tx[:100], q, 5))
    sh = gorio.Search()
    sh.set_cloud_from_apd(owner, 0)
    same(sh.knn(q, 5), R.knn(sx, q, 5))
    # the owner dies: the sharer keeps working
    del owner
    same(s.knn(q, 20), R.knn(tx, q, 20))
    same(sh.knn(None, 3), R.knn(sx, None, 3))
    empty = gorio.ApdGicp()
    with pytest.raises(gorio.GorioError) as e:
        s.set_cloud_from_apd(empty, 0)  # no such cloud: GORIO_ERR_STATE, and the cloud held stays
    assert e.value.code == -3
    same(s.knn(q, 20), R.knn(tx, q, 20))
    for h in (s, s2, sh, up):
        h.close()


def test_shared_from_keyframe(gpu, gorio):
    xyz = uniform(3000, 4)
    q = jittered(xyz, 130, 5)
    store = gorio.KeyframeStore()
    kid = store.add(xyz)
    k0 = store.add(np.zeros((0, 3), np.float32))
    assert store.info(kid)["index_built"] == 0
    s = gorio.Search()
    s.set_cloud_from_keyframe(store, kid)
    assert store.info(kid)["index_built"] == 1  # built through the store: its next consumer finds it
    assert store.counters()["point_uploads"] == 2
    same(s.knn(q, 20), R.knn(xyz, q, 20))
    cnt, total = s.radius(q, 3.0)
    same_csr(s, cnt, total, R.radius(xyz, q, 3.0))
    c = s.counters()
    assert (c["point_uploads"], c["index_builds"]) == (0, 0)
    store.release(kid)  # the store lets go: the sharer keeps the cloud
    same(s.knn(q, 20), R.knn(xyz, q, 20))
    e = gorio.Search()
    e.set_cloud_from_keyframe(store, k0)  # an empty keyframe is the empty cloud
    assert e.cloud_size() == 0 and (e.knn(q, 3)[2] == 0).all()
    with pytest.raises(gorio.GorioError):
        e.set_cloud_from_keyframe(store, kid)  # released
    store.close()
    same(s.knn(None, 5), R.knn(xyz, None, 5))
    s.close()
    e.close()
