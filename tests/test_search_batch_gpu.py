"""GPU tests of gorio_search_radius_batch (include/gorio_search.h): several radius calls run by one set of launches.  Every comparison is
EXACT equality -- offsets, indices, float bits of the squared distances, counts, totals -- with two references: the NumPy restatement
tests/search_restatement.py, and a single gorio_search_radius call on a fresh handle.

Shapes.  Query counts 1, 63, 64, 65, 257 and 513 straddle the 64-lane wave, so that the jobs' waves meet at every alignment in the shared
launch; the clouds of 300 and 2 000 points are the ones of the FastGICPMultiPoints tests.  A long segment needs more than 4 096 neighbours
of one query: a 4 200-point ball."""
import importlib

import numpy as np
import pytest

import icp_scenes as S
import search_restatement as R
from test_search_gpu import jittered

apd = importlib.import_module("go-rio_amd.apd")
pytestmark = pytest.mark.gpu
INVALID = -1
NQS = [1, 63, 64, 65, 257, 513]


def ball(n, radius, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 1.0, (n, 3))
    v *= (radius * rng.uniform(0.0, 1.0, (n, 1)) ** (1.0 / 3.0)) / np.linalg.norm(v, axis=1, keepdims=True)
    return (v + np.array([3.0, -2.0, 1.0])).astype(np.float32)


def same_job(got, want, what):
    """got: (count, total, offsets, idx, sqd) of one job; want: (offsets, idx, sqd)"""
    cnt, total, offs, idx, sqd = got
    wo, wi, ws = want
    assert total == int(wo[-1]), what
    assert np.array_equal(cnt, np.diff(wo)) and np.array_equal(offs, wo), what
    assert idx.dtype == np.int32 and np.array_equal(idx, wi) and sqd.view(np.uint32).tobytes() == ws.view(np.uint32).tobytes(), what


def single(gorio, cloud, q, radius, max_nn):
    """the job as one gorio_search_radius call on a fresh handle: (offsets, idx, sqd)"""
    s = gorio.Search()
    s.set_cloud(cloud)
    _, total = s.radius(q, radius, max_nn)
    out = s.radius_get(total)
    s.close()
    return out


def make(gorio, cloud):
    s = gorio.Search()
    s.set_cloud(cloud)
    return s


def run_and_check(gorio, handles, clouds, queries, radii, max_nns):
    got = gorio.Search.radius_batch(handles, queries, radii, max_nns)
    assert len(got) == len(handles)
    for j, g in enumerate(got):
        same_job(g, R.radius(clouds[j], queries[j], radii[j], max_nns[j]), "job %d against the restatement" % j)
        same_job(g, single(gorio, clouds[j], queries[j], radii[j], max_nns[j]), "job %d against a single call" % j)
    return got


@pytest.fixture(scope="module")
def mixed():
    """(clouds, queries, radii, max_nns) of the mixed batch; jobs 10 and 11 are appended by the test (they need a registration handle)"""
    c300, c2000 = S.target(300), S.target(2000)
    clouds, queries, radii, max_nns = [], [], [], []
    for i, nq in enumerate(NQS):
        cloud = c300 if i % 2 == 0 else c2000
        clouds.append(cloud)
        queries.append(jittered(cloud, nq, 40 + i, sigma=0.1))
        radii.append(0.5 if i % 3 else 0.25)
        max_nns.append(5 if i in (1, 4) else 0)
    nan_q = jittered(c2000, 130, 50, sigma=0.1)
    nan_q[65, 1] = np.nan  # in the middle of the job's second wave
    clouds += [c300, c2000, np.zeros((0, 3), np.float32), c2000]
    queries += [None, np.zeros((0, 3), np.float32), jittered(c300, 65, 51), nan_q]
    radii += [0.25, 0.5, 0.5, 0.5]
    max_nns += [0, 0, 0, 3]
    return clouds, queries, radii, max_nns


def test_mixed_batch(gorio, gpu, mixed):
    clouds, queries, radii, max_nns = [list(x) for x in mixed]
    handles = [make(gorio, c) for c in clouds]
    # two more handles share the target of ONE registration handle
    reg = gorio.ApdGicp()
    reg.setInputTarget(S.target(2000))
    reg.setInputSource(S.source(64, 2000))
    for seed, r in ((60, 0.5), (61, 0.25)):
        s = gorio.Search()
        s.set_cloud_from_apd(reg, 1)
        handles.append(s)
        clouds.append(S.target(2000))
        queries.append(jittered(S.target(2000), 257, seed, sigma=0.1))
        radii.append(r)
        max_nns.append(0)
    first = run_and_check(gorio, handles, clouds, queries, radii, max_nns)
    assert first[6][1] > 0 and first[7][1] == 0 and first[8][1] == 0  # self queries found themselves; nq = 0; the empty cloud
    assert first[9][0][65] == 0 and first[9][0][64] > 0  # the NaN query has no neighbour, the one before it does
    # held results: every handle holds its own job
    for j, s in enumerate(handles):
        offs, idx, sqd = s.radius_get(first[j][1])
        assert np.array_equal(offs, first[j][2]) and np.array_equal(idx, first[j][3]) and sqd.tobytes() == first[j][4].tobytes()
    # a single call on one handle leaves the others' results as they were
    handles[3].radius(queries[0], 0.3)
    for j, s in enumerate(handles):
        if j != 3:
            assert np.array_equal(s.radius_get(first[j][1])[1], first[j][3])
    # repeatability: the same batch once more gives the same bits
    again = gorio.Search.radius_batch(handles, queries, radii, max_nns)
    for a, b in zip(first, again):
        assert a[1] == b[1] and all(x.tobytes() == y.tobytes() for x, y in zip(a[2:], b[2:]))


@pytest.mark.parametrize("n_long", [1, 2])
def test_long_segments(gorio, gpu, n_long):
    dense = [ball(4200, 0.1, 70 + i) for i in range(n_long)]
    centre = np.array([[3.0, -2.0, 1.0]] * 3, np.float32)
    c300 = S.target(300)
    clouds = [c300] + dense + [S.target(2000)]
    queries = [jittered(c300, 65, 80, sigma=0.1)] + [centre + np.float32(1e-3 * i) for i in range(n_long)] + [jittered(S.target(2000), 257, 81, sigma=0.1)]
    radii = [0.5] + [0.25] * n_long + [0.5]
    max_nns = [0] + [0, 4100][:n_long] + [0]
    handles = [make(gorio, c) for c in clouds]
    got = run_and_check(gorio, handles, clouds, queries, radii, max_nns)
    for j in range(1, 1 + n_long):
        assert (np.diff(R.radius(clouds[j], queries[j], radii[j])[0]) > 4096).all()  # every segment of the job is a long one
        assert got[j][1] == 3 * (4200 if max_nns[j] == 0 else max_nns[j])


def test_refusals_leave_every_result_held(gorio, gpu):
    c300 = S.target(300)
    a, b = make(gorio, c300), make(gorio, S.target(2000))
    qa, qb = jittered(c300, 65, 90, sigma=0.1), jittered(S.target(2000), 63, 91, sigma=0.1)
    held = gorio.Search.radius_batch([a, b], [qa, qb], 0.5)

    def unchanged():
        for s, h in zip((a, b), held):
            offs, idx, sqd = s.radius_get(h[1])
            assert np.array_equal(offs, h[2]) and np.array_equal(idx, h[3]) and sqd.tobytes() == h[4].tobytes()

    cases = [
        ([a, a], [qa, qa], [0.5, 0.5], [0, 0], "twice"),
        ([a, b], [qa, qb], [0.5, -1.0], [0, 0], "job 1"),
        ([a, b], [qa, qb], [float("nan"), 0.5], [0, 0], "job 0"),
        ([a, b], [qa, qb], [0.5, 0.5], [0, -2], "job 1"),
    ]
    for hs, qs, rs, ms, word in cases:
        with pytest.raises(apd.GorioError) as e:
            gorio.Search.radius_batch(hs, qs, rs, ms)
        assert e.value.code == INVALID and word in str(e.value), str(e.value)
        unchanged()
    # the raw call: count < 0, null arrays, a null handle, a bad stride, nq that does not fit self queries
    import ctypes as C

    lib = a.lib
    hs = (C.c_void_p * 2)(a.h, b.h)
    qp = (C.c_void_p * 2)(qa.ctypes.data, qb.ctypes.data)
    tot = (C.c_longlong * 2)(-7, -7)
    ok = dict(nq=(C.c_int * 2)(65, 63), st=(C.c_int * 2)(12, 12), r=(C.c_double * 2)(0.5, 0.5), m=(C.c_int * 2)(0, 0))

    def call(handles=hs, count=2, q=qp, **over):
        k = dict(ok)
        k.update(over)
        return lib.gorio_search_radius_batch(handles, count, q, k["nq"], k["st"], k["r"], k["m"], None, tot)

    assert call(count=-1) == INVALID
    assert call(handles=None) == INVALID and call(q=None) == INVALID and call(nq=None) == INVALID
    assert call(handles=(C.c_void_p * 2)(a.h, None)) == INVALID and b"job 1" in lib.gorio_search_last_error()
    assert call(st=(C.c_int * 2)(12, 10)) == INVALID and b"job 1" in lib.gorio_search_last_error()
    assert call(nq=(C.c_int * 2)(-1, 63)) == INVALID and b"job 0" in lib.gorio_search_last_error()
    assert call(q=(C.c_void_p * 2)(qa.ctypes.data, None)) == INVALID and b"job 1" in lib.gorio_search_last_error()  # NULL queries, nq != the cloud's size
    assert call(count=0) == 0
    assert list(tot) == [-7, -7]
    unchanged()
    assert call() == 0 and list(tot) == [held[0][1], held[1][1]]  # count_out == NULL is legal
