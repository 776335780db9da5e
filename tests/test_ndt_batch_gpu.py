"""gorio_ndt_align_batch and gorio_ndt_set_target_shared (include/gorio_ndt.h) on the GPU.

The contract of the batch is equality with the single call: every output of handle i is, bit for bit, that of gorio_ndt_align on a
fresh handle with the same clouds, parameters and guess.  So every comparison here is == / np.array_equal, without a tolerance.  One
test anchors the shared-target batch to tests/ndt_restatement.py with the comparison tests/test_ndt_gpu.py applies to a single align."""
import numpy as np
import pytest

import ndt_restatement as R
import ndt_scenes as S
from conftest import rot_err

pytestmark = pytest.mark.gpu
SEARCHES = [R.DIRECT1, R.DIRECT7, R.DIRECT26]
SIZES = [1, 63, 64, 65, 255, 256, 257, 300, 513]  # the workgroup-table edges: last workgroup partial, full, or a single point
FIELDS = ("converged", "nr_iterations", "trans_probability", "n_derivatives", "n_hessians", "n_mt", "score")
TYPICAL = dict(transformation_epsilon=0.01, max_iterations=64)


@pytest.fixture(scope="module")
def real():
    return S.real_pair()


def _guess(rng, scale=1.0):
    """A small perturbation of the identity: up to 1 degree of yaw, 0.1 m per axis (times scale)."""
    G = np.eye(4, dtype=np.float32)
    a = np.deg2rad(rng.uniform(-1.0, 1.0)) * scale
    G[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    G[:3, 3] = rng.uniform(-0.1, 0.1, 3) * scale
    return G


def _handle(gorio, gpu, tgt, src, **params):
    n = gorio.Ndt(device=gpu, **params)
    if tgt is not None:
        n.set_target(tgt)
    if src is not None:
        n.set_source(src)
    return n


def _single(gorio, gpu, tgt, src, guess, **params):
    """gorio_ndt_align on a fresh handle with a private target."""
    n = _handle(gorio, gpu, tgt, src, **params)
    r = n.align(guess)
    n.close()
    return r


def _same(a, b):
    assert np.array_equal(a["T"], b["T"]), (a["T"], b["T"])
    for k in FIELDS:
        assert a[k] == b[k], (k, a[k], b[k])


def _evals(r):
    return r["n_derivatives"] + r["n_hessians"]


@pytest.mark.parametrize("count", [1, 2, 3, 9])
def test_batch_equals_single_bit_for_bit(gorio, gpu, real, count):
    src, tgt, _ = real
    tgt = tgt[:2048]
    rng = np.random.default_rng(100 + count)
    cases = []
    for i in range(count):
        size = SIZES[i % len(SIZES)]
        first = 97 * i
        cases.append((src[first:first + size], None if i == 0 else _guess(rng), dict(search=SEARCHES[i % 3], **TYPICAL)))
    singles = [_single(gorio, gpu, tgt, s, g, **p) for s, g, p in cases]
    hs = [_handle(gorio, gpu, tgt, s, **p) for s, _, p in cases]
    res, stats = gorio.ndt.align_batch(hs, [np.eye(4, dtype=np.float32) if g is None else g for _, g, _ in cases])
    for a, b in zip(res, singles):
        _same(a, b)
    assert stats.rounds == max(_evals(r) for r in singles) and stats.evaluations == sum(_evals(r) for r in singles)
    assert stats.launches <= 4 * stats.rounds
    if count == 2:  # guesses = None is the identity for every handle
        res0, _ = gorio.ndt.align_batch(hs)
        for a, (s, _, p) in zip(res0, cases):
            _same(a, _single(gorio, gpu, tgt, s, None, **p))
    for h in hs:
        h.close()


def test_handles_finish_in_different_rounds_and_modes_mix(gorio, gpu, real):
    src, tgt, _ = real
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = [5000.0, 0.0, 0.0]  # no neighbours: the guess comes back after the first evaluation
    near = np.eye(4, dtype=np.float32)
    near[:3, 3] = [0.1, -0.1, 0.0]
    rng = np.random.default_rng(7)
    cases = [(far, {}), (near, dict(max_iterations=1, transformation_epsilon=1e-6)), (None, dict(step_size=0.1, **TYPICAL)), (_guess(rng), dict(step_size=0.05, **TYPICAL))]
    singles = [_single(gorio, gpu, tgt, src, g, **p) for g, p in cases]
    assert singles[0]["n_derivatives"] == 1 and np.array_equal(singles[0]["T"], far)
    # the <double, true> (computeHessian) and <float, false> (inner line-search) instantiations run in the single path, hence in the batch
    assert sum(r["n_hessians"] for r in singles) > 0 or sum(r["n_mt"] for r in singles) > 0
    assert len({_evals(r) for r in singles}) > 2  # they do finish in different rounds
    hs = [_handle(gorio, gpu, tgt, src, **p) for _, p in cases]
    res, stats = gorio.ndt.align_batch(hs, [np.eye(4, dtype=np.float32) if g is None else g for g, _ in cases])
    for a, b in zip(res, singles):
        _same(a, b)
    assert stats.rounds == max(_evals(r) for r in singles)
    assert stats.evaluations == sum(_evals(r) for r in singles)
    assert stats.launches <= 4 * stats.rounds
    for h in hs:
        h.close()


def _shared_cases(src, searches):
    rng = np.random.default_rng(11)
    return [(src[i::5], np.eye(4, dtype=np.float32) if i == 0 else _guess(rng), dict(search=searches[i % len(searches)], **TYPICAL)) for i in range(5)]


def _shared_handles(gorio, gpu, tgt, cases):
    owner = _handle(gorio, gpu, tgt, cases[0][0], **cases[0][2])
    hs = [owner]
    for s, _, p in cases[1:]:
        n = _handle(gorio, gpu, None, s, **p)
        n.set_target_shared(owner)
        hs.append(n)
    return hs


def test_shared_target(gorio, gpu, real):
    src, tgt, _ = real
    cases = _shared_cases(src, SEARCHES)
    private = [_single(gorio, gpu, tgt, s, g, **p) for s, g, p in cases]
    hs = _shared_handles(gorio, gpu, tgt, cases)
    guesses = [g for _, g, _ in cases]
    res, _ = gorio.ndt.align_batch(hs, guesses)
    for a, b in zip(res, private):
        _same(a, b)
    owner_caps = hs[0].capacities()
    assert owner_caps["target"] >= tgt.shape[0] and owner_caps["leaves"] > 0 and owner_caps["keys"] >= tgt.shape[0]
    for n in hs[1:]:
        c = n.capacities()
        assert (c["target"], c["leaves"], c["keys"]) == (0, 0, 0) and c["source"] > 0
    vo, vs = hs[0].voxels(), hs[3].voxels()
    assert vo["leaf_index"].size > 200
    for k in vo:
        assert np.array_equal(vo[k], vs[k]), k
    # a new target on one sharer detaches that sharer only
    other = S.clusters(3000, 5)
    hs[4].set_target(other)
    _same(hs[0].align(guesses[0]), private[0])
    _same(hs[1].align(guesses[1]), private[1])
    _same(hs[4].align(guesses[4]), _single(gorio, gpu, other, cases[4][0], guesses[4], **cases[4][2]))
    assert hs[4].capacities()["target"] >= other.shape[0]
    # the sharers outlive the owner
    hs[0].close()
    _same(hs[2].align(guesses[2]), private[2])
    res2, _ = gorio.ndt.align_batch(hs[1:4], guesses[1:4])
    for a, b in zip(res2, private[1:4]):
        _same(a, b)
    for n in hs[1:]:
        n.close()


def test_map_parameter_rule(gorio, gpu, real):
    src, tgt, _ = real
    owner = _handle(gorio, gpu, tgt, src[0::4], **TYPICAL)
    sharer = _handle(gorio, gpu, None, src[1::4], **TYPICAL)
    sharer.set_target_shared(owner)
    before, _ = gorio.ndt.align_batch([owner, sharer])  # builds the map at resolution 1.0
    sharer.set_params(resolution=0.5)
    for call in (sharer.align, lambda: sharer.derivatives(np.zeros(6))):
        with pytest.raises(gorio.GorioError) as e:
            call()
        assert e.value.code == -1 and "resolution" in str(e.value)  # GORIO_ERR_INVALID
    with pytest.raises(gorio.GorioError) as e:
        gorio.ndt.align_batch([owner, sharer])
    assert e.value.code == -1 and "handle 1" in str(e.value) and "resolution" in str(e.value)
    _same(owner.align(), before[0])  # the owner's map was not dropped under it
    sharer.set_params(resolution=1.0)
    after, _ = gorio.ndt.align_batch([owner, sharer])
    for a, b in zip(after, before):
        _same(a, b)
    sharer.close()
    # the only holder of a target still rebuilds after a changed resolution
    owner.set_params(resolution=0.5)
    _same(owner.align(), _single(gorio, gpu, tgt, src[0::4], None, resolution=0.5, **TYPICAL))
    fresh = _handle(gorio, gpu, tgt, None, resolution=0.5)
    vo, vf = owner.voxels(), fresh.voxels()
    for k in vo:
        assert np.array_equal(vo[k], vf[k]), k
    fresh.close()
    owner.close()


def test_validation_on_a_device(gorio, gpu, real):
    src, tgt, _ = real
    a = _handle(gorio, gpu, tgt[:2048], src[:300], **TYPICAL)
    b = _handle(gorio, gpu, tgt[:2048], src[300:813], search=R.DIRECT1, **TYPICAL)
    nosrc = _handle(gorio, gpu, tgt[:2048], None)
    before, _ = gorio.ndt.align_batch([a, b])
    with pytest.raises(gorio.GorioError) as e:
        gorio.ndt.align_batch([a, b, a])
    assert e.value.code == -1  # GORIO_ERR_INVALID
    after, _ = gorio.ndt.align_batch([a, b])
    for x, y in zip(after, before):
        _same(x, y)
    with pytest.raises(gorio.GorioError) as e:
        gorio.ndt.align_batch([a, b, nosrc])
    assert e.value.code == -3 and "handle 2" in str(e.value)  # GORIO_ERR_STATE
    after, _ = gorio.ndt.align_batch([b, a])
    _same(after[0], before[1])
    _same(after[1], before[0])
    for n in (a, b, nosrc):
        n.close()


def _anchor(r, src, tgt, guess, **params):
    """The comparison of tests/test_ndt_gpu.py::_align_both for a result r that is already there."""
    ref = R.Ndt(**{("min_points" if k == "min_points_per_voxel" else k): v for k, v in params.items()})
    ref.set_target(tgt)
    ref.set_source(src)
    q = ref.align(guess)
    dt, dr = rot_err(q["T"], r["T"])
    assert dt < 1e-4 and dr < 1e-4, (dt, dr)
    for k in ("converged", "nr_iterations", "n_derivatives", "n_hessians", "n_mt"):
        assert r[k] == q[k], (k, r[k], q[k])
    assert abs(r["trans_probability"] - q["trans_probability"]) <= 1e-6 * abs(q["trans_probability"]) + 1e-12


def test_shared_batch_against_the_restatement(gorio, gpu, real):
    src, tgt, _ = real
    cases = _shared_cases(src, [R.DIRECT7])
    hs = _shared_handles(gorio, gpu, tgt, cases)
    res, _ = gorio.ndt.align_batch(hs, [g for _, g, _ in cases])
    for n in hs:
        n.close()
    for i in (0, 3):
        s, g, p = cases[i]
        _anchor(res[i], s, tgt, g, **p)


def test_reuse_without_reallocation(gorio, gpu, real):
    src, tgt, _ = real
    tgt = tgt[:2048]
    rng = np.random.default_rng(3)
    sources = [src[:513], src[600:900], src[1000:1257]]
    guesses = [_guess(rng) for _ in sources]
    params = [dict(search=s, **TYPICAL) for s in SEARCHES]
    hs = [_handle(gorio, gpu, tgt, s, **p) for s, p in zip(sources, params)]
    res, _ = gorio.ndt.align_batch(hs, guesses)
    for a, s, g, p in zip(res, sources, guesses, params):
        _same(a, _single(gorio, gpu, tgt, s, g, **p))
    caps = [n.capacities() for n in hs]
    sources[0] = src[2000:2065]
    hs[0].set_source(sources[0])
    res, _ = gorio.ndt.align_batch(hs, guesses)
    for a, s, g, p in zip(res, sources, guesses, params):
        _same(a, _single(gorio, gpu, tgt, s, g, **p))
    assert [n.capacities() for n in hs] == caps  # nothing was reallocated
    for n in hs:
        n.close()
