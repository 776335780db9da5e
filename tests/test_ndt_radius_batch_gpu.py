"""gorio_ndt_align_batch and gorio_ndt_calculate_score_batch with handles whose radius switch is on, mixed with DIRECT handles.

The contract is equality with the single call, so every comparison is == / np.array_equal: each member's outputs are bit for bit those
of gorio_ndt_align / gorio_ndt_calculate_score on a fresh handle with the same clouds, parameters, switch and guess.  The launch count
of a round stays within the bound include/gorio_ndt.h states (ndt.radius_round_launch_bound)."""
import numpy as np
import pytest

import ndt_restatement as R
import ndt_scenes as S

pytestmark = pytest.mark.gpu
SIZES = [257, 1, 300, 64, 513, 63, 256]
SEARCHES = [R.DIRECT7, R.DIRECT1, R.DIRECT26]
FIELDS = ("converged", "nr_iterations", "trans_probability", "n_derivatives", "n_hessians", "n_mt", "score")
TYPICAL = dict(transformation_epsilon=0.01, max_iterations=64)


@pytest.fixture(scope="module")
def real():
    src, tgt, _ = S.real_pair()
    return src, tgt[:2048]


def _guess(rng):
    G = np.eye(4, dtype=np.float32)
    a = np.deg2rad(rng.uniform(-1.0, 1.0))
    G[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    G[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    return G


def _cases(src, count, direct_leads=False):
    """Member i: its source slice, guess, switch and parameters.  Radius and DIRECT alternate, member 0 (whose scratch carries the rounds)
    being a radius handle unless direct_leads; the
    last member of a batch of three or more starts 5 km away, has no neighbour and is done after its first evaluation."""
    rng = np.random.default_rng(300 + count)
    far = np.eye(4, dtype=np.float32)
    far[:3, 3] = [5000.0, 0.0, 0.0]
    out = []
    for i in range(count):
        size, first = SIZES[i % len(SIZES)], 131 * i
        guess = far if (count >= 3 and i == count - 1) else (np.eye(4, dtype=np.float32) if i == 0 else _guess(rng))
        out.append((src[first:first + size], guess, (i % 2 == 0) != direct_leads, dict(search=SEARCHES[i % 3], **TYPICAL)))
    return out


def _handle(gorio, gpu, tgt, src, radius, params):
    n = gorio.Ndt(device=gpu, radius_search=radius, **params)
    n.set_target(tgt)
    n.set_source(src)
    return n


def _evals(r):
    return r["n_derivatives"] + r["n_hessians"]


@pytest.mark.parametrize("count,direct_leads", [(1, False), (3, False), (3, True), (7, False)])
def test_align_batch_equals_single_bit_for_bit(gorio, gpu, real, count, direct_leads):
    src, tgt = real
    cases = _cases(src, count, direct_leads)
    singles, lists = [], []
    for s, g, radius, p in cases:
        n = _handle(gorio, gpu, tgt, s, radius, p)
        singles.append(n.align(g))
        lists.append(n.neighbours() if radius else None)
        n.close()
    if count >= 3:
        assert singles[-1]["n_derivatives"] == 1 and singles[-1]["nr_iterations"] == 0  # the member that converges at once
    hs = [_handle(gorio, gpu, tgt, s, radius, p) for s, _, radius, p in cases]
    res, stats = gorio.ndt.align_batch(hs, [g for _, g, _, _ in cases])
    for a, b in zip(res, singles):
        assert np.array_equal(a["T"], b["T"]), (a["T"], b["T"])
        for k in FIELDS:
            assert a[k] == b[k], (k, a[k], b[k])
    assert stats.rounds == max(_evals(r) for r in singles) and stats.evaluations == sum(_evals(r) for r in singles)
    assert stats.launches <= gorio.ndt.radius_round_launch_bound(max(s.shape[0] for s, _, radius, _ in cases if radius)) * stats.rounds
    for h, (_, _, radius, _), ref in zip(hs, cases, lists):  # the neighbour lists held are those of the member's last evaluation
        if radius:
            assert all(np.array_equal(a, b) for a, b in zip(h.neighbours(), ref))
        h.close()


@pytest.mark.parametrize("count", [1, 3, 7])
def test_score_batch_equals_single_bit_for_bit(gorio, gpu, real, count):
    src, tgt = real
    cases = _cases(src, count)
    hs = [_handle(gorio, gpu, tgt, s, radius, p) for s, _, radius, p in cases]
    Ts = [g for _, g, _, _ in cases]
    singles = np.array([h.calculate_score(T) for h, T in zip(hs, Ts)])
    batch = gorio.ndt.calculate_score_batch(hs, Ts)
    assert np.array_equal(batch, singles) and (singles[:1] != 0).all()
    flipped = [not radius for _, _, radius, _ in cases]  # the same handles with every switch turned over
    for h, radius in zip(hs, flipped):
        h.set_radius_search(radius)
    singles2 = np.array([h.calculate_score(T) for h, T in zip(hs, Ts)])
    assert np.array_equal(gorio.ndt.calculate_score_batch(hs, Ts), singles2) and singles2[0] != singles[0]
    for h in hs:
        h.close()


def test_sharers_of_one_target_in_one_batch(gorio, gpu, real):
    """Two radius handles and a DIRECT one look at ONE target state (one centroid index); each has its own search state."""
    src, tgt = real
    rng = np.random.default_rng(9)
    cases = [(src[0:300], np.eye(4, dtype=np.float32), True), (src[300:557], _guess(rng), True), (src[600:900], _guess(rng), False)]
    singles = []
    for s, g, radius in cases:
        n = _handle(gorio, gpu, tgt, s, radius, TYPICAL)
        singles.append(n.align(g))
        n.close()
    owner = _handle(gorio, gpu, tgt, cases[0][0], True, TYPICAL)
    hs = [owner]
    for s, _, radius in cases[1:]:
        n = gorio.Ndt(device=gpu, radius_search=radius, **TYPICAL)
        n.set_source(s)
        n.set_target_shared(owner)
        hs.append(n)
    res, _ = gorio.ndt.align_batch(hs, [g for _, g, _ in cases])
    for a, b in zip(res, singles):
        assert np.array_equal(a["T"], b["T"]) and all(a[k] == b[k] for k in FIELDS)
    for h in hs:
        h.close()
