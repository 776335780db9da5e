"""The J^T J of the state correlation skips the gyro rows of the Jacobian for the output tiles those rows cannot reach (ata_kernel,
which = 2: tile rows at or behind column 3S, workgroups that start at chunk floor(3G / KC)).  gorio_ugpm_debug_set_path(1) selects the
dense kernel path -- the plain cut of the tiles, every workgroup over every row -- in the same library.  The two must give the same
records BIT FOR BIT, and the records must match the CPU oracle under the gates of test_ugpm_gpu._cmp.  Shapes: the smallest at which the
skip can go wrong -- 3S on a tile edge (S = 32) and inside a tile (S = 22, 66), 3G on a chunk edge and inside a chunk, the KC = 8
instantiation (S = 116), 1, 9 and 24 windows per batch, and a window without the correlation step."""
import importlib

import numpy as np
import pytest

from test_ugpm_gpu import _cmp

synth = importlib.import_module("go-rio_amd.synth")
ug = importlib.import_module("go-rio_amd.ugpm")
pytestmark = pytest.mark.gpu

_DIAG = ("nb_state", "nb_gyr", "nb_vel", "iters_rot", "iters_vel")


@pytest.fixture(scope="module")
def ugpm_oracle():
    import oracle
    from oracle import ugpm as u

    oracle.build()
    return u


def _gyro_inside(win, S, overlap=8, state_freq=50.0):
    """Indices of the gyro samples strictly inside the state window (preint.h:777-789): they are the G rows x 3 of the Jacobian."""
    t0 = win["start_t"] - overlap / state_freq
    t = np.asarray(win["gyr_t"])
    return np.nonzero((t > t0) & (t < t0 + (S - 1) / state_freq))[0]


def window(S, seed, chunk, rem):
    """A 200 Hz window with S states whose gyro sample count G inside the state window has G % chunk == rem (3G % chunk == 3 rem % chunk;
    chunk = 16 or 8 = KC): samples from the middle of the window are dropped until it has."""
    win = synth.window_for_states(S, seed=seed)
    idx = _gyro_inside(win, S)
    drop = (len(idx) - rem) % chunk
    if drop:
        mid = idx[len(idx) // 2]
        win = synth.perturb_stream(win, "gyr", seed + 1, drop=tuple(range(mid, mid + 2 * drop, 2)))
    assert len(_gyro_inside(win, S)) % chunk == rem and synth.ugpm_state_count(win)[0] == S
    return win


def _run(gorio, wins, dense, correlate=None):
    b = gorio.UgpmBatch(wins)
    for k, c in enumerate(correlate or []):
        b.arr[k].correlate = int(c)
    try:
        ug.ugpm_debug_set_path(dense_ata=dense)
        b.run()
    finally:
        ug.ugpm_debug_set_path()
    diag = b.diagnostics()
    assert all(d["status"] == 0 for d in diag)
    return b.out.copy(), b.results(), diag


# (S, chunk = KC of the instantiation, G % chunk): 3S = 96 is a tile edge, 66 and 198 lie inside a tile; G % chunk = 0 puts 3G on a chunk edge
_SHAPES = [(32, 16, 0), (32, 16, 5), (22, 16, 0), (22, 16, 7), (66, 16, 0), (66, 16, 3), (116, 8, 0), (116, 8, 3)]


@pytest.mark.parametrize("S,chunk,rem", _SHAPES)
def test_single_window_dense_and_skipping_paths(gpu, gorio, ugpm_oracle, S, chunk, rem):
    win = window(S, 7000 + S, chunk, rem)
    dense, _, dd = _run(gorio, [win], True)
    skip, rs, ds = _run(gorio, [win], False)
    assert ds[0]["nb_state"] == S and ds[0]["nb_gyr"] % chunk == rem
    assert np.array_equal(dense, skip) and np.isfinite(skip).all()
    assert [dd[0][k] for k in _DIAG] == [ds[0][k] for k in _DIAG]
    ro, do = ugpm_oracle.preintegrate(win)
    assert [ds[0][k] for k in _DIAG] == [do[k] for k in _DIAG]
    print("S = %d, G = %d: rotation %.2e rad, position %.2e m" % ((S, ds[0]["nb_gyr"]) + _cmp(rs[0][0], ro[0])))


@pytest.fixture(scope="module")
def batch_windows():
    """24 windows of S = 22, 32 and 66 in turn (max_S = 66 sizes the grid for all), G on and off a chunk edge."""
    return [window((22, 32, 66)[q % 3], 7100 + q, 16, (0, 5, 11, 0)[q % 4]) for q in range(24)]


@pytest.fixture(scope="module")
def single_records(gorio, gpu, batch_windows):
    """Every window of batch_windows alone, on the skipping path (computed once, shared, never modified)."""
    out = np.stack([_run(gorio, [w], False)[0][0] for w in batch_windows])
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("n", [1, 9, 24])
def test_batches_dense_and_skipping_paths(gpu, gorio, batch_windows, single_records, n):
    """1 window, 9 (one full row of 8 workgroup slots and a partial one) and 24: both paths equal each other and the single-window calls."""
    wins = batch_windows[:n]
    dense, _, _ = _run(gorio, wins, True)
    skip, _, _ = _run(gorio, wins, False)
    assert np.array_equal(dense, skip)
    assert np.array_equal(skip, single_records[:n])


def test_window_without_correlation_in_the_batch(gpu, gorio, ugpm_oracle, batch_windows, single_records):
    """correlate off for windows 1 and 4 of 9: they have no correlation Jacobian at all (no buffer is carved for it), their neighbours
    are unaffected, and both paths agree on every window."""
    wins = batch_windows[:9]
    corr = [q not in (1, 4) for q in range(9)]
    dense, _, _ = _run(gorio, wins, True, corr)
    skip, rs, ds = _run(gorio, wins, False, corr)
    assert np.array_equal(dense, skip)
    for q in range(9):
        if corr[q]:
            assert np.array_equal(skip[q], single_records[q])
    ro, do = ugpm_oracle.preintegrate(wins[1], correlate=False)
    assert [ds[1][k] for k in _DIAG] == [do[k] for k in _DIAG]
    _cmp(rs[1][0], ro[0])
    assert not np.array_equal(skip[1], single_records[1])  # the correlation does change the covariance of a record
