"""The GP solver kernels (gram_kernel, lm_step_kernel, corr_diag_kernel, infer_kernel) run in instantiations whose LDS panel rows and
register blocks are sized to the largest window of the batch (solver_sizes, ugpm_windows.h; tests/test_ugpm_footprint.py checks the rule
on the CPU).  gorio_ugpm_debug_set_path bit 2 selects the capacities of the largest system of the library for all of them, in the same
library.  A sized instantiation runs the same instructions on the same data, so the raw 83-double records must be the same BITS, and they
must match the CPU oracle under the gates of tests/test_ugpm_shapes_gpu.py.  Shapes: S = 17 (the smallest window at the default overlap),
66 (the scan-to-scan step's), 160 (the cap), and both sides of every switch point of the rule: 69 | 70 (lm_step_kernel's panel rows),
88 | 89 (blocks per wave of the 6 S-row solves), 96 | 97 (gram_kernel's panel rows)."""
import importlib

import numpy as np
import pytest

from test_ugpm_gpu import _cmp

synth = importlib.import_module("go-rio_amd.synth")
ug = importlib.import_module("go-rio_amd.ugpm")
pytestmark = pytest.mark.gpu

_DIAG = ("nb_state", "nb_gyr", "nb_vel", "iters_rot", "iters_vel")
_S = (17, 66, 69, 70, 88, 89, 96, 97, 160)
_MIXED = (17, 66, 97)  # max_S = 97 lies above every switch point: the two small windows run the largest instantiations there


@pytest.fixture(scope="module")
def ugpm_oracle():
    import oracle
    from oracle import ugpm as u

    oracle.build()
    return u


def _window(S):
    return synth.window_for_states(S, seed=8000 + S)


def _run(gorio, wins, full, correlate=True):
    b = gorio.UgpmBatch(wins)
    for k in range(len(wins)):
        b.arr[k].correlate = int(correlate)
    try:
        ug.ugpm_debug_set_path(full_capacity=full)
        b.run()
    finally:
        ug.ugpm_debug_set_path()
    diag = b.diagnostics()
    assert all(d["status"] == 0 for d in diag)
    return np.ascontiguousarray(b.out).view(np.uint64).copy(), b.results(), diag


@pytest.fixture(scope="module")
def sized_single(gorio, gpu):
    """The sized path's raw records of one window alone, per S (computed once per S, shared, never modified)."""
    cache = {}

    def get(S):
        if S not in cache:
            bits, res, diag = _run(gorio, [_window(S)], False)
            bits.setflags(write=False)
            cache[S] = (bits, res, diag)
        return cache[S]

    return get


@pytest.mark.parametrize("S", _S)
def test_sized_and_full_capacity_paths(gpu, gorio, ugpm_oracle, sized_single, S):
    win = _window(S)
    sized, rs, ds = sized_single(S)
    full, _, df = _run(gorio, [win], True)
    assert ds[0]["nb_state"] == S
    assert sized.shape == full.shape and sized.shape[-1] == 83 and np.array_equal(sized, full)
    assert [ds[0][k] for k in _DIAG] == [df[0][k] for k in _DIAG]
    ro, do = ugpm_oracle.preintegrate(win)
    assert [ds[0][k] for k in _DIAG] == [do[k] for k in _DIAG]
    rot, pos = _cmp(rs[0][0], ro[0])
    print(f"S = {S}: rotation {rot:.2e} rad, position {pos:.2e} m")
    assert rot < 1e-7 and pos < 1e-7, (rot, pos)  # the bound of test_state_count_sweep


def test_window_without_correlation(gpu, gorio, ugpm_oracle, sized_single):
    """correlate off: no correlation system exists, corr_diag_kernel returns at once and infer_kernel takes the diagonal covariance."""
    win = _window(66)
    sized, rs, ds = _run(gorio, [win], False, correlate=False)
    full, _, _ = _run(gorio, [win], True, correlate=False)
    assert np.array_equal(sized, full)
    assert not np.array_equal(sized, sized_single(66)[0])  # the correlation does change the covariance of a record
    ro, do = ugpm_oracle.preintegrate(win, correlate=False)
    assert [ds[0][k] for k in _DIAG] == [do[k] for k in _DIAG]
    rot, pos = _cmp(rs[0][0], ro[0])
    assert rot < 1e-7 and pos < 1e-7, (rot, pos)


def test_mixed_batch_equals_single_windows(gpu, gorio, sized_single):
    """S = 17, 66 and 97 in one batch: the largest window selects the instantiations for all three, and each window equals its own
    single-window call (where S = 17 and 66 ran the small ones) bit for bit, on the sized path and with the full capacities."""
    wins = [_window(S) for S in _MIXED]
    sized, _, ds = _run(gorio, wins, False)
    full, _, _ = _run(gorio, wins, True)
    assert np.array_equal(sized, full)
    for k, S in enumerate(_MIXED):
        assert ds[k]["nb_state"] == S
        assert np.array_equal(sized[k], sized_single(S)[0][0]), S
