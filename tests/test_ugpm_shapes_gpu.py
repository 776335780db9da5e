"""GPU parity of the UGPM GP pre-integration at the window shapes where the device switches kernels and code paths with the number of
GP states S (listed in tests/ugpm_shape_cases.py), at small S and other state rates, with irregular gyro / ego-velocity streams, on ROS
epoch stamps, in one mixed batch, at the 160-state cap and for awkward query times.  Every window is compared with the CPU oracle under
the gates of test_ugpm_gpu._cmp, and the solver diagnostics must be equal."""
import importlib

import numpy as np
import pytest

import ugpm_shape_cases as cases
from test_ugpm_gpu import _cmp, _cmp_chunked

synth = importlib.import_module("go-rio_amd.synth")
pytestmark = pytest.mark.gpu

_DIAG = ("nb_state", "nb_gyr", "nb_vel", "iters_rot", "iters_vel")
_LPM_GATES = dict(rot_tol=1e-10, pos_tol=1e-10, cov_rtol=1e-9, jac_rtol=1e-6)  # sequential integration on both sides (test_ugpm_gpu)
ERR_UNSUPPORTED = -5  # GORIO_UGPM_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def ugpm_oracle():
    import oracle
    from oracle import ugpm as u

    oracle.build()
    return u


def _oracle(u, c):
    kw = dict(c["kw"])
    if "quantum" in kw:
        r, d = u.preintegrate_chunked(c["win"], kw.pop("quantum"), **kw)
        return r[0], d
    return u.preintegrate(c["win"], **kw)


def _device_kw(c):
    kw = dict(c["kw"])
    if "infer_t" in kw:
        kw["infer_t"] = [kw["infer_t"]]
    return kw


def _device(gorio, c):
    r, d = gorio.ugpm_preint_batch([c["win"]], return_diag=True, **_device_kw(c))
    return r[0], d[0]


def _check(c, rg, dg, ro, do):
    """Device records and diagnostics against the oracle's for one case; returns the worst (rotation, position) difference."""
    assert dg["status"] == 0
    if c["kw"].get("type") == cases.LPM:
        return tuple(np.max([_cmp(a, b, **_LPM_GATES) for a, b in zip(rg, ro)], axis=0))
    keys = _DIAG if "quantum" not in c["kw"] else ("nb_state", "iters_rot", "iters_vel")  # a chunked request reports its last chunk
    assert [dg[k] for k in keys] == [do[k] for k in keys], (c["name"], dg, do)
    if c["S"] is not None:
        assert dg["nb_state"] == c["S"]
    cmp = _cmp_chunked if "quantum" in c["kw"] else _cmp
    assert len(rg) == len(ro)
    worst = [cmp(a, b) for a, b in zip(rg, ro)]
    return tuple(np.max(worst, axis=0))


@pytest.mark.parametrize("S", cases.SWEEP_S)
def test_state_count_sweep(gpu, gorio, ugpm_oracle, S):
    """One window at every S where a kernel choice switches (and on both sides of each switch), up to the 160-state cap.  Same algorithm,
    same arithmetic: the C2 bound (rotation and position < 1e-7) holds at every S.  The oracle's own rounding sensitivity on the S = 160
    window (gyro and velocity samples scaled by 1 +- 1e-14) is 1e-14 rad and 1.5e-10 m, far below it."""
    c = cases.sweep_case(S)
    ro, do = _oracle(ugpm_oracle, c)
    rg, dg = _device(gorio, c)
    rot, pos = _check(c, rg, dg, ro, do)
    print(f"S = {S}: rotation {rot:.2e} rad, position {pos:.2e} m")
    assert rot < 1e-7 and pos < 1e-7, (rot, pos)


@pytest.mark.parametrize("c", cases.small_cases(), ids=lambda c: c["name"])
def test_small_state_counts_and_state_rates(gpu, gorio, ugpm_oracle, c):
    """Overlap 0..4 and state rates 10..100 Hz: S from 5 to 25, matrices smaller than one 16 x 16 MFMA tile."""
    ro, do = _oracle(ugpm_oracle, c)
    rg, dg = _device(gorio, c)
    print(c["name"], "rotation %.2e rad, position %.2e m" % _check(c, rg, dg, ro, do))


@pytest.mark.parametrize("c", cases.rate_cases(), ids=lambda c: c["name"])
def test_sensor_rates_jitter_and_dropouts(gpu, gorio, ugpm_oracle, c):
    ro, do = _oracle(ugpm_oracle, c)
    rg, dg = _device(gorio, c)
    print(c["name"], "rotation %.2e rad, position %.2e m" % _check(c, rg, dg, ro, do))


@pytest.mark.parametrize("pair", cases.epoch_cases(), ids=lambda p: p[0]["name"])
def test_epoch_stamps(gpu, gorio, ugpm_oracle, pair):
    """Every time moved by 1.6e9 s plus a fraction.  The device against the oracle on the same stamps, under the gates; then against the
    oracle on the unshifted window.  There the stamps' own rounding (2.4e-7 s near 1.6e9) is all that differs, and the pose and covariance
    gates hold.  The numeric Jacobians do not stay within 1e-3 of their unshifted values, in either restatement: they are difference
    quotients over 0.01 s time shifts and 1e-4 rad/s bias steps (PRE:352-379, 1265-1399), which amplify the stamp rounding to 1e-3 relative
    (tests/test_oracle_ugpm_shapes.py pins that in both oracles), and a chained covariance inherits it.  So the device's Jacobians and
    covariance may be no further from the unshifted ones than the oracle's on the same stamps are, plus the gate."""
    c, plain = pair
    rg, dg = _device(gorio, c)
    ro, do = _oracle(ugpm_oracle, c)
    same = _check(c, rg, dg, ro, do)
    rp, dp = _oracle(ugpm_oracle, plain)
    assert dg["nb_state"] == dp["nb_state"]
    unshifted = _cmp_unshifted(_cmp_chunked if "quantum" in c["kw"] else _cmp, rg, ro, rp)
    print(c["name"], "same stamps: rotation %.2e rad, position %.2e m; unshifted oracle: rotation %.2e rad, position %.2e m, "
          "covariance / Jacobians %.1e relative (oracle on the shifted stamps %.1e)" % (same + unshifted))


_JAC = ("d_delta_R_d_bw", "d_delta_R_d_t", "d_delta_p_d_bw", "d_delta_p_d_bv", "d_delta_p_d_t")


def _cmp_unshifted(cmp, rg, ro, rp):
    """Device records on epoch stamps `rg` against the oracle's on the unshifted window `rp`: dt to one stamp spacing, the pose under the
    gates of `cmp`; covariance and Jacobians no further from rp than the oracle's own records on the epoch stamps `ro` are, plus 1e-3."""
    worst, jw, jo = [], 0.0, 0.0
    for a, o, b in zip(rg, ro, rp):
        assert abs(a["dt"] - b["dt"]) <= np.spacing(cases.EPOCH + 20.0)
        worst.append(cmp(a, dict(b, dt=a["dt"], dt_sq_half=a["dt_sq_half"], **{k: a[k] for k in ("cov",) + _JAC})))
        for k in ("cov",) + _JAC:
            scale = max(np.abs(b[k]).max(), 1e-6)
            da, do = np.abs(a[k] - b[k]).max() / scale, np.abs(o[k] - b[k]).max() / scale
            assert da <= do + 1e-3, (k, da, do)
            jw, jo = max(jw, da), max(jo, do)
    return tuple(np.max(worst, axis=0)) + (jw, jo)


def _all_cases():
    return cases.sweep_cases() + cases.small_cases() + cases.rate_cases() + [e for e, _ in cases.epoch_cases()]


def _batch(gorio, cs):
    """One UgpmBatch over cases with per-window options (the ABI carries type, quantum, overlap and state_freq per window)."""
    infer_t = [c["kw"].get("infer_t", [c["win"]["end_t"]]) for c in cs]
    b = gorio.UgpmBatch([c["win"] for c in cs], infer_t=infer_t, quantum=[c["kw"].get("quantum", -1.0) for c in cs])
    for k, c in enumerate(cs):
        b.arr[k].type = c["kw"].get("type", gorio.ugpm.UGPM)
        b.arr[k].overlap = c["kw"].get("overlap", 8)
        b.arr[k].state_freq = c["kw"].get("state_freq", 50.0)
    return b


def _records(b, k):
    o = sum(b.counts[:k])
    return b.out[o:o + b.counts[k]]


def test_mixed_batch_equals_single_windows(gpu, gorio):
    """Every case above in ONE batch: max_S = 160 selects the kernel templates for all of them, S = 5 windows included, beside LPM and
    chunked requests on epoch stamps.  Each window must equal its own single-window call bit for bit."""
    cs = _all_cases()
    b = _batch(gorio, cs)
    b.run()
    diag = b.diagnostics()
    assert all(d["status"] == 0 for d in diag)
    for k, c in enumerate(cs):
        s = _batch(gorio, [c])
        s.run()
        assert np.array_equal(_records(s, 0), _records(b, k)), c["name"]
        ds = s.diagnostics()[0]
        assert [ds[q] for q in _DIAG] == [diag[k][q] for q in _DIAG], c["name"]


def test_window_past_the_cap_is_refused_alone(gpu, gorio):
    """S = 161 between an S = 160 and an S = 21 window: the call reports GORIO_UGPM_ERR_UNSUPPORTED, only that window carries the status and
    NaN records, and the other two equal their single-window calls."""
    cs = [cases.sweep_case(160), dict(name="S161", win=synth.window_for_states(161, seed=1161), kw={}, S=161), cases.sweep_case(21)]
    b = _batch(gorio, cs)
    with pytest.raises(gorio.GorioError) as e:
        b.run()
    assert e.value.code == ERR_UNSUPPORTED
    diag = b.diagnostics()
    assert [d["status"] for d in diag] == [0, ERR_UNSUPPORTED, 0]
    assert np.isnan(_records(b, 1)).all()
    for k in (0, 2):
        s = _batch(gorio, [cs[k]])
        s.run()
        assert np.array_equal(_records(s, 0), _records(b, k)), cs[k]["name"]
        assert diag[k]["nb_state"] == cs[k]["S"]


def test_query_at_start_duplicated_and_unsorted(gpu, gorio, ugpm_oracle):
    """Queries end_t, start_t exactly, a duplicated stamp and one out of order.  At start_t the oracle's covariance is 0 / 0 in the
    correlation scaling (NaN, as in the SciPy restatement): the device must give NaN at the same places and match everywhere else."""
    w = synth.window_for_states(66, seed=5066)
    q = [w["end_t"], w["start_t"], w["start_t"] + 0.4, w["start_t"] + 0.4, w["start_t"] + 0.7]
    c = dict(name="queries", win=w, kw=dict(infer_t=q), S=66)
    ro, do = _oracle(ugpm_oracle, c)
    rg, dg = _device(gorio, c)
    assert [dg[k] for k in _DIAG] == [do[k] for k in _DIAG]
    for j, (a, b) in enumerate(zip(rg, ro)):
        for k in a:
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), (j, k)
        if np.isnan(b["cov"]).any():
            a, b = dict(a, cov=np.nan_to_num(a["cov"])), dict(b, cov=np.nan_to_num(b["cov"]))
        _cmp(a, b)
    assert np.isnan(ro[1]["cov"]).all() and ro[1]["dt"] == 0.0
    assert np.array_equal(rg[1]["delta_R"], np.eye(3)) and np.array_equal(rg[1]["delta_p"], np.zeros(3)) and rg[1]["dt"] == 0.0
    for k in rg[2]:
        assert np.array_equal(rg[2][k], rg[3][k]), k  # the same stamp twice: the same record
