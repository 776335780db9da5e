"""CPU test: the two UGPM restatements (oracle/ugpm_oracle.cpp, oracle/ugpm_scipy.py) at the window shapes where the device switches
code paths (tests/ugpm_shape_cases.py), on irregular streams and on epoch stamps, before tests/test_ugpm_shapes_gpu.py holds the device
to the C++ side there.  Every window must land on its intended number of GP states S in both restatements, so that the device sweep
sits on its boundaries, and the C++ oracle must not depend on where the time axis starts beyond the rounding of the stamps themselves."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation as Rot

import ugpm_shape_cases as cases
from test_oracle_ugpm_scipy import _agree

synth = importlib.import_module("go-rio_amd.synth")

_STATE_CASES = cases.sweep_cases() + cases.small_cases() + [c for c in cases.rate_cases() if c["S"] is not None]


@pytest.fixture(scope="module")
def both():
    import oracle
    from oracle import ugpm as cpp
    from oracle import ugpm_scipy as sp

    oracle.build()
    return cpp, sp


def _opts(c):
    return dict(state_freq=c["kw"].get("state_freq", 50.0), overlap=c["kw"].get("overlap", 8))


@pytest.mark.parametrize("c", _STATE_CASES, ids=lambda c: c["name"])
def test_window_state_count_and_restatements_agree(both, c):
    """S from the helper's own restatement of preint.h:766-775, from the C++ oracle and from SciPy; then the measurement of both sides."""
    cpp, sp = both
    assert synth.ugpm_state_count(c["win"], **_opts(c))[0] == c["S"]
    ro, do = cpp.preintegrate(c["win"], **c["kw"])
    rs, ds = sp.preintegrate(c["win"], **c["kw"])
    assert do["nb_state"] == ds["nb_state"] == c["S"]
    assert (do["nb_gyr"], do["nb_vel"]) == (ds["nb_gyr"], ds["nb_vel"])
    assert do["state_freq"] == pytest.approx(ds["state_freq"], rel=1e-14)
    _agree(rs[0], ro[0], pos_tol=_pos_tol(rs[0]))


def _pos_tol(m):
    """_agree's 5e-7 m, or 8e-8 of the distance travelled on long windows.  The C++ side stops the velocity fit where Ceres would (relative
    cost decrease 1e-10, PRE:948) and SciPy runs on: at S = 160 (12 m in 2.87 s) its velocity cost is 4e-8 relative above SciPy's, and
    delta_p differs by 6.7e-7 m (5.6e-8 of the distance)."""
    return max(5e-7, 8e-8 * np.linalg.norm(m["delta_p"]))


def test_refused_window_is_one_state_past_the_cap(both):
    """The device refuses S > 160 (GORIO_UGPM_ERR_UNSUPPORTED); the window the GPU test uses for that is S = 161 in the oracle."""
    cpp, _ = both
    w = synth.window_for_states(161, seed=1161)
    assert synth.ugpm_state_count(w)[0] == 161 and cpp.preintegrate(w)[1]["nb_state"] == 161


def test_irregular_streams_clamp_the_state_rate(both):
    """Gyro 400 Hz, ego-velocity 12 Hz with +-20 % stamp jitter and 3 lost frames: the state rate is the velocity stream's mean rate."""
    cpp, sp = both
    c = [c for c in cases.rate_cases() if c["name"] == "g400_v12"][0]
    vt = c["win"]["vel_t"]
    _, do = cpp.preintegrate(c["win"])
    _, ds = sp.preintegrate(c["win"])
    assert do["state_freq"] == pytest.approx((len(vt) - 1) / (vt[-1] - vt[0]), rel=1e-14) == pytest.approx(11.0, abs=0.1)
    assert do["state_freq"] == pytest.approx(ds["state_freq"], rel=1e-14) and do["nb_state"] == ds["nb_state"] == 33
    assert np.diff(vt).max() > 1.5 / 12.0  # a dropped frame really left a gap (two periods, less at most 2 x 20 % jitter)


@pytest.mark.parametrize("name", ["epoch_S21", "epoch_S160", "epoch_lpm"])
def test_restatements_agree_on_epoch_stamps(both, name):
    cpp, sp = both
    c = [e for e, _ in cases.epoch_cases() if e["name"] == name][0]
    ro, do = cpp.preintegrate(c["win"], **c["kw"])
    rs, ds = sp.preintegrate(c["win"], **c["kw"])
    if c["S"] is not None:
        assert do["nb_state"] == ds["nb_state"] == c["S"]
    for a, b in zip(rs, ro):  # LPM too: the two sides difference stamps 2.4e-7 s apart in different orders (1e-6 m at 5 m/s at most)
        _agree(a, b, pos_tol=_pos_tol(a))


@pytest.mark.parametrize("S", [21, 66, 134, 160])
def test_oracle_shift_invariance_at_epoch_stamps(both, S):
    """The same window with every time moved by 1.6e9 s.  The shifted stamps are rounded to the 2.4e-7 s spacing of doubles near 1.6e9,
    which is all that may change: measured over S = 21..160, rotation <= 2.4e-7 rad, position <= 1.4e-6 m, covariance <= 1.9e-4
    relative and dt <= 1.2e-7 s; bounds at about 4x those, inside the 1e-4 / 1e-3 gates of SURVEY 8d.  dt = end - start of two rounded
    stamps can be off by one spacing at most.  The numeric Jacobians are difference quotients over 0.01 s time shifts and 1e-4 rad/s bias
    steps (PRE:352-379, 1265-1399) and amplify that rounding: 0.6e-3 to 4.7e-3 of their size measured, bound 1e-2.  The SciPy restatement
    moves the same way (test_restatements_agree_on_epoch_stamps holds the two to 1e-6 on the shifted stamps): a property of the
    algorithm on epoch stamps, not of either restatement."""
    cpp, _ = both
    shifted, plain = [(e, p) for e, p in cases.epoch_cases() if e["name"] == f"epoch_S{S}"][0]
    ra, da = cpp.preintegrate(shifted["win"])
    rb, db = cpp.preintegrate(plain["win"])
    assert da["nb_state"] == db["nb_state"] == S and (da["iters_rot"], da["iters_vel"]) == (db["iters_rot"], db["iters_vel"])
    a, b = ra[0], rb[0]
    rot = np.linalg.norm(Rot.from_matrix(b["delta_R"].T @ a["delta_R"]).as_rotvec())
    pos = np.linalg.norm(a["delta_p"] - b["delta_p"])
    cov = np.abs(a["cov"] - b["cov"]).max() / np.abs(b["cov"]).max()
    assert rot < 1e-6 and pos < 5e-6 and cov < 1e-3, (rot, pos, cov)
    assert abs(a["dt"] - b["dt"]) <= np.spacing(cases.EPOCH + 20.0)
    for k in ("d_delta_R_d_bw", "d_delta_R_d_t", "d_delta_p_d_bw", "d_delta_p_d_bv", "d_delta_p_d_t"):
        assert np.abs(a[k] - b[k]).max() <= 1e-2 * max(np.abs(b[k]).max(), 1e-6), k
