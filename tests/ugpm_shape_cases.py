"""The GP pre-integration windows of tests/test_oracle_ugpm_shapes.py (CPU: the two restatements) and tests/test_ugpm_shapes_gpu.py
(the device against the oracle), built once here so that both files exercise exactly the same shapes.

Each case is dict(name, win, kw, S): `kw` are the request options (state_freq, overlap, type, quantum, infer_t) in the keyword form of
oracle.ugpm.preintegrate / gorio.ugpm_preint_batch, and `S` the number of GP states the request must have (None for LPM requests).
Where the device switches code paths with S (ugpm_api.hip launch_ata, block_cholesky, lm_step_kernel, infer_kernel's LDS budget):
  correlation J^T J, n = 6 S:          ata_kernel<4,16> / <8,16> / <16,8>  at S <= 40 / 41..82 / >= 83
  velocity-fit J^T J, n = 3 S:         ata_kernel<4,16> / <8,16>           at S <= 80 / >= 81
  correlation Cholesky, n = 6 S:       one pass with look-ahead / several  at S <= 66 / >= 67
  rotation-fit LM step, ns = 3 S:      fused / unfused one pass / several  at S <= 127 / 128..133 / >= 134
  infer_kernel LDS:                    163 744 of 163 840 B                at S = 160, the cap; S = 161 is refused
"""
import importlib

synth = importlib.import_module("go-rio_amd.synth")

SWEEP_S = (21, 40, 41, 66, 67, 80, 81, 82, 83, 127, 128, 133, 134, 159, 160)
EPOCH = 1.6e9 + 0.123456789  # ROS epoch seconds (header.stamp.toSec()) with a fractional part that is no short binary fraction
LPM = 0


def sweep_case(S):
    """One 200 Hz / 200 Hz window at the default overlap 8 and 50 Hz state rate: duration (S - 16 - 0.5) / 50."""
    return dict(name=f"S{S}", win=synth.window_for_states(S, seed=1000 + S), kw={}, S=S)


def sweep_cases():
    return [sweep_case(S) for S in SWEEP_S]


def small_cases():
    """Overlap 0, 1, 2 and 4 at state rates 10, 20 and 100 Hz (S = 2 overlap + 5..7, all below one 16 x 16 MFMA tile), plus the shapes the
    oracle pair was pinned on first: overlap 0 with S = 25 and with S = 5 (a 0.1 s window), overlap 1 with S = 7."""
    out = []
    for i, (ov, sf) in enumerate([(ov, sf) for ov in (0, 1, 2, 4) for sf in (10.0, 20.0, 100.0)]):
        S = 2 * ov + 5 + i % 3
        out.append(dict(name=f"ov{ov}_f{sf:g}_S{S}", win=synth.window_for_states(S, seed=2000 + i, overlap=ov, state_freq=sf), kw=dict(overlap=ov, state_freq=sf), S=S))
    for ov, S in ((0, 25), (0, 5), (1, 7)):
        out.append(dict(name=f"ov{ov}_S{S}", win=synth.window_for_states(S, seed=2100 + S, overlap=ov), kw=dict(overlap=ov), S=S))
    return out


def rate_cases():
    """Gyro at 100, 400 and 1000 Hz with ego-velocity at 10, 12 and 20 Hz, both streams jittered (velocity +-20 % of its period, gyro
    +-10 %) and velocity frames dropped; the state rate clamps to the velocity stream's mean rate.  Then the LPM output type on a 200 Hz
    and a 1000 Hz gyro (at 1000 Hz the 500 Hz min_freq fill of preint.h:228 adds no stamps)."""
    out = []
    for gyr_hz, vel_hz, S, drop in ((100.0, 10.0, 30, (7,)), (400.0, 12.0, 33, (5, 9, 14)), (1000.0, 20.0, 50, (3, 20))):
        win = synth.window_for_states(S, seed=3000 + int(gyr_hz), gyr_hz=gyr_hz, vel_hz=vel_hz, gyr_jitter=0.1, vel_jitter=0.2, vel_drop=drop)
        out.append(dict(name=f"g{gyr_hz:g}_v{vel_hz:g}", win=win, kw={}, S=S))
    for gyr_hz in (200.0, 1000.0):
        win = synth.perturb_stream(synth.imu_window(seed=3100 + int(gyr_hz), duration=1.2, gyr_hz=gyr_hz, vel_hz=12.0), "vel", 3200, jitter=0.2, drop=(6,))
        q = [win["start_t"] + 0.35, win["start_t"] + 0.8, win["end_t"]]
        out.append(dict(name=f"lpm_g{gyr_hz:g}", win=win, kw=dict(type=LPM, infer_t=q), S=None))
    return out


def epoch_cases():
    """S = 21, 66, 134 and 160, one LPM request and one chunked request (quantum 0.7123 s over a 2 s window, stamps in every chunk), each
    with every time moved by EPOCH.  Returns (case on epoch stamps, the same case unshifted)."""
    base = [sweep_case(S) for S in (21, 66, 134, 160)]
    w = synth.imu_window(seed=4001, duration=1.0, vel_hz=20.0)
    base.append(dict(name="lpm", win=w, kw=dict(type=LPM, infer_t=[w["start_t"] + 0.4, w["end_t"]]), S=None))
    w = synth.imu_window(seed=4002, duration=2.0)
    # quantum 0.7123, not 0.7: chunk ends 0.7 k after start_t fall exactly on 200 Hz stamps, and which chunk such a sample joins is then
    # decided by the rounding of the stamps (on epoch stamps the last chunk's fit sees different data and differs by 1e-4 m)
    base.append(dict(name="chunked", win=w, kw=dict(quantum=0.7123, infer_t=[w["start_t"] + 0.6, w["start_t"] + 1.3, w["end_t"]]), S=None))
    out = []
    for c in base:
        kw = dict(c["kw"])
        if "infer_t" in kw:
            kw["infer_t"] = [t + EPOCH for t in kw["infer_t"]]
        out.append((dict(name="epoch_" + c["name"], win=synth.shift_window(c["win"], EPOCH), kw=kw, S=c["S"]), c))
    return out
