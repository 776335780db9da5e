"""The C++ drop-in gorio::IterativeClosestPoint (go-rio_amd/host/gorio/icp.hpp) driven through a pcl::Registration base pointer by
go-rio_amd/host/test/icp_sequence.cpp: the factory's setter calls (registrations.cpp:72-79), then the odometry nodelet's call order
(scan_matching_odometry_nodelet.cpp:430-479) over three frames against one keyframe, each align seeded with the previous transformation.
Its JSON is held against the NumPy restatement (iterations, state, pairs, pose within 1e-4 m / 1e-4 rad); the driver's batch of the same
aligns must equal its singles bit for bit."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import icp_restatement as R
import icp_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "icp_sequence")
# reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance, reg_use_reciprocal_correspondences
LAUNCH = dict(transformation_epsilon=1e-5, max_iterations=64, max_correspondence_distance=1.0, use_reciprocal=False)
SOURCES = [257, 513, 256]


def frames():
    return [S.target(2000)] + [S.source(n, 2000) for n in SOURCES]


def restate(source, guess):
    return R.align(source, S.target(2000), guess, **LAUNCH)


def _write(path, clouds):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(clouds)))
        for xyz in clouds:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def test_the_sequence_is_decided_with_margin():
    """The restatement alone, each align seeded with the one before: every criterion has a relative margin above icp_scenes.MARGIN."""
    guess = np.eye(4, dtype=np.float32)
    for src in frames()[1:]:
        r = restate(src, guess)
        print("%d points: %d iterations, state %d, margin %.3e" % (src.shape[0], r["nr_iterations"], r["state"], r["margin"]))
        assert r["converged"] and r["margin"] > S.MARGIN
        guess = r["T"]


@pytest.mark.gpu
def test_cpp_sequence_matches_the_restatement(gorio, gpu, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/icp_sequence"], stdout=subprocess.DEVNULL)
    path = os.path.join(str(tmp_path), "frames.bin")
    _write(path, frames())
    args = [DRIVER, path, repr(LAUNCH["transformation_epsilon"]), str(LAUNCH["max_iterations"]), repr(LAUNCH["max_correspondence_distance"]), str(int(LAUNCH["use_reciprocal"]))]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["defaults"] == dict(max_iterations=10, transformation_epsilon=0.0, fitness_epsilon_is_lowest=1, distance_is_sqrt_max=1, reciprocal=0)
    assert len(out["aligns"]) == len(SOURCES)
    guess = np.eye(4, dtype=np.float32)
    for src, got in zip(frames()[1:], out["aligns"]):
        want = restate(src, guess)  # the guess the driver used: its own previous transformation
        T = np.array(got["T"], np.float32).reshape(4, 4)
        dt, dr = S.pose_error(want["T"], T)
        print("%d points: %d / %d iterations, state %d / %d, pose error %.3e m %.3e rad" % (src.shape[0], got["iterations"], want["nr_iterations"], got["state"], want["state"], dt, dr))
        assert want["margin"] > S.MARGIN
        assert (got["converged"], got["iterations"], got["state"], got["pairs"]) == (int(want["converged"]), want["nr_iterations"], want["state"], want["pairs"])
        assert dt <= 1e-4 and dr <= 1e-4
        assert abs(got["mse"] - want["mse"]) <= 1e-6 * want["mse"]
        assert np.array_equal(np.array(got["aligned0"], np.float32), R.transform_f(T, src[:1])[0])
        # pcl::Registration::getFitnessScore at the final transformation: the mean squared nearest-neighbour distance of the moved source
        _, sqd = R.nearest(R.transform_f(T, src), S.target(2000))
        assert abs(got["fitness"] - float(sqd.astype(np.float64).mean())) <= 1e-9 * got["fitness"]
        if got["converged"]:
            guess = T
    assert out["batch_equals_singles"] == 1
    assert out["rounds"] == out["longest"] and out["launches"] <= 3 * out["rounds"]
    assert out["batch_fitness"] == [a["fitness"] for a in out["aligns"]]
