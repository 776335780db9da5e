"""pclomp::NormalDistributionsTransform fed by gorio::ScanPreprocessor, through go-rio_amd/host/test/ndt_scan_sequence: the front end
with the default registration over a few raw radar messages and one scan-to-submap step.  Route A (setInputSourceFromScan /
setInputTargetFromScan / setInputTargetSubmap: the frame stays on the device) and route B (setInputSource / setInputTarget with the
host clouds) must agree bit for bit in every pose and every fitness score, and route A must not move the pipeline's counters."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_pipeline_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "ndt_scan_sequence")
IDENTITY_BITS = [int(x) for x in np.eye(4, dtype=np.float32).reshape(-1).view(np.uint32)]


def _write(path, scans, rotation, ang_vel, seed):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scans)))
        f.write(np.asarray(rotation, np.float64).reshape(9).tobytes())
        f.write(struct.pack("iii", 0, sr.OUTLIER_STATISTICAL, 1))
        f.write(np.asarray(ang_vel, np.float64).tobytes())
        f.write(struct.pack("I", seed))
        for raw in scans:
            f.write(struct.pack("i", raw.shape[0]))
            f.write(np.ascontiguousarray(raw, np.float32).tobytes())


def test_ndt_scan_driver_builds(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/ndt_scan_sequence"])
    assert os.path.exists(DRIVER)


def test_ndt_scan_driver_refuses_without_gpu(gorio, tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/ndt_scan_sequence"])
    path = str(tmp_path / "scans.bin")
    _write(path, [sr.raw_scan(3, n_ground=200, movers=10)], np.eye(3), (0, 0, 0), 1)
    r = subprocess.run([DRIVER, path, "1.0", "0.5"], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_scan_fed_route_equals_the_host_route_bit_for_bit(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_scan_sequence"])
    rot = sr.tilt()
    scans = [sr.raw_scan(seed, n_ground=sr.SEQUENCE_N_GROUND, rotation=rot) for seed in sr.SEQUENCE_SEEDS[:4]]
    scans.insert(2, scans[0][:0])  # an empty message in the middle: no frame, nothing is handed over, the keyframe stays
    path = str(tmp_path / "scans.bin")
    _write(path, scans, rot, sr.CHAIN_ANG_VEL, 4242)
    r = subprocess.run([DRIVER, path, "1.0", "0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    a, b = [x for x in lines if x["route"] == "A"], [x for x in lines if x["route"] == "B"]
    assert len(a) == len(b) == len(scans) + 1 and a[-1]["submap"] == 1 and b[-1]["submap"] == 1
    n_ok = n_aligned = n_moved = 0
    for x, y in zip(a, b):
        for key in ("frame", "submap", "status", "n", "aligned", "converged", "iterations"):
            assert x[key] == y[key], (x["frame"], key, x[key], y[key])
        assert x["T_bits"] == y["T_bits"], x["frame"]  # the pose: the same float bits
        assert x["fitness"] == y["fitness"] and x["probability"] == y["probability"], x["frame"]  # 17 digits: the same doubles
        assert x["before"] == x["after"], x["frame"]  # route A: hand-offs, align and fitness score move no counter of the pipeline
        if not x["submap"]:
            n_ok += x["status"] == 0
            n_aligned += x["aligned"]
        if x["aligned"]:
            n_moved += x["iterations"] >= 1 and x["T_bits"] != IDENTITY_BITS and x["fitness"] < 1e300
    assert a[2]["status"] == 2 and n_ok == 4 and n_aligned == n_ok - 1  # every frame after the first is matched against its keyframe
    assert a[-1]["aligned"] == 1 and n_moved == n_aligned + 1  # the matches did work: a trivial answer cannot pass for agreement
    assert len({tuple(x["T_bits"]) for x in a if x["aligned"]}) == n_aligned + 1  # the frames differ
    # over the whole sequence the pipeline built its own two indices per frame (outlier stage, DBSCAN) and downloaded each frame once
    # (what process() publishes): nothing for the registrations or the fitness scores
    uploads, builds, downloads = a[-1]["after"]
    assert builds == 2 * n_ok and downloads == n_ok and uploads >= n_ok
