"""gorio::ScanPreprocessor<PointXYZINormal> (go-rio_amd/host/radar_preprocessing/scan_preprocessor.hpp) and
FastAPDGICP::setInputSourceFromScan / setInputTargetFromScan, through go-rio_amd/host/test/preprocess_sequence: a sequence of raw radar
messages replayed through the class and through the single calls with host compaction (apps/preprocessing_nodelet_ntu.cpp:370-581).
The two must agree exactly, frame by frame, with the Patchwork++ state carried by each."""
import os
import struct
import subprocess

import numpy as np
import pytest

import scan_pipeline_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "preprocess_sequence")
ANG_VEL = sr.CHAIN_ANG_VEL


def _write(path, scans, rotation, dor, method, ang_vel, seed):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scans)))
        f.write(np.asarray(rotation, np.float64).reshape(9).tobytes())
        f.write(struct.pack("iii", int(dor), int(method), 0 if ang_vel is None else 1))
        f.write(np.asarray(ang_vel if ang_vel is not None else (0, 0, 0), np.float64).tobytes())
        f.write(struct.pack("I", seed))
        for raw in scans:
            f.write(struct.pack("i", raw.shape[0]))
            f.write(np.ascontiguousarray(raw, np.float32).tobytes())


def _read(path, k):
    """k messages x (class, single calls): dicts of the header, the published cloud's bytes and the registration result."""
    out = []
    with open(path, "rb") as f:
        for _ in range(2 * k):
            status, n_out, n_ground, n_clusters = struct.unpack("iiii", f.read(16))
            v = f.read(48)
            cloud = f.read(24 * n_out)
            aligned, = struct.unpack("i", f.read(4))
            T = f.read(64)
            conv, = struct.unpack("i", f.read(4))
            out.append(dict(status=status, n_out=n_out, n_ground=n_ground, n_clusters=n_clusters, v=v, cloud=cloud, aligned=aligned, T=T, converged=conv))
        assert f.read() == b""
    return out[0::2], out[1::2]


def test_preprocess_driver_builds(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/preprocess_sequence"])
    assert os.path.exists(DRIVER)


def test_preprocess_driver_refuses_without_gpu(gorio, tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/preprocess_sequence"])
    path = str(tmp_path / "scans.bin")
    _write(path, [sr.raw_scan(3, n_ground=200, movers=10)], np.eye(3), False, sr.OUTLIER_STATISTICAL, None, 1)
    r = subprocess.run([DRIVER, path, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("dor,method", [(False, sr.OUTLIER_STATISTICAL), (True, sr.OUTLIER_RADIUS)])
def test_class_sequence_equals_single_calls_with_host_compaction(gpu, gorio, tmp_path, dor, method):
    subprocess.check_call(["make", "-C", HOST, "test/preprocess_sequence"])
    rot = sr.tilt()
    scans = [sr.raw_scan(seed, n_ground=sr.SEQUENCE_N_GROUND, rotation=rot) for seed in sr.SEQUENCE_SEEDS]
    scans.insert(2, scans[0][:0])  # an empty message in the middle: no frame, and the state of neither chain moves
    s0 = scans[0]
    scans.insert(4, s0[np.isfinite(s0).all(1) & (s0[:, 3] > 0)][:20])  # mean_k points: the statistical filter refuses, both chains go on
    path, out = str(tmp_path / "scans.bin"), str(tmp_path / "out.bin")
    _write(path, scans, rot, dor, method, ANG_VEL, 4242)
    r = subprocess.run([DRIVER, path, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a, b = _read(out, len(scans))
    n_ok = n_aligned = 0
    for k, (x, y) in enumerate(zip(a, b)):
        for key in ("status", "n_out", "n_ground", "n_clusters", "aligned", "converged"):
            assert x[key] == y[key], (k, key, x[key], y[key])
        assert x["v"] == y["v"], k       # v_r and sigma_v_r, the same bits
        assert x["cloud"] == y["cloud"], k  # points, intensity, Doppler and labels in the published order
        assert x["T"] == y["T"], k       # setInput*FromScan + align against setInput* + align
        n_ok += x["status"] == 0
        n_aligned += x["aligned"]
    assert a[2]["status"] == 2 and n_ok >= len(sr.SEQUENCE_SEEDS) and n_aligned == n_ok - 1
    if method == sr.OUTLIER_STATISTICAL:
        assert a[4]["status"] == 3  # refused by the class as by the single call, and the frames after it still agree
    assert all(x["n_ground"] > 0 and x["n_clusters"] >= 1 for x in a if x["status"] == 0)
    assert len({x["n_ground"] for x in a}) > 2  # the frames differ: one frame's answer cannot pass for another's
