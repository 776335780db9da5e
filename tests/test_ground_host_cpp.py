"""The drop-in PatchWorkpp<PointXYZINormal> (go-rio_amd/host/patchworkpp/patchworkpp.hpp) driven the way the preprocessing nodelet
drives it (apps/preprocessing_nodelet_ntu.cpp:502-519), through go-rio_amd/host/test/ground_sequence."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ground_scenes as gs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "ground_sequence")


def _write(path, scans):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scans)))
        for xyz, inten in scans:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, inten[:, None]], axis=1).astype(np.float32).tobytes())


def _read(path, k):
    out = []
    with open(path, "rb") as f:
        for _ in range(k):
            ng, nf = struct.unpack("ii", f.read(8))
            out.append((ng, np.frombuffer(f.read(16 * nf), np.float32).reshape(nf, 4)))
    return out


def test_ground_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST])
    assert os.path.exists(DRIVER)
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    path = str(tmp_path / "scans.bin")
    _write(path, [gs.scan(1, n_ground=200, extras=False)])
    r = subprocess.run([DRIVER, path, str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("id", [0, 1])
def test_ground_sequence_matches_python_binding(gpu, gorio, tmp_path, id):
    scans = gs.sequence(7, frames=8)
    path, out = str(tmp_path / "scans.bin"), str(tmp_path / "out.bin")
    _write(path, scans)
    r = subprocess.run([DRIVER, path, out, str(id)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = _read(out, len(scans))
    seg = gorio.ground.GroundSegmenter()
    for (xyz, inten), (ng, full) in zip(scans, got):
        g, n = seg.estimate(xyz, inten, id=id)
        idx = np.concatenate([g, n])
        assert ng == len(g)
        want = np.concatenate([xyz, inten[:, None]], axis=1)[idx]
        assert full.tobytes() == want.astype(np.float32).tobytes()
