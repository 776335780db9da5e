"""The drop-in pclomp::NormalDistributionsTransform (go-rio_amd/host/pclomp/ndt_omp.h) built by the factory's setter calls
(registrations.cpp:117-134) and driven through a pcl::Registration base pointer as ndt_omp/apps/align.cpp does
(host/test/ndt_sequence.cpp): the pose equals the ctypes binding's bit for bit.  Without a GPU the constructor throws."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import ndt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "ndt_sequence")


def _write(path, target, source):
    with open(path, "wb") as f:
        f.write(struct.pack("i", 2))
        for c in (target, source):
            f.write(struct.pack("i", c.shape[0]))
            f.write(np.concatenate([c, np.zeros((c.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def test_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/ndt_sequence"])
    assert os.path.exists(DRIVER)
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    src, tgt, _ = S.real_pair()
    path = str(tmp_path / "pair.bin")
    _write(path, tgt[:500], src[:500])
    r = subprocess.run([DRIVER, path, "1.0", "DIRECT7"], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # the constructor throws: no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1"])
def test_sequence_matches_python_binding(gpu, gorio, tmp_path, search):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_sequence"])
    src, tgt, T = S.real_pair()
    path = str(tmp_path / "pair.bin")
    _write(path, tgt, src)
    r = subprocess.run([DRIVER, path, "1.0", search], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    n = gorio.Ndt(device=gpu, resolution=1.0, transformation_epsilon=0.01, max_iterations=64, search=getattr(gorio.ndt, search))
    n.set_target(tgt)
    n.set_source(src)
    res = n.align()
    assert np.array_equal(np.array(out["T"], np.float32).reshape(4, 4), res["T"])  # bit for bit
    assert bool(out["converged"]) == res["converged"] and out["iterations"] == res["nr_iterations"]
    assert out["n_derivatives"] == res["n_derivatives"] and out["n_mt"] == res["n_mt"]
    assert out["probability"] == res["trans_probability"]
    # calculateScore of the aligned cloud: the binding scores the source moved by the same float matrix
    assert out["score_aligned"] == pytest.approx(n.calculate_score(res["T"]), rel=1e-12)
    # getFitnessScore (apps/align.cpp:30, SMO:675): the registration ABI's fitness pass over the same clouds and pose
    g = gorio.ApdGicp(device=gpu)
    g.setInputTarget(tgt, np.zeros(tgt.shape[0], np.float32))
    g.setInputSource(src, np.zeros(src.shape[0], np.float32))
    assert out["fitness"] == pytest.approx(g.getFitnessScore(res["T"])[0], rel=1e-12) and 0 < out["fitness"] < 1e6
    n.close()


@pytest.mark.gpu
def test_kdtree_is_refused_by_the_dropin(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_sequence"])
    src, tgt, _ = S.real_pair()
    path = str(tmp_path / "pair.bin")
    _write(path, tgt[:500], src[:500])
    r = subprocess.run([DRIVER, path, "1.0", "KDTREE"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "KDTREE" in r.stderr
