"""gorio::GpuSearch (go-rio_amd/host/gorio/gpu_search.hpp) through its driver host/test/search_sequence.cpp on a 2 k cloud: the batch
overloads, the single-point overloads and the form that shares the target of a FastAPDGICP agree with each other, and with the
values this test passes in from tests/search_restatement.py (exact equality, checked inside the driver)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import search_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "search_sequence")


def _case(tmp_path, n=2000, nq=150, k=7, radius=2.5, max_nn=9, spoil=False):
    rng = np.random.default_rng(21)
    xyz = rng.uniform(-15.0, 15.0, (n, 3)).astype(np.float32)
    xyz[n // 2:] = np.round(xyz[n // 2:])  # half of the cloud on the integer lattice: equal distances
    q = (xyz[rng.integers(0, n, nq)] + rng.normal(0.0, 0.4, (nq, 3))).astype(np.float32)
    q[: nq // 3] = np.round(q[: nq // 3])
    idx, sqd, cnt = R.knn(xyz, q, k)
    offs, ridx, rsqd = R.radius(xyz, q, radius, max_nn)
    if spoil:
        idx = idx.copy()
        idx[nq // 2, 0] += 1
    path = os.path.join(tmp_path, "spoiled.bin" if spoil else "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("i", n) + xyz.tobytes() + struct.pack("i", nq) + q.tobytes() + struct.pack("i", k) + struct.pack("d", radius) + struct.pack("i", max_nn))
        f.write(idx.astype(np.int32).tobytes() + sqd.astype(np.float32).tobytes() + cnt.astype(np.int32).tobytes())
        f.write(offs.astype(np.int64).tobytes() + ridx.astype(np.int32).tobytes() + rsqd.astype(np.float32).tobytes())
    return path


def test_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/search_sequence"])
    assert os.path.exists(DRIVER)
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    r = subprocess.run([DRIVER, _case(str(tmp_path), n=50, nq=5, k=3)], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_overloads_agree_with_each_other_and_the_restatement(gpu, gorio, tmp_path):
    r = subprocess.run([DRIVER, _case(str(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert (out["n"], out["nq"], out["k"]) == (2000, 150, 7)
    assert (out["knn_ok"], out["radius_ok"], out["pick_ok"], out["single_ok"], out["shared_ok"]) == (1, 1, 1, 1, 1)
    assert out["empty_ok"] == 1  # no queries: empty lists, not an error
    assert (out["own_uploads"], out["own_builds"]) == (1, 1)
    # the driver does compare: one expected index off by one is reported
    r = subprocess.run([DRIVER, _case(str(tmp_path), spoil=True)], capture_output=True, text=True, timeout=120)
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert r.returncode == 1 and out["knn_ok"] == 0 and out["radius_ok"] == 1
