"""The C++ drop-in class fast_gicp::NDTCuda (go-rio_amd/host/fast_gicp/ndt/ndt_cuda.hpp) driven through a pcl::Registration base pointer
in the nodelet's call order (host/test/ndt_cuda_sequence.cpp), compared with the ctypes binding of the same ABI: the float bits of every
pose are equal."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _frames

apd = importlib.import_module("go-rio_amd.apd")
DRIVER = os.path.join(HOST, "test", "ndt_cuda_sequence")


def test_driver_builds_and_headers_carry_the_surface(gorio):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_cuda_sequence"])
    assert os.path.exists(DRIVER)
    text = open(os.path.join(HOST, "fast_gicp", "ndt", "ndt_cuda.hpp")).read()
    for member in ("setDistanceMode(NDTDistanceMode mode)", "setResolution(double resolution)", "setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0)",
                   "swapSourceAndTarget()", "clearSource()", "clearTarget()", "alignBatch(", "setInputTargetShared(", "getFitnessScoreBatch(", "setInputSourceFromScan(",
                   "setInputTargetFromScan("):
        assert member in text, member
    assert "enum class NDTDistanceMode { P2D, D2D };" in open(os.path.join(HOST, "fast_gicp", "ndt", "ndt_settings.hpp")).read()


@pytest.mark.gpu
def test_class_through_base_pointer_matches_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_cuda_sequence"])
    path, frames = _frames(str(tmp_path))
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]
    for name, mode in (("P2D", apd.NDT_CUDA_P2D), ("D2D", apd.NDT_CUDA_D2D)):
        mine = [l for l in lines if l["mode"] == name]
        aligns = [l for l in mine if l["step"] == "align"]
        assert len(aligns) == len(frames) - 1
        g = gorio.ApdGicp()
        g.set_ndt_cuda_params(mode)
        g.set_method(apd.METHOD_NDT_CUDA, 2.0, apd.VOXEL_DIRECT7)

        def same(out, res, h=None):
            h = h or g
            assert np.array(out["T"], np.float32).reshape(4, 4).tobytes() == res["T"].tobytes() and bool(out["converged"]) == res["converged"]
            assert out["fitness"] == pytest.approx(h.getFitnessScore(res["T"])[0], rel=1e-12)

        prev = np.eye(4, dtype=np.float32)
        g.setInputTarget(*frames[0])
        for k in range(1, len(frames)):
            g.setInputSource(*frames[k])
            res = g.align(prev)
            same(aligns[k - 1], res)
            if res["converged"]:
                prev = res["T"]
            if k % 2 == 0:  # new keyframe
                g.setInputTarget(*frames[k])
                prev = np.eye(4, dtype=np.float32)
        steps = {l["step"]: l for l in mine if l["step"] != "batch" and l["step"] != "align"}
        g.setInputTarget(*frames[0])
        g.setInputSource(*frames[1])
        g.align()
        assert steps["voxels"]["target"] == len(g.ndt_cuda_voxels(1)["num_points"]) and steps["voxels"]["source"] == len(g.ndt_cuda_voxels(0)["num_points"])
        assert (steps["voxels"]["source"] == 0) == (name == "P2D")
        g.swapSourceAndTarget()
        same(steps["swapped"], g.align())
        g.set_ndt_cuda_params(mode, 1.5)
        g.set_method(apd.METHOD_NDT_CUDA, 1.0, apd.VOXEL_DIRECT_RADIUS)
        same(steps["radius"], g.align())
        batch = [l for l in mine if l["step"] == "batch"]
        assert len(batch) == len(frames) - 1
        for k in range(1, len(frames)):
            o = gorio.ApdGicp()
            o.set_ndt_cuda_params(mode)
            o.set_method(apd.METHOD_NDT_CUDA, 2.0, apd.VOXEL_DIRECT7)
            o.setInputTarget(*frames[0])
            o.setInputSource(*frames[k])
            same(batch[k - 1], o.align(), o)
