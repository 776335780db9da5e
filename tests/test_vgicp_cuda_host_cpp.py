"""The C++ drop-in class fast_gicp::FastVGICPCuda (go-rio_amd/host/fast_gicp/gicp/fast_vgicp_cuda.hpp) driven through a pcl::Registration
base pointer in the nodelet's call order (host/test/vgicp_cuda_sequence.cpp), compared with the ctypes binding of the same ABI: the float
bits of every pose are equal."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _frames

apd = importlib.import_module("go-rio_amd.apd")
DRIVER = os.path.join(HOST, "test", "vgicp_cuda_sequence")
MODES = (("KDTREE", apd.NN_CPU_PARALLEL_KDTREE), ("BRUTEFORCE", apd.NN_GPU_BRUTEFORCE), ("RBF", apd.NN_GPU_RBF_KERNEL))


def test_driver_builds_and_header_carries_the_surface(gorio):
    subprocess.check_call(["make", "-C", HOST, "test/vgicp_cuda_sequence"])
    assert os.path.exists(DRIVER)
    text = open(os.path.join(HOST, "fast_gicp", "gicp", "fast_vgicp_cuda.hpp")).read()
    for member in ("enum class NearestNeighborMethod { CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL };", "class FastVGICPCuda : public FastGICP<PointSource, PointTarget>",
                   "setCorrespondenceRandomness(int) {}", "setResolution(double resolution)", "setKernelWidth(double kernel_width, double max_dist = -1.0)",
                   "setRegularizationMethod(RegularizationMethod method)", "setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0)",
                   "setNearestNeighborSearchMethod(NearestNeighborMethod method)", "swapSourceAndTarget()", "clearSource()", "clearTarget()",
                   "setInputSource(const PointCloudSourceConstPtr& cloud)", "setInputTarget(const PointCloudTargetConstPtr& cloud)", "alignBatch(", "setInputTargetShared(",
                   "getFitnessScoreBatch(", "setInputSourceFromScan(", "setInputTargetFromScan("):
        assert member in text, member
    assert "setInputSourceKeyframe" in open(os.path.join(HOST, "fast_gicp", "gicp", "fast_gicp.hpp")).read()  # inherited


@pytest.mark.gpu
def test_class_through_base_pointer_matches_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/vgicp_cuda_sequence"])
    path, frames = _frames(str(tmp_path))
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [json.loads(l) for l in r.stdout.strip().splitlines()]

    def new(nn):
        o = gorio.ApdGicp()
        o.set_vgicp_cuda_params(nn, 0.5, 2.5)  # setKernelWidth(0.5): max_dist = 5 widths
        o.set_method(apd.METHOD_VGICP_CUDA, 2.0, apd.VOXEL_DIRECT7)
        return o

    for name, nn in MODES:
        mine = [l for l in lines if l["mode"] == name]
        aligns = [l for l in mine if l["step"] == "align"]
        assert len(aligns) == len(frames) - 1
        g = new(nn)

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
        c = steps["counts"]
        assert c["voxels"] == len(g.vgicp_cuda_voxels()["num_points"])
        assert (c["kept_source"], c["kept_target"]) == (len(g.vgicp_cuda_points(0)["kept_index"]), len(g.vgicp_cuda_points(1)["kept_index"]))
        assert 0 < c["kept_source"] <= c["source"] and 0 < c["kept_target"] <= c["target"]
        g.swapSourceAndTarget()
        same(steps["swapped"], g.align())
        g.set_params(regularization=1)  # MIN_EIG
        g.set_ndt_cuda_params(apd.NDT_CUDA_D2D, 1.5)
        g.set_method(apd.METHOD_VGICP_CUDA, 1.0, apd.VOXEL_DIRECT_RADIUS)
        same(steps["radius"], g.align())
        batch = [l for l in mine if l["step"] == "batch"]
        assert len(batch) == len(frames) - 1
        for k in range(1, len(frames)):
            o = new(nn)
            o.setInputTarget(*frames[0])
            o.setInputSource(*frames[k])
            same(batch[k - 1], o.align(), o)
    poses = {name: [l["T"] for l in lines if l["mode"] == name and "T" in l] for name, _ in MODES}
    assert poses["KDTREE"] == poses["BRUTEFORCE"] and poses["KDTREE"] != poses["RBF"]  # one path, and another
