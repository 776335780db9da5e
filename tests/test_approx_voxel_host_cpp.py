"""gorio::ApproximateVoxelGrid (go-rio_amd/host/gorio/approx_voxel_grid.hpp) and setSubmapDownsampleMethod of the C++ drop-in classes:
the header compiles against host/compat; on the GPU the driver go-rio_amd/host/test/approx_voxel_sequence.cpp prints what the Python
binding computes, bit for bit."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

synth = importlib.import_module("go-rio_amd.synth")
apd = importlib.import_module("go-rio_amd.apd")
prep = importlib.import_module("go-rio_amd.prep")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "approx_voxel_sequence")
F = np.float32
LEAF = 0.25


def _scene(n_frames=5, n=2000):
    frames, odoms = [], []
    for k in range(n_frames):
        odom = synth.gt_transform([0.6 * k, 0.05 * k, 0.01 * k], [0.1 * k, -0.05 * k, 1.2 * k])
        frames.append(synth.radar_scan(n + 37 * k, seed=900 + k, sensor_pose=odom))
        odoms.append(odom)
    rel = [np.linalg.inv(odoms[-1]) @ odoms[i] for i in range(n_frames - 1)]
    return frames, rel


def _write(tmp, frames, rel):
    fp, pp = os.path.join(tmp, "frames.bin"), os.path.join(tmp, "poses.bin")
    with open(fp, "wb") as f:
        f.write(struct.pack("i", len(frames)))
        for xyz, lab in frames:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, lab[:, None]], axis=1).astype(F).tobytes())
    with open(pp, "wb") as f:
        for T in rel:
            f.write(np.ascontiguousarray(T, np.float64).tobytes())
    return fp, pp


def _fnv(a):
    h = 1469598103934665603
    for b in np.ascontiguousarray(a, F).tobytes():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_header_compiles_against_compat(tmp_path):
    src = os.path.join(str(tmp_path), "use.cpp")
    with open(src, "w") as f:
        f.write("#include <gorio/approx_voxel_grid.hpp>\n"
                "template class gorio::ApproximateVoxelGrid<pcl::PointXYZINormal>;\n"
                "template class gorio::ApproximateVoxelGrid<pcl::PointXYZI>;\n"
                "static_assert(gorio::avg_point_fields<pcl::PointXYZINormal>::count == 8 && gorio::avg_point_fields<pcl::PointXYZI>::count == 4, \"fields\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + HOST, "-I" + os.path.join(HOST, "compat"), "-I" + os.path.join(ROOT, "include"), src])


def test_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/approx_voxel_sequence"], stdout=subprocess.DEVNULL)
    assert os.path.exists(DRIVER)
    import torch

    if torch.cuda.is_available():
        return  # the GPU test below runs the driver
    frames, rel = _scene(n_frames=2, n=100)
    r = subprocess.run([DRIVER, *_write(str(tmp_path), frames, rel), "0.25"], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_driver_equals_the_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/approx_voxel_sequence"], stdout=subprocess.DEVNULL)
    frames, rel = _scene()
    r = subprocess.run([DRIVER, *_write(str(tmp_path), frames, rel), repr(LEAF)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    # ---- the filter: frame 0 as PointXYZINormal rows (normal_x = label, intensity = 5 + label), all data, then x y z with three leaves
    xyz, lab = frames[0]
    z = np.zeros(len(xyz), F)
    rows = np.stack([xyz[:, 0], xyz[:, 1], xyz[:, 2], lab, z, z, F(5.0) + lab, z], axis=1).astype(F)
    want = prep.approx_voxel_downsample(rows, LEAF)
    got = out["filter"]
    assert (got["n"], got["hash"]) == (len(want), _fnv(want)) and 0 < got["n"] < len(xyz)
    assert (got["width"], got["height"], got["is_dense"]) == (len(want), 1, 0)
    assert np.array_equal(np.array(got["first"], F), want[0, [0, 1, 2, 3, 6]])
    assert out["default_all_data"] == 1
    leaf3 = np.array([LEAF, 2 * LEAF, 4 * LEAF], F)
    assert np.array_equal(np.array(out["leaf"], F), leaf3)
    want3 = prep.approx_voxel_downsample(xyz, leaf3.astype(np.float64))
    got3 = out["filter_xyz"]
    assert (got3["n"], got3["hash"]) == (len(want3), _fnv(want3)) and got3["first"][3:] == [0, 0]  # the fields left out keep a default point's zeros
    # ---- the submap in both forms, and the align against it
    keyframes, newest = frames[:-1], frames[-1]
    g = gorio.ApdGicp(transformation_epsilon=0.1, max_iterations=64, corr_dist_threshold=2.0, k_correspondences=20)
    g.setSubmapDownsample(apd.DOWNSAMPLE_APPROX_VOXELGRID)
    n = g.setInputTargetSubmap(keyframes, rel, voxel_leaf=LEAF)
    x, l = g.getTargetPoints()
    sub = np.concatenate([x, l[:, None]], axis=1)
    assert out["method"] == 1
    for key in ("submap_host", "submap_store"):
        assert (out[key]["n"], out[key]["hash"]) == (n, _fnv(sub)), key
    assert 0 < n < sum(len(f[0]) for f in keyframes)
    g.setInputSource(*newest)
    res = g.align()
    a = out["align"]
    assert (a["converged"], a["nr_iterations"]) == (int(res["converged"]), res["nr_iterations"])
    assert np.array_equal(np.array(a["T"], F).reshape(4, 4), res["T"])
