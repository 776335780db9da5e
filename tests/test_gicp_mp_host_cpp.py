"""The C++ drop-in fast_gicp::FastGICPMultiPoints (go-rio_amd/host/fast_gicp/gicp/experimental/fast_gicp_mp.hpp) driven through a pcl::Registration
base pointer by go-rio_amd/host/test/gicp_mp_sequence.cpp in the odometry nodelet's call order, each align seeded with the previous
transformation.  Its poses equal the ctypes binding's of the same ABI bit for bit; its constructor defaults are those of
fast_gicp_mp_impl.hpp:20-36."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import gicp_mp_restatement as R
import icp_scenes as S

apd = importlib.import_module("go-rio_amd.apd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "gicp_mp_sequence")
SOURCES = [257, 513, 256]


def frames():
    return [S.target(2000)] + [S.source(n, 2000) for n in SOURCES]


def _write(path, clouds):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(clouds)))
        for xyz in clouds:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def test_driver_builds_and_header_carries_the_surface(gorio):
    subprocess.check_call(["make", "-C", HOST, "test/gicp_mp_sequence"], stdout=subprocess.DEVNULL)
    assert os.path.exists(DRIVER)
    text = open(os.path.join(HOST, "fast_gicp", "gicp", "experimental", "fast_gicp_mp.hpp")).read()
    for member in ("class FastGICPMultiPoints : public pcl::Registration<PointSource, PointTarget, float>", "void setNumThreads(int) {}", "void setRotationEpsilon(double eps)",
                   "void setCorrespondenceRandomness(int k)", "void setRegularizationMethod(RegularizationMethod method)",
                   "virtual void setInputSource(const PointCloudSourceConstPtr& cloud) override", "virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override",
                   "virtual void computeTransformation(PointCloudSource& output, const Matrix4& guess) override", "ADDITION", "void setNeighborSearchRadius(double radius)",
                   "setInputTargetShared(", "setInputSourceFromScan(", "setInputTargetFromScan(", "setInputSourceKeyframe(", "setInputTargetKeyframe("):
        assert member in text, member


@pytest.mark.gpu
def test_class_through_base_pointer_matches_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/gicp_mp_sequence"], stdout=subprocess.DEVNULL)
    path = os.path.join(str(tmp_path), "frames.bin")
    fr = frames()
    _write(path, fr)
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["defaults"] == dict(k_correspondences=20, max_iterations=64, rotation_epsilon=1e-5, transformation_epsilon=1e-5, regularization=R.PLANE, corr_dist_is_float_max=1,
                                   neighbor_search_radius=0.5)  # fast_gicp_mp_impl.hpp:20-36

    def new(**over):
        p = dict(R.DEFAULTS)
        p.update(over)
        g = gorio.ApdGicp()
        g.set_params(k_correspondences=p["k_correspondences"], regularization=p["regularization"], max_iterations=p["max_iterations"], rotation_epsilon=p["rotation_epsilon"],
                     transformation_epsilon=p["transformation_epsilon"])
        g.set_gicp_mp_params(p["neighbor_search_radius"])
        g.set_method(apd.METHOD_GICP_MP)
        return g

    def same(got, g, res, src):
        T = np.array(got["T"], np.float32).reshape(4, 4)
        assert T.tobytes() == res["T"].tobytes() and bool(got["converged"]) == res["converged"] and got["iterations"] == res["nr_iterations"] and got["passes"] == res["n_linearize"]
        d = g.gicp_mp_diag()
        assert (got["used"], got["neighbours"]) == (d["used"], d["total"])
        assert got["fitness"] == pytest.approx(g.getFitnessScore(res["T"])[0], rel=1e-12)
        assert np.array_equal(np.array(got["aligned0"], np.float32), R.transform_points_f32(T, src[:1])[0])

    assert len(out["aligns"]) == len(SOURCES)
    g = new()
    g.setInputTarget(fr[0])
    prev = np.eye(4, dtype=np.float32)
    for k in range(1, len(fr)):
        g.setInputSource(fr[k])
        res = g.align(prev)
        same(out["aligns"][k - 1], g, res, fr[k])
        assert res["converged"]
        prev = res["T"]
    g.setInputSource(fr[1])
    same(out["shared"], g, g.align(), fr[1])
    v = new(neighbor_search_radius=0.25, regularization=R.FROBENIUS, k_correspondences=12, rotation_epsilon=1e-4, transformation_epsilon=1e-4)
    v.setInputTarget(fr[0])
    v.setInputSource(fr[1])
    same(out["variant"], v, v.align(), fr[1])
    assert out["variant"]["T"] != out["shared"]["T"]
