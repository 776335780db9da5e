"""The drop-in gorio::NormalDistributionsTransform (go-rio_amd/host/gorio/ndt.hpp: pcl::NormalDistributionsTransform, the radius
neighbourhood) built by the factory's setter calls for plain "NDT" (registrations.cpp:111-115) and driven through a pcl::Registration
base pointer in the nodelets' call order (host/test/ndt_pcl_sequence.cpp): the pose equals the ctypes binding's bit for bit.  The pclomp
drop-in keeps refusing KDTREE.  Without a GPU the constructor throws."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import ndt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "ndt_pcl_sequence")
OMP_DRIVER = os.path.join(HOST, "test", "ndt_sequence")


def _write(path, target, source):
    with open(path, "wb") as f:
        f.write(struct.pack("i", 2))
        for c in (target, source):
            f.write(struct.pack("i", c.shape[0]))
            f.write(np.concatenate([c, np.zeros((c.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def test_class_has_the_pcl_surface_and_the_driver_builds(gorio):
    txt = open(os.path.join(HOST, "gorio", "ndt.hpp")).read()
    for member in ("class NormalDistributionsTransform : public pclomp::NormalDistributionsTransform<PointSource, PointTarget>", "gorio_ndt_set_radius_search(this->handle(), 1)",
                   "double getOulierRatio() const", "void setOulierRatio(double outlier_ratio)", "static void alignBatch(", "static std::vector<double> calculateScoreBatch("):
        assert member in txt, member
    base = open(os.path.join(HOST, "pclomp", "ndt_omp.h")).read()
    for member in ("void setResolution(float resolution)", "float getResolution() const", "void setStepSize(double step_size)", "double getStepSize() const",
                   "double getTransformationProbability() const", "int getFinalNumIteration() const", "void setInputTargetShared(", "void setInputSourceFromScan(",
                   "void setInputTargetFromScan(", "setInputTargetSubmap("):
        assert member in base, member
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/ndt_pcl_sequence"])
    assert os.path.exists(DRIVER)


@pytest.mark.gpu
def test_sequence_matches_python_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_pcl_sequence"])
    src, tgt, _ = S.real_pair()
    path = str(tmp_path / "pair.bin")
    _write(path, tgt, src)
    r = subprocess.run([DRIVER, path, "1.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    n = gorio.Ndt(device=gpu, radius_search=True, resolution=1.0, transformation_epsilon=0.01, max_iterations=64)
    n.set_target(tgt)
    n.set_source(src)
    res = n.align()
    assert np.array_equal(np.array(out["T"], np.float32).reshape(4, 4), res["T"])  # bit for bit
    assert bool(out["converged"]) == res["converged"] and out["iterations"] == res["nr_iterations"]
    assert out["n_derivatives"] == res["n_derivatives"] and out["n_mt"] == res["n_mt"]
    assert out["probability"] == res["trans_probability"]
    assert out["score_aligned"] == pytest.approx(n.calculate_score(res["T"]), rel=1e-12)
    n.set_radius_search(False)  # and it is not the DIRECT7 pose
    assert not np.array_equal(n.align()["T"], res["T"])
    n.close()


@pytest.mark.gpu
def test_pclomp_dropin_still_refuses_kdtree(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_sequence"])
    src, tgt, _ = S.real_pair()
    path = str(tmp_path / "pair.bin")
    _write(path, tgt[:500], src[:500])
    r = subprocess.run([OMP_DRIVER, path, "1.0", "KDTREE"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "KDTREE" in r.stderr
