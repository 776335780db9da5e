"""The C++ drop-in pclomp::GeneralizedIterativeClosestPoint (go-rio_amd/host/pclomp/gicp_omp.h) driven through a pcl::Registration base
pointer by go-rio_amd/host/test/gicp_omp_sequence.cpp: the factory's setter calls (registrations.cpp:93-99), then set target / set source
/ align as ndt_omp/apps/align.cpp does.  Its pose must equal the Python binding's bit for bit: both are the same library calls."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import gicp_omp_scenes as S

apd = importlib.import_module("go-rio_amd.apd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "gicp_omp_sequence")
# reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance, reg_correspondence_randomness, reg_max_optimizer_iterations
LAUNCH = dict(transformation_epsilon=0.01, max_iterations=64, corr=2.5, k=15, max_inner=10)


def _write(path, clouds):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(clouds)))
        for xyz in clouds:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, np.zeros((xyz.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


@pytest.mark.gpu
def test_cpp_sequence_equals_the_python_binding(gorio, gpu, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/gicp_omp_sequence"], stdout=subprocess.DEVNULL)
    sc = S.scenes()["general"]
    path = os.path.join(str(tmp_path), "frames.bin")
    _write(path, [sc["target"], sc["source"]])
    args = [DRIVER, path] + [repr(v) for v in (LAUNCH["transformation_epsilon"], LAUNCH["max_iterations"], LAUNCH["corr"], LAUNCH["k"], LAUNCH["max_inner"])]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    g = gorio.ApdGicp(device=gpu, k_correspondences=LAUNCH["k"], max_iterations=LAUNCH["max_iterations"], transformation_epsilon=LAUNCH["transformation_epsilon"],
                      rotation_epsilon=2e-3, corr_dist_threshold=LAUNCH["corr"])
    g.set_method(apd.METHOD_GICP_OMP)
    g.setGicpOmpParams(1e-3, LAUNCH["max_inner"])
    g.setInputTarget(sc["target"])
    g.setInputSource(sc["source"])
    want = g.align()
    diag = g.gicpOmpDiag()
    assert np.array_equal(np.array(out["T"], np.float32).reshape(4, 4), want["T"])
    assert (out["converged"], out["outer"], out["inner"], out["evaluations"]) == (int(want["converged"]), want["nr_iterations"], diag["inner_total"], diag["evaluations"])
    assert (out["k"], out["max_inner"], out["rotation_epsilon"]) == (LAUNCH["k"], LAUNCH["max_inner"], 2e-3)
    assert np.array_equal(np.array(out["aligned0"], np.float32), g.transformSource(want["T"])[0])
    maha = g.getMahalanobis() if g.gicpOmpUpdate(np.eye(4, dtype=np.float32)) else None  # the driver read mahalanobis(0) after its align
    assert maha is not None and out["m00"] > 0
    assert out["fitness"] == g.getFitnessScore(want["T"])[0]
    dt, dr = S.pose_error(S.reference("general")[1]["T"], want["T"])
    assert dt < 0.02 and dr < 0.01  # other launch parameters than the restatement's run: the same alignment, not the same bits
