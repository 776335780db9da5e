"""The batch surface of the drop-in pclomp::GeneralizedIterativeClosestPoint (go-rio_amd/host/pclomp/gicp_omp.h): setInputTargetShared,
alignBatch and getFitnessScoreBatch against the single members on equal inputs, in the loop-closure order (host/test/gicp_omp_batch.cpp:
one target, N candidate sources, a fitness score each, the best candidate).  The driver prints every float in hex: the batched lines must
equal the one-by-one lines character for character, and the binding's gicp_omp_align_batch on the same clouds bit for bit."""
import importlib
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import gicp_omp_batch_scenes as B

apd = importlib.import_module("go-rio_amd.apd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "gicp_omp_batch")
# reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance, reg_correspondence_randomness, reg_max_optimizer_iterations
LAUNCH = dict(transformation_epsilon=0.01, max_iterations=64, corr=0.5, k=20, max_inner=10)


def _cloud(f, c):
    f.write(struct.pack("i", c.shape[0]))
    f.write(np.concatenate([c, np.zeros((c.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def _floats(text):
    return np.array([float.fromhex(t) for t in text.split()])


def test_driver_builds(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/gicp_omp_batch"], stdout=subprocess.DEVNULL)
    assert os.path.exists(DRIVER)


@pytest.mark.gpu
def test_batch_members_equal_single_members_and_the_binding(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/gicp_omp_batch"], stdout=subprocess.DEVNULL)
    scenes = B.loop_closure()[1:4]  # 257, 512 and 513 points on one target
    path = str(tmp_path / "candidates.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scenes)))
        _cloud(f, scenes[0][1]["target"])
        for _, sc in scenes:
            _cloud(f, sc["source"])
            f.write(np.ascontiguousarray(sc["guess"], np.float32).tobytes())
    args = [DRIVER, path] + [repr(v) for v in (LAUNCH["transformation_epsilon"], LAUNCH["max_iterations"], LAUNCH["corr"], LAUNCH["k"], LAUNCH["max_inner"])]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    single = [x for x in lines if '"mode": "single"' in x]
    batch = [x for x in lines if '"mode": "batch"' in x]
    assert len(single) == len(batch) == len(scenes)
    for a, b in zip(single, batch):
        assert a.replace('"mode": "single"', '"mode": "batch"') == b  # hex floats: bit for bit
    last = json.loads(lines[-1])
    assert last["bit_identical"] == 1 and last["best_single"] == last["best_batch"] >= 0
    outs = [json.loads(x) for x in batch]
    assert last["rounds"] == max(o["evaluations"] + o["outer"] + (0 if o["converged"] else 1) for o in outs) and last["launches"] <= 4 * last["rounds"] + len(scenes)
    # the binding on the same clouds: the same library calls
    objs = []
    for k, (_, sc) in enumerate(scenes):
        g = gorio.ApdGicp(device=gpu, k_correspondences=LAUNCH["k"], max_iterations=LAUNCH["max_iterations"], transformation_epsilon=LAUNCH["transformation_epsilon"],
                          rotation_epsilon=2e-3, corr_dist_threshold=LAUNCH["corr"])
        g.set_method(apd.METHOD_GICP_OMP)
        g.setGicpOmpParams(1e-3, LAUNCH["max_inner"])
        if k == 0:
            g.setInputTarget(sc["target"])
        else:
            g.setInputTargetShared(objs[0])
        g.setInputSource(sc["source"])
        objs.append(g)
    res = gorio.gicp_omp_align_batch(objs, np.stack([sc["guess"] for _, sc in scenes]))
    diags = [g.gicpOmpDiag() for g in objs]
    scores, _ = gorio.fitness_score_batch(objs)
    for o, want, d, g, score in zip(outs, res, diags, objs, scores):
        assert np.array_equal(_floats(o["T"]).astype(np.float32).reshape(4, 4), want["T"])
        assert (o["converged"], o["outer"], o["inner"], o["evaluations"]) == (int(want["converged"]), want["nr_iterations"], d["inner_total"], d["evaluations"])
        assert np.array_equal(_floats(o["aligned0"]).astype(np.float32), g.transformSource(want["T"])[0])
        assert float.fromhex(o["fitness"]) == score
    assert res[0]["batch_diag"] == dict(rounds=last["rounds"], launches=last["launches"])
