"""The batch surface of the drop-in pclomp::NormalDistributionsTransform (go-rio_amd/host/pclomp/ndt_omp.h): setInputTargetShared,
alignBatch and getFitnessScoreBatch against the single members on equal inputs (host/test/ndt_batch.cpp), character for character, and
against the ctypes binding's poses bit for bit."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import ndt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "ndt_batch")


def _guesses(count):
    rng = np.random.default_rng(21)
    out = []
    for i in range(count):
        G = np.eye(4, dtype=np.float32)
        if i:
            a = np.deg2rad(rng.uniform(-1.0, 1.0))
            G[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            G[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        out.append(G)
    return out


def _cloud(f, c):
    f.write(struct.pack("i", c.shape[0]))
    f.write(np.concatenate([c, np.zeros((c.shape[0], 1), np.float32)], axis=1).astype(np.float32).tobytes())


def _write(path, target, sources, guesses):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(sources)))
        _cloud(f, target)
        for s, g in zip(sources, guesses):
            _cloud(f, s)
            f.write(np.ascontiguousarray(g, np.float32).tobytes())


def test_driver_builds(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/ndt_batch"])
    assert os.path.exists(DRIVER)


@pytest.mark.gpu
@pytest.mark.parametrize("search", ["DIRECT7", "DIRECT1"])
def test_batch_members_equal_single_members_and_the_binding(gpu, gorio, tmp_path, search):
    subprocess.check_call(["make", "-C", HOST, "test/ndt_batch"])
    src, tgt, _ = S.real_pair()
    sources = [src[0::3], src[1::3][:777], src[2::3][:257]]
    guesses = _guesses(3)
    path = str(tmp_path / "candidates.bin")
    _write(path, tgt, sources, guesses)
    r = subprocess.run([DRIVER, path, "1.0", search], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    single = [x for x in lines if '"mode": "single"' in x]
    batch = [x for x in lines if '"mode": "batch"' in x]
    assert len(single) == 3 and len(batch) == 3
    for a, b in zip(single, batch):
        assert a.replace('"mode": "single"', '"mode": "batch"') == b  # character for character
    last = json.loads(lines[-1])
    assert last == {"mismatch_error": "runtime_error", "names_resolution": 1, "unchanged": 1}
    for k, line in enumerate(batch):
        out = json.loads(line)
        n = gorio.Ndt(device=gpu, resolution=1.0, transformation_epsilon=0.01, max_iterations=64, search=getattr(gorio.ndt, search))
        n.set_target(tgt)
        n.set_source(sources[k])
        res = n.align(guesses[k])
        n.close()
        assert np.array_equal(np.array(out["T"], np.float32).reshape(4, 4), res["T"])  # bit for bit
        assert bool(out["converged"]) == res["converged"] and out["iterations"] == res["nr_iterations"]
        assert out["n_derivatives"] == res["n_derivatives"] and out["n_hessians"] == res["n_hessians"] and out["n_mt"] == res["n_mt"]
        assert out["probability"] == res["trans_probability"] and out["score"] == res["score"]
        assert 0 < out["fitness"] < 1e6
