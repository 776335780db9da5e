"""The drop-in SCManager (go-rio_amd/host/scan_context/Scancontext.h) driven the way the back end drives it, through
go-rio_amd/host/test/sc_sequence: loop ids and yaw equal the Python binding's, every loop is verified by one batched APD-GICP
alignment and fitness pass against historyKeyframeFitnessScore = 6."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sc_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "sc_sequence")


def _write(path, scans, cands):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scans)))
        for xyz, inten in scans:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, inten[:, None]], axis=1).astype(np.float32).tobytes())
        for c in cands:
            f.write(struct.pack("i", len(c)))
            f.write(np.asarray(c, np.int32).tobytes())


def test_sc_driver_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_sequence"])
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    path = str(tmp_path / "seq.bin")
    scans, _ = ss.loop_sequence(n_lap=6, n_points=200)
    _write(path, scans, ss.candidate_lists(len(scans)))
    r = subprocess.run([DRIVER, path], capture_output=True, text=True)
    assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_sc_sequence_matches_python_binding(gpu, gorio, tmp_path):
    scans, _ = ss.loop_sequence(n_lap=80, n_points=2000)
    cands = ss.candidate_lists(len(scans))
    path = str(tmp_path / "seq.bin")
    _write(path, scans, cands)
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(rows) == len(scans)
    sc = gorio.ScanContext()
    sc.add_scans(scans)
    n_loop = n_acc = 0
    for q, row in enumerate(rows):
        lid, yaw, _, _ = sc.detect(q, cands[q])
        assert row["loop"] == lid, q
        assert np.float32(row["yaw"]) == yaw, q
        if lid >= 0:
            n_loop += 1
            assert np.isfinite(row["fitness"])
            assert row["accepted"] == int(bool(row["converged"]) and row["fitness"] <= 6.0)
            n_acc += row["accepted"]
    assert n_loop >= 5 and n_acc >= 1
