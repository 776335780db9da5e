"""The exhaustive members of the drop-in SCManager (go-rio_amd/host/scan_context/Scancontext.h) through
go-rio_amd/host/test/sc_exhaustive_sequence: what the driver prints equals what the Python binding returns for the same inputs, and
its --mine mode turns bestMatches into loop pairs verified by one batched APD-GICP alignment and fitness pass."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sc_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "sc_exhaustive_sequence")


def _write(path, scans, cands):
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(scans)))
        for xyz, inten in scans:
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, inten[:, None]], axis=1).astype(np.float32).tobytes())
        for c in cands:
            f.write(struct.pack("i", len(c)))
            f.write(np.asarray(c, np.int32).tobytes())


def _hex(v):
    return float.fromhex(v)


def test_exhaustive_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_exhaustive_sequence"])
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    path = str(tmp_path / "seq.bin")
    scans, _ = ss.loop_sequence(n_lap=6, n_points=200)
    _write(path, scans, ss.candidate_lists(len(scans)))
    for args in ([path], ["--mine", path]):
        r = subprocess.run([DRIVER] + args, capture_output=True, text=True)
        assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_exhaustive_driver_matches_python_binding(gpu, gorio, tmp_path):
    scans, _ = ss.loop_sequence(n_lap=16, seed=11, n_points=400)
    n = len(scans)
    cands = ss.candidate_lists(n)
    path = str(tmp_path / "seq.bin")
    _write(path, scans, cands)
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(rows) == n + 3
    sc = gorio.ScanContext()
    sc.add_scans(scans)
    want = sc.detect_exhaustive(list(range(n)), cands)
    for q, row in enumerate(rows[:n]):
        assert (row["q"], row["loop"]) == (q, want[q][0]), q
        assert np.float32(row["yaw"]) == want[q][1] and _hex(row["min_dist"]) == want[q][2], q
    assert sum(1 for w in want if w[0] >= 0) >= 3
    idx, dist, shift = sc.best_matches(None, 10)
    assert [[b[0], _hex(b[1]), b[2]] for b in rows[n]["best"]] == [[int(i), float(d), int(s)] for i, d, s in zip(idx, dist, shift)]
    d, s = sc.distance_pairs(np.arange(n), (7 * np.arange(n)) % n)
    assert [[_hex(p[0]), p[1]] for p in rows[n + 1]["pairs"]] == [[float(a), int(b)] for a, b in zip(d, s)]
    d, s = sc.distance_matrix(np.arange(9), n - 1 - np.arange(9))
    assert [_hex(v) for v in rows[n + 2]["matrix"]["dist"]] == d.reshape(-1).tolist() and rows[n + 2]["matrix"]["shift"] == s.reshape(-1).tolist()
    # --mine: the accepted best matches, each verified by the batched align and fitness
    r = subprocess.run([DRIVER, "--mine", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    mined = [json.loads(l) for l in r.stdout.splitlines()]
    expect = [q for q in range(n) if idx[q] >= 0 and dist[q] < 0.5]
    assert [m["q"] for m in mined] == expect and len(expect) >= 3
    unit = 113.0 / 20.0
    for m in mined:
        q = m["q"]
        assert m["loop"] == idx[q] and _hex(m["dist"]) == dist[q]
        assert np.float32(m["yaw"]) == np.float32(np.float64(np.float32(shift[q] * unit)) * np.pi / 180.0)
        assert np.isfinite(m["fitness"]) and m["accepted"] == int(bool(m["converged"]) and m["fitness"] <= 6.0)
