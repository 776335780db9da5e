"""The cross-database members of the drop-in SCManager (go-rio_amd/host/scan_context/Scancontext.h) through
go-rio_amd/host/test/sc_cross_sequence: two SCManagers filled from the two laps of a loop sequence, what the driver prints equals what
the Python binding returns for the same two databases (index and shift equal, distances the same bits), and its --mine mode turns the
top lists into loop pairs verified by one batched APD-GICP alignment and one fitness pass."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import sc_scenes as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "sc_cross_sequence")


def _write(path, first, second):
    with open(path, "wb") as f:
        f.write(struct.pack("ii", len(first), len(second)))
        for xyz, inten in list(first) + list(second):
            f.write(struct.pack("i", xyz.shape[0]))
            f.write(np.concatenate([xyz, inten[:, None]], axis=1).astype(np.float32).tobytes())


def _hex(v):
    return float.fromhex(v)


def _rows(lists):
    return [[[b[0], _hex(b[1]), b[2]] for b in l] for l in lists]


def _used(idx, dist, shift):
    """The binding's [n, k] arrays as the driver's lists: unused slots dropped."""
    return [[[int(i), float(d), int(s)] for i, d, s in zip(ri, rd, rs) if i >= 0] for ri, rd, rs in zip(idx, dist, shift)]


def test_cross_driver_builds_and_refuses_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_cross_sequence"])
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    path = str(tmp_path / "sessions.bin")
    scans, _ = ss.loop_sequence(n_lap=6, n_points=200)
    _write(path, scans[:6], scans[6:])
    for args in ([path], ["--mine", path]):
        r = subprocess.run([DRIVER] + args, capture_output=True, text=True)
        assert r.returncode == 3 and "no usable HIP device" in r.stderr  # no CPU fallback


@pytest.mark.gpu
def test_cross_driver_matches_python_binding(gpu, gorio, tmp_path):
    scans, _ = ss.loop_sequence(n_lap=16, seed=11, n_points=400)
    first, second = scans[:16], scans[16:]
    n1, n2 = len(first), len(second)
    path = str(tmp_path / "sessions.bin")
    _write(path, first, second)
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(rows) == n2 + 4
    old, new = gorio.ScanContext(), gorio.ScanContext()
    old.add_scans(first), new.add_scans(second)
    idx, dist, shift = new.top_matches(old, None, None, 3)
    want = _used(idx, dist, shift)
    for q, row in enumerate(rows[:n2]):
        assert row["q"] == q and _rows([row["top"]])[0] == want[q], q
    assert all(len(w) == 3 for w in want)
    d, s = new.cross_distance_pairs(old, np.arange(n2), (5 * np.arange(n2)) % n1)
    assert [[_hex(p[0]), p[1]] for p in rows[n2]["pairs"]] == [[float(a), int(b)] for a, b in zip(d, s)]
    d, s = new.cross_distance_matrix(old, np.arange(9), n1 - 1 - np.arange(9))
    assert [_hex(v) for v in rows[n2 + 1]["matrix"]["dist"]] == d.reshape(-1).tolist() and rows[n2 + 1]["matrix"]["shift"] == s.reshape(-1).tolist()
    backwards = np.arange(n1 - 1, -1, -1)
    det = new.cross_detect(old, list(range(n2)), [backwards] * n2)
    for q, got in enumerate(rows[n2 + 2]["detect"]):
        assert got[0] == det[q][0] and np.float32(got[1]) == det[q][1] and _hex(got[2]) == det[q][2], q
        assert det[q][2] == dist[q, 0]  # the minimum over all of session 1 is the first of the top list
    tri = old.top_matches(None, None, np.maximum(0, np.arange(n1) - 10 + 1), 2)
    assert _rows(rows[n2 + 3]["triangle"]) == _used(*tri)
    # --mine: every entry of the top lists below the threshold, each verified by the batched align and fitness
    r = subprocess.run([DRIVER, "--mine", path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    mined = [json.loads(l) for l in r.stdout.splitlines()]
    expect = [(q, j) for q in range(n2) for j in range(3) if idx[q, j] >= 0 and dist[q, j] < 0.5]
    assert [(m["q"], m["rank"]) for m in mined] == expect and len(expect) >= 3
    unit = 113.0 / 20.0
    for m in mined:
        q, j = m["q"], m["rank"]
        assert m["loop"] == idx[q, j] and _hex(m["dist"]) == dist[q, j]
        assert np.float32(m["yaw"]) == np.float32(np.float64(np.float32(shift[q, j] * unit)) * np.pi / 180.0)
        assert np.isfinite(m["fitness"]) and m["accepted"] == int(bool(m["converged"]) and m["fitness"] <= 6.0)
    old.close(), new.close()
