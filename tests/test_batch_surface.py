"""Batch surface of the library without a GPU: the batched fitness entry point is exported and declared, and the two C++ drivers of the
batch members (FastAPDGICP::alignBatch / getFitnessScoreBatch / getInlierFractionBatch, VelPreintegration::batch) build and refuse
cleanly when no HIP device is usable."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

synth = importlib.import_module("go-rio_amd.synth")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
LOOP_DRIVER = os.path.join(HOST, "test", "loop_closure_batch")
PREINT_DRIVER = os.path.join(HOST, "test", "preint_batch")


def test_fitness_score_batch_is_exported_and_declared(gorio):
    gorio.build()
    lib = gorio.load_library()
    assert hasattr(lib, "gorio_apd_fitness_score_batch")
    from importlib import import_module

    assert "gorio_apd_fitness_score_batch" in import_module("go-rio_amd.apd").APD_SYMBOLS
    with open(os.path.join(ROOT, "include", "gorio_apd.h")) as f:
        header = f.read()
    assert re.search(r"int\s+gorio_apd_fitness_score_batch\s*\(\s*gorio_apd_t\s*\*\*\s*handles\s*,\s*int\s+count\s*,\s*const\s+float\s*\*\s*T\s*,\s*double\s+max_range\s*,"
                     r"\s*double\s+inlier_dist\s*,\s*double\s*\*\s*score\s*,\s*double\s*\*\s*inlier_fraction\s*\)\s*;", header)


def test_fitness_score_batch_empty_and_bad_arguments(gorio):
    """count == 0 is a no-op that succeeds (no device is touched); a null handle array with count > 0 is GORIO_ERR_INVALID."""
    lib = gorio.load_library()
    score = (C.c_double * 1)()
    T = (C.c_float * 16)()
    assert lib.gorio_apd_fitness_score_batch(None, 0, None, C.c_double(1.0), C.c_double(0.0), None, None) == 0
    assert lib.gorio_apd_fitness_score_batch(None, 1, T, C.c_double(1.0), C.c_double(0.0), score, None) == -1
    s, f = gorio.fitness_score_batch([])
    assert s.shape == (0,) and f.shape == (0,)


def _loop_file(path, n_cand=2, n=200):
    tx, tl = synth.radar_scan(n, seed=1)
    with open(path, "wb") as f:
        f.write(struct.pack("<ii", n_cand, n))
        f.write(np.concatenate([tx, tl[:, None]], axis=1).astype(np.float32).tobytes())
        for k in range(n_cand):
            sx, sl = synth.radar_scan(n, seed=10 + k)
            f.write(struct.pack("<i", n))
            f.write(np.concatenate([sx, sl[:, None]], axis=1).astype(np.float32).tobytes())
            f.write(np.eye(4, dtype=np.float32).tobytes())
    return path


def _preint_file(path):
    win = synth.imu_window(seed=1)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", 1))
        for t, d in ((win["gyr_t"], win["gyr"]), (win["vel_t"], win["vel"])):
            f.write(struct.pack("<i", len(t)))
            f.write(np.concatenate([np.asarray(t)[:, None], d], axis=1).astype(np.float64).tobytes())
        f.write(struct.pack("<didi", win["start_t"], 1, -1.0, 1))
        f.write(struct.pack("<id", 1, win["end_t"]))
    return path


def test_batch_drivers_build_and_refuse_without_gpu(gorio, tmp_path):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    assert os.path.exists(LOOP_DRIVER) and os.path.exists(PREINT_DRIVER)
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present (tests/test_batch_surface_gpu.py runs the drivers)")
    for cmd in ([LOOP_DRIVER, _loop_file(str(tmp_path / "loop.bin"))], [PREINT_DRIVER, _preint_file(str(tmp_path / "imu.bin"))],
                [PREINT_DRIVER, _preint_file(str(tmp_path / "imu.bin")), "errors"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 3 and "no usable HIP device" in r.stderr, (cmd, r.returncode, r.stderr)  # no CPU fallback
