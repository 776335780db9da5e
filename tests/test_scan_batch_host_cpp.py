"""gorio::ScanPreprocessor::processBatch (go-rio_amd/host/radar_preprocessing/scan_preprocessor.hpp) through
go-rio_amd/host/test/preprocess_batch: four packed messages through one processBatch call and the same four through process_packed with an
equally seeded generator; the driver prints the sha256 of every output cloud and the two lists must be equal."""
import os
import subprocess

import pytest

import scan_pipeline_restatement as sr
from test_scan_host_cpp import _write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")
DRIVER = os.path.join(HOST, "test", "preprocess_batch")


def test_preprocess_batch_driver_builds(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/preprocess_batch"])
    assert os.path.exists(DRIVER)


@pytest.mark.gpu
def test_process_batch_equals_process_packed_one_after_another(gpu, gorio, tmp_path):
    subprocess.check_call(["make", "-C", HOST, "test/preprocess_batch"])
    rot = sr.tilt()
    scans = [sr.raw_scan(seed, n_ground=sr.SEQUENCE_N_GROUND, rotation=rot) for seed in sr.SEQUENCE_SEEDS[:4]]
    path = str(tmp_path / "scans.bin")
    _write(path, scans, rot, False, sr.OUTLIER_STATISTICAL, sr.CHAIN_ANG_VEL, 4242)
    r = subprocess.run([DRIVER, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln.split(" ", 7) for ln in r.stdout.splitlines()]
    a = [ln[1:] for ln in lines if ln[0] == "A"]
    b = [ln[1:] for ln in lines if ln[0] == "B"]
    assert len(a) == len(b) == 8 and a == b  # two frames of four messages: status, counts, sha256 and text
    assert all(x[2] == "0" and len(x[5]) == 64 and int(x[3]) > 0 and int(x[4]) >= 1 for x in a), a  # every frame OK, a digest each, last_scan() the cloud
    for frame in ("0", "1"):  # four different clouds per call: one member's answer cannot pass for another's
        assert len({x[5] for x in a if x[0] == frame}) == 4
