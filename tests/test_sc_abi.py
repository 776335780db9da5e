"""CPU-side checks of the Scan Context boundary (include/gorio_sc.h): the binding covers the header, the defaults are the launch
files', there is no CPU fallback, and the C++ drop-in and its driver build against the stand-ins.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "go-rio_amd", "host")


def _declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(gorio_[a-z0-9_]+)\s*\(", txt)))


def test_binding_covers_header(gorio):
    assert sorted(gorio.SC_SYMBOLS) == _declared("gorio_sc.h")
    lib = gorio.load_library()
    for name in gorio.SC_SYMBOLS:
        assert hasattr(lib, name)


def test_struct_layouts(gorio):
    S = gorio.scan_context
    assert C.sizeof(S.ScParams) == 16
    assert C.sizeof(S.ScDiag) == 96  # sizeof(gorio_sc_diag) on x86-64 and gfx950 hosts


def test_default_params_are_the_launch_files(gorio):
    p = gorio.scan_context.default_params()
    assert (p.sc_dist_thresh, p.azimuth_range) == (0.5, 56.5)


def test_no_cpu_fallback_without_device(gorio):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = gorio.load_library()
    h = C.c_void_p()
    p = gorio.scan_context.default_params()
    assert lib.gorio_sc_create(C.byref(h), 0, C.byref(p)) == -2  # GORIO_ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(gorio.GorioError):
        gorio.ScanContext()


def test_bad_params_refused_before_device(gorio):
    lib = gorio.load_library()
    h = C.c_void_p()
    p = gorio.scan_context.default_params()
    p.azimuth_range = 0.0
    assert lib.gorio_sc_create(C.byref(h), 0, C.byref(p)) == -1
    assert lib.gorio_sc_detect(None, 10, None, 0, None, None, None, None) == -1


def test_dropin_and_driver_build(gorio):
    gorio.build()
    subprocess.check_call(["make", "-C", HOST, "test/sc_sequence"])
    assert os.path.exists(os.path.join(HOST, "test", "sc_sequence"))
