"""CPU-side checks of the batched FastGICPMultiPoints entries of include/gorio_apd.h: exported, bound, declared as documented, the
header text says which batch call serves the method, and the argument rules that need no device.  No GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
SIGNATURES = [
    "int gorio_apd_gicp_mp_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations);",
    "int gorio_apd_gicp_mp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches, int* syncs, int* max_round_launches);",
    "int gorio_apd_gicp_mp_last_hessian(const gorio_apd_t* h, double* H36);",
]


def test_symbols_exported_bound_and_declared(gorio):
    lib = gorio.load_library()
    text = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", open(os.path.join(ROOT, "include", "gorio_apd.h")).read()))  # comments as running text
    for sig in SIGNATURES:
        name = re.search(r"(gorio_[a-z0-9_]+)\(", sig).group(1)
        assert hasattr(lib, name) and name in gorio.apd.APD_SYMBOLS and sig in text, name
    assert callable(gorio.gicp_mp_align_batch) and gorio.gicp_mp_align_batch is gorio.apd.gicp_mp_align_batch
    assert gorio.gicp_mp_align_batch([]) == []  # an empty batch makes no call
    for word in ("the batched form of this method is gorio_apd_gicp_mp_align_batch", "two synchronisations per round", "bit for bit those of its own gorio_apd_align",
                 "handle <q>", "ends alone", "MAY differ"):
        assert word in text, word
    machine = open(os.path.join(ROOT, "go-rio_amd", "csrc", "gicp_mp_machine.h")).read()
    assert "hip" not in machine.replace("apd_gicp_mp.hip", "").replace("apd_kernels.hip", "").lower().replace("nothing here knows about hip", "")  # host only


def test_arguments_refused_without_a_device(gorio):
    lib = gorio.load_library()
    fn = lib.gorio_apd_gicp_mp_align_batch
    g = (C.c_float * 32)()
    T = (C.c_float * 32)()
    hs = (C.c_void_p * 2)(None, None)
    assert fn(None, 0, None, None, None, None) == 0  # count == 0 touches nothing
    assert fn(hs, -1, g, T, None, None) == INVALID
    assert fn(None, 2, g, T, None, None) == INVALID and fn(hs, 2, None, T, None, None) == INVALID and fn(hs, 2, g, None, None, None) == INVALID
    assert fn(hs, 2, g, T, None, None) == INVALID  # null entries
    assert lib.gorio_apd_gicp_mp_batch_diag(None, None, None, None, None) == INVALID
    assert lib.gorio_apd_gicp_mp_last_hessian(None, None) == INVALID
