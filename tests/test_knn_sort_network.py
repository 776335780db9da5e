"""CPU test of the comparator network knn_collect_kernel<20> sorts its buffered keys with (go-rio_amd/csrc/knn_sort_network.h), through the
stand-alone driver go-rio_amd/host/test/knn_sort_network.cpp, which includes the header the device code includes and links nothing of HIP
or the library.  The driver checks the network by the 0/1 principle over all 2^24 inputs (64 per machine word) and checks padded inputs
of 0 .. 24 real keys against std::sort.  It is built twice, plain and with -fsanitize=address,undefined; both binaries are run directly,
must print the same and stay silent on stderr."""
import json
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
NAMES = ("knn_sort_network", "knn_sort_network_san")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", HOST] + ["test/" + n for n in NAMES], stdout=subprocess.DEVNULL)
    out = {}
    for name in NAMES:
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stdout[-2000:], r.stderr[-2000:])
        out[name] = r.stdout
    return out


def test_sanitized_build_prints_the_same(outputs):
    assert outputs["knn_sort_network"] == outputs["knn_sort_network_san"] and outputs["knn_sort_network"].count("\n") == 1


def test_network_sorts_every_zero_one_input(outputs):
    r = json.loads(outputs["knn_sort_network"])
    assert (r["width"], r["keep"]) == (24, 20)  # CAP and K of knn_collect_kernel<20>
    assert r["zero_one_inputs"] == 2**24 and r["zero_one_failures"] == 0


def test_padded_keys_come_out_as_std_sort_leaves_them(outputs):
    r = json.loads(outputs["knn_sort_network"])
    assert r["padded_cases"] >= 25 * 1000 and r["padded_failures"] == 0  # every cnt = 0 .. 24


def test_network_is_smaller_than_the_insertion_it_replaces(outputs):
    """20 rounds of a 20-slot insertion are 400 compare-exchanges; the network is there to do less."""
    assert json.loads(outputs["knn_sort_network"])["comparators"] <= 130
