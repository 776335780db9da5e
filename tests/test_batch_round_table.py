"""CPU test of the round table of the lock-step batched aligns (go-rio_amd/csrc/batch_rounds.h) through its stand-alone driver
go-rio_amd/host/test/batch_round_table.cpp, which links nothing of HIP or the library.  The driver is built twice, plain and with
-fsanitize=address,undefined; both binaries must print the same and stay silent on stderr.  Every number is recomputed here from the
rules the header states: a job has nblk = ceil(n / 256) blocks that own a partial slot and nwg = ceil(max(n, index padding) / 256)
workgroups, first is the prefix sum of nwg, the first list holds (k, 0) .. (k, nwg[k] - 1) job after job, the second list behind it the
nblk blocks of the marked jobs, the trailing class starts at the sum of the leading nwg, and the table of any round fits the bytes
reserved for the round with every handle pending."""
import json
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
LAYOUTS = ["block_edges", "padding_blocks", "second_list", "second_list_subset", "two_classes", "all_trailing", "one_job", "no_job"]
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def rows():
    subprocess.check_call(["make", "-C", HOST, "test/batch_round_table", "test/batch_round_table_san"], stdout=subprocess.DEVNULL)
    out = {}
    for name in ("batch_round_table", "batch_round_table_san"):
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["batch_round_table"] == out["batch_round_table_san"]
    return {r["case"]: r for r in map(json.loads, out["batch_round_table"].strip().splitlines())}


def _ceil(a, b):
    return (a + b - 1) // b


@pytest.mark.parametrize("name", LAYOUTS)
def test_layout(rows, name):
    r = rows[name]
    njobs = len(r["n"])
    nblk = [_ceil(n, 256) for n in r["n"]]
    nwg = [_ceil(max(n, p), 256) for n, p in zip(r["n"], r["spad"])]
    first = [sum(nwg[:k]) for k in range(njobs)]
    assert r["njobs"] == njobs and r["nblk"] == nblk and r["nwg"] == nwg and r["first"] == first
    first_list = [(k, b) for k in range(njobs) for b in range(nwg[k])]
    second = [(k, b) for k in range(njobs) if r["marked"][k] for b in range(nblk[k])]
    refs = list(zip(r["ref_job"], r["ref_blk"]))
    assert r["wg"] == sum(nwg) and r["second"] == len(second)
    assert refs[: r["wg"]] == first_list and refs[r["wg"]:] == second  # the second list starts where the first ends
    lead = min(r["n_leading_in"], njobs)
    assert r["n_leading"] == lead and r["lead_wg"] == sum(nwg[:lead])
    assert refs[r["lead_wg"]: r["wg"]] == [(k, b) for k in range(lead, njobs) for b in range(nwg[k])]
    for job, blk in refs:  # what the kernels rely on
        assert 0 <= job < njobs and 0 <= blk < nwg[job]
    for job, blk in refs[r["wg"]:]:
        assert blk < nblk[job]
    total_wg = sum(_ceil(max(n, p), 256) for n, p in zip(r["all_n"], r["all_spad"]))
    reserved = r["job_size"] * len(r["all_n"]) + 8 * total_wg * (2 if r["second_list"] else 1)
    assert r["bytes"] == r["job_size"] * njobs + 8 * len(refs)
    assert r["reserved"] == reserved and r["bytes"] <= reserved and r["grown"] == reserved + reserved // 4


def test_named_edges(rows):
    e = rows["block_edges"]
    assert e["n"] == [1, 255, 256, 257] and e["nblk"] == [1, 1, 1, 2] and e["first"] == [0, 1, 2, 3] and e["wg"] == 5 and e["second"] == 0
    p = rows["padding_blocks"]
    assert (p["n"][0], p["spad"][0], p["nblk"][0], p["nwg"][0]) == (3, 512, 1, 2) and p["first"] == [0, 2, 4]
    s = rows["second_list"]
    assert s["marked"] == [1, 0, 1, 0] and s["wg"] == 2 + 4 + 2 + 2
    assert list(zip(s["ref_job"], s["ref_blk"]))[s["wg"]:] == [(0, 0), (0, 1), (2, 0)]
    t = rows["two_classes"]
    assert t["n_leading"] == 2 and t["n"] == [1, 256, 257, 513, 1000] and t["lead_wg"] == 2 and t["first"][2] == 2 and t["wg"] == 2 + 2 + 3 + 4
    assert rows["all_trailing"]["lead_wg"] == 0 and rows["all_trailing"]["wg"] == 3
    assert rows["one_job"]["first"] == [0] and rows["one_job"]["wg"] == 1 and rows["one_job"]["lead_wg"] == 1
    z = rows["no_job"]
    assert z["njobs"] == 0 and z["first"] == [] and z["ref_job"] == [] and z["wg"] == z["second"] == z["lead_wg"] == z["bytes"] == 0


@pytest.mark.parametrize("divisor", [16, 32])
def test_overflow_refusal(rows, divisor):
    r = rows["overflow_%d" % divisor]
    assert r["divisor"] == divisor and r["cap"] == INT_MAX // divisor
    assert (r["below"], r["at_cap"], r["above"], r["far_above"]) == (0, 0, 1, 1)  # fires at the first total above the cap, not at the cap
