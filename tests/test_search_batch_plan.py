"""CPU test of the host-side planning of a BATCH of radius queries (go-rio_amd/csrc/search_plan.h) through its stand-alone driver
go-rio_amd/host/test/search_batch_plan.cpp, which links nothing of HIP or the library.  The driver is built twice, plain and with
-fsanitize=address,undefined; both binaries must print the same and stay silent on stderr.  Every number is recomputed here from the
rules the header states: a job takes ceil(nq / 64) waves and nq segment-sort workgroups, its nq + 1 found offsets follow the earlier
jobs', a job with cross queries owns one key segment of the power of two >= nq (at least 4096), and the merged long-segment table is the
jobs' own tables one after the other with the slots moved behind the earlier jobs' slots."""
import json
import os
import subprocess

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
TILE = 4096


@pytest.fixture(scope="module")
def rows():
    subprocess.check_call(["make", "-C", HOST, "test/search_batch_plan", "test/search_batch_plan_san"], stdout=subprocess.DEVNULL)
    out = {}
    for name in ("search_batch_plan", "search_batch_plan_san"):
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["search_batch_plan"] == out["search_batch_plan_san"]
    return {r["case"]: r for r in map(json.loads, out["search_batch_plan"].strip().splitlines())}


def _pow2(n):
    p = TILE
    while p < n:
        p *= 2
    return p


def test_layouts(rows):
    names = ["wave_edges", "all_empty", "no_job", "empty_between", "one"]
    for name in names:
        r = rows[name]
        nq = [q if a else 0 for q, a in zip(r["nq"], r["active"])]
        waves = [(q + 63) // 64 for q in nq]
        assert r["ok"] == 1
        assert r["wave_first"] == np.concatenate([[0], np.cumsum(waves)]).astype(int).tolist()
        assert r["query_first"] == np.concatenate([[0], np.cumsum(nq)]).astype(int).tolist()
        assert r["offs_first"] == np.concatenate([[0], np.cumsum([q + 1 if q else 0 for q in nq])]).astype(int).tolist()
        assert r["wave_job"] == [j for j, w in enumerate(waves) for _ in range(w)] == r["owner_of_wave"]
        assert r["wave_in_job"] == [k for w in waves for k in range(w)]
        assert r["owner_of_query"] == [j for j, q in enumerate(nq) for _ in range(q)]
        keyed = [j for j, (q, s) in enumerate(zip(nq, r["self"])) if q and not s]
        assert r["key_jobs"] == keyed and r["key_seg"] == [keyed.index(j) if j in keyed else -1 for j in range(len(nq))]
        blocks = [_pow2(nq[j]) // 256 for j in keyed]
        assert r["key_first"] == np.concatenate([[0], np.cumsum(blocks)]).astype(int).tolist() and r["key_items"] == sum(blocks)
        assert r["max_key_pow2"] == max([_pow2(nq[j]) for j in keyed], default=0)
    e = rows["wave_edges"]
    assert e["nq"] == [0, 1, 63, 64, 65] and e["wave_first"] == [0, 0, 1, 2, 3, 5] and e["key_jobs"] == [1, 2, 4]
    assert rows["all_empty"]["wave_job"] == [] and rows["all_empty"]["query_first"] == [0, 0, 0, 0] and rows["all_empty"]["max_key_pow2"] == 0
    assert rows["empty_between"]["max_key_pow2"] == 8192


def test_merged_long_segments(rows):
    for name in ("two_long_jobs", "two_long_jobs_cut", "no_long"):
        r = rows[name]
        m = r["max_nn"]
        want = dict(job=[], query=[], src=[], slot=[], out=[], len=[], npow2=[], kept=[])
        base = 0
        for j, cnt in enumerate(r["counts"]):
            cnt = np.array(cnt, np.int64)
            kept = np.minimum(cnt, m) if m > 0 else cnt
            fo = np.concatenate([[0], np.cumsum(cnt)])
            ko = np.concatenate([[0], np.cumsum(kept)])
            own = 0
            for q in np.nonzero(cnt > TILE)[0]:
                want["job"].append(j), want["query"].append(int(q)), want["src"].append(int(fo[q])), want["slot"].append(base + own), want["out"].append(int(ko[q]))
                want["len"].append(int(cnt[q])), want["npow2"].append(_pow2(cnt[q])), want["kept"].append(int(kept[q]))
                own += _pow2(cnt[q])
            assert r["job_slot_keys"][j] == own
            base += own
        assert r["ok"] == 1 and r["slot_keys"] == base and r["max_pow2"] == max(want["npow2"], default=0)
        for k, v in want.items():
            assert r[k] == v, (name, k)
    two = rows["two_long_jobs"]
    assert two["job"] == [0, 0, 2, 2] and two["own_slot"] == [0, 8192, 0, 16384] and two["slot"] == [0, 8192, 16384, 32768] and two["max_pow2"] == 32768
    assert rows["two_long_jobs_cut"]["kept"] == [4100, 4097, 4100, 4100]
    assert rows["no_long"]["job"] == [] and rows["no_long"]["slot_keys"] == 0
