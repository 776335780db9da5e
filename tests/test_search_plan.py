"""CPU test of the host-side planning of the radius queries (go-rio_amd/csrc/search_plan.h) through its stand-alone driver
go-rio_amd/host/test/search_plan.cpp, which links nothing of HIP or the library.  The driver is built twice, plain and with
-fsanitize=address,undefined; both binaries must print the same and stay silent on stderr.  Every number it prints is recomputed
here from the rules the header states: exclusive scans, kept = min(found, max_nn), segments of at most 4096 keys sort in LDS, longer
ones get a power-of-two slot of at least 4096 keys, totals above 2^31 - 1 are refused."""
import json
import os
import subprocess

import numpy as np
import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
LDS_MAX, TILE = 4096, 4096


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", HOST, "test/search_plan", "test/search_plan_san"], stdout=subprocess.DEVNULL)
    out = {}
    for name in ("search_plan", "search_plan_san"):
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    return out


def test_sanitized_build_prints_the_same(outputs):
    assert outputs["search_plan"] == outputs["search_plan_san"] and outputs["search_plan"].count("\n") == 5 * 4 + 2


@pytest.fixture(scope="module")
def rows(outputs):
    return list(map(json.loads, outputs["search_plan"].strip().splitlines()))


def _slot(n):
    p = TILE
    while p < n:
        p *= 2
    return p


def test_plans(rows):
    plans = [r for r in rows if isinstance(r["case"], int)]
    assert len(plans) == 20 and {r["case"] for r in plans} == set(range(5))
    seen_long = 0
    for r in plans:
        fo = np.array(r["found_offs"], np.int64)
        cnt = np.diff(fo)
        m = r["max_nn"]
        kept = np.minimum(cnt, m) if m > 0 else cnt
        assert r["ok"] == 1 and r["planned"] == 1 and fo[0] == 0 and (cnt >= 0).all()
        assert np.array_equal(np.array(r["kept_offs"], np.int64), np.concatenate([[0], np.cumsum(kept)]).astype(np.int64))
        cls = np.where(cnt == 0, 0, np.where(cnt <= LDS_MAX, 1, 2))
        assert r["class"] == cls.tolist() and r["n_lds"] == int((cls == 1).sum())
        lq = np.nonzero(cls == 2)[0]
        seen_long += len(lq)
        slots = np.array([_slot(c) for c in cnt[lq]], np.int64)
        assert r["long_query"] == lq.tolist() and r["long_len"] == cnt[lq].tolist() and r["long_kept"] == kept[lq].tolist()
        assert r["long_src"] == fo[lq].tolist() and r["long_out"] == np.array(r["kept_offs"], np.int64)[lq].tolist()
        assert r["long_npow2"] == slots.tolist() and r["long_slot"] == (np.cumsum(slots) - slots).tolist()
        assert r["slot_keys"] == int(slots.sum()) and r["max_pow2"] == (int(slots.max()) if len(slots) else 0)
        assert r["found_total"] == int(fo[-1]) and r["kept_total"] == int(kept.sum())
    assert seen_long > 0
    boundary = next(r for r in plans if r["case"] == 3 and r["max_nn"] == 0)
    assert boundary["class"] == [1, 1, 2, 0, 2, 2, 2, 1] and boundary["long_npow2"] == [8192, 8192, 16384, 16384]


def test_refusals_and_arithmetic(rows):
    ref = next(r for r in rows if r["case"] == "refusals")
    assert ref == dict(case="refusals", total_3x2e30=0, total_2e31=0, total_2e31m1=1, negative=0, start=0, descending=0, over=0, one_segment_2e31m1=0)
    a = next(r for r in rows if r["case"] == "arith")
    assert (a["slot_1"], a["slot_4097"], a["slot_2e30"], a["slot_2e30p1"]) == (4096, 8192, 2 ** 30, 0)
    assert a["grown_0"] >= 1 and a["grown_800"] >= 800 and (a["cap_eq"], a["cap_less"]) == (1, 0)
    assert (a["kept_0_5"], a["kept_9_5"], a["kept_9_0"]) == (0, 5, 9)
