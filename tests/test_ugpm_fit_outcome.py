"""CPU test of two pieces of host logic of the UGPM back end through their stand-alone driver go-rio_amd/host/test/ugpm_fit_outcome.cpp
(no HIP, no library), built plain and with -fsanitize=address,undefined:
  fit_outcome (ugpm_windows.h): after a batch whose fits got the previous batch's iteration budget and no look at the done flags, the
    windows to run again are exactly those the device marked unfinished, and the next budget is what the slowest FINISHED window needed;
  ata_cut (ugpm_device.h): the cut of the lower-triangular 16 x 16 tiling of a J^T J into workgroups covers every tile once, no group
    exceeds its tile count or straddles the first tile row behind the zero columns, and a larger window never has fewer groups (the
    launch sizes its grid by the largest window of the batch)."""
import json
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
UNFINISHED, NUMERIC, RANGE = 2, -6, -3  # kStatusUnfinished (ugpm_device.h), gorio_ugpm_status

# per window: host status, is_lpm, device status word, iterations the rotation / velocity fit needed
_BATCHES = {
    "all_finished": [(0, 0, 0, 4, 6), (0, 0, 0, 3, 5), (0, 0, 0, 4, 2)],
    "one_unfinished_rotation": [(0, 0, 0, 4, 6), (0, 0, UNFINISHED, 0, 0), (0, 0, 0, 3, 5)],
    "unfinished_velocity_keeps_no_need": [(0, 0, UNFINISHED, 9, 0), (0, 0, 0, 3, 5)],  # its rotation count comes back with the re-run
    "refused_lpm_and_failed": [(RANGE, 0, 0, 40, 40), (0, 1, 1, 40, 40), (0, 0, NUMERIC, 40, 40), (0, 0, 0, 3, 5), (0, 1, UNFINISHED, 0, 0)],
    "all_unfinished": [(0, 0, UNFINISHED, 0, 0), (0, 0, UNFINISHED, 0, 0)],
    "empty": [],
}
_WANT = {
    "all_finished": ([], [4, 6]),
    "one_unfinished_rotation": ([1], [4, 6]),
    "unfinished_velocity_keeps_no_need": ([0], [3, 5]),
    "refused_lpm_and_failed": ([], [3, 5]),  # an LPM window's word 16 is not a fit's status
    "all_unfinished": ([0, 1], [0, 0]),
    "empty": ([], [0, 0]),
}
_CUTS = [(n, zc, tpg) for tpg in (24, 48) for S in range(5, 161) for n, zc in ((6 * S, 3 * S), (6 * S, 6 * S), (3 * S, 3 * S))]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    subprocess.check_call(["make", "-C", HOST, "test/ugpm_fit_outcome", "test/ugpm_fit_outcome_san"])
    path = str(tmp_path_factory.mktemp("ugpm_outcome") / "commands.txt")
    with open(path, "w") as f:
        for rows in _BATCHES.values():
            f.write("batch %d\n" % len(rows) + "".join("%d %d %d %d %d\n" % r for r in rows))
        f.write("".join("cut %d %d %d\n" % c for c in _CUTS))
    plain = subprocess.run([os.path.join(HOST, "test", "ugpm_fit_outcome"), path], capture_output=True, text=True, timeout=120)
    san = subprocess.run([os.path.join(HOST, "test", "ugpm_fit_outcome_san"), path], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stderr == "", plain.stderr
    assert san.returncode == 0 and san.stderr == "", san.stderr
    assert san.stdout == plain.stdout
    out = [json.loads(line) for line in plain.stdout.splitlines()]
    assert len(out) == len(_BATCHES) + len(_CUTS)
    return out


@pytest.mark.parametrize("k,name", list(enumerate(_BATCHES)))
def test_windows_to_rerun_and_next_budget(lines, k, name):
    assert (lines[k]["rerun"], lines[k]["need"]) == _WANT[name]


def test_tile_cut_covers_every_tile_once(lines):
    cuts = dict(zip(_CUTS, lines[len(_BATCHES):]))
    for (n, zc, tpg), c in cuts.items():
        T = (n + 15) // 16
        tz = T if zc >= n else (zc + 15) // 16
        assert c["ntile"] == T * (T + 1) // 2 and c["q_zero"] == tz * (tz + 1) // 2
        lo, hi, skips = c["lo"], c["hi"], c["skips"]
        assert len(lo) == c["ng_dense"] + c["ng_skip"] and lo[0] == 0 and hi[-1] == c["ntile"] and lo[1:] == hi[:-1]
        assert all(0 < h - l <= tpg for l, h in zip(lo, hi))
        assert skips == [0] * c["ng_dense"] + [1] * c["ng_skip"]
        for l, h, s in zip(lo, hi, skips):  # a skipping group holds only tiles whose rows start at or behind zero_col
            assert (l >= c["q_zero"]) if s else (h <= c["q_zero"])
        if zc >= n:  # no zero columns: the plain cut
            ng = -(-c["ntile"] // tpg)
            assert c["ng_skip"] == 0 and lo == [g * c["ntile"] // ng for g in range(ng)]
        # the first tile row a skipping group may hold is the first that starts at or behind zero_col: 16 tz >= zero_col > 16 (tz - 1)
        assert 16 * tz >= min(zc, n) > 16 * (tz - 1)


def test_group_count_grows_with_the_window(lines):
    cuts = dict(zip(_CUTS, lines[len(_BATCHES):]))
    for tpg in (24, 48):
        for kind in (lambda S: (6 * S, 3 * S), lambda S: (6 * S, 6 * S), lambda S: (3 * S, 3 * S)):
            counts = [cuts[kind(S) + (tpg,)]["ng_dense"] + cuts[kind(S) + (tpg,)]["ng_skip"] for S in range(5, 161)]
            assert counts == sorted(counts)


def test_c4_shape(lines):
    """S = 66 (n = 396, 25 tile rows, 325 tiles): 91 tiles in 2 groups see the gyro rows, 234 tiles in 5 groups do not."""
    c = dict(zip(_CUTS, lines[len(_BATCHES):]))[(396, 198, 48)]
    assert (c["ntile"], c["q_zero"], c["ng_dense"], c["ng_skip"]) == (325, 91, 2, 5)
