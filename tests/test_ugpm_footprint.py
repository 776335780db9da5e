"""CPU test of the rule that picks the instantiations of the GP solver kernels for a batch (solver_sizes, go-rio_amd/csrc/ugpm_windows.h)
through its stand-alone driver go-rio_amd/host/test/ugpm_footprint.cpp (no HIP, no library), built plain and with
-fsanitize=address,undefined.  The kernels are templates on the panel rows block_cholesky keeps in LDS (ROWS) and on the 16 x 16 blocks a
wave of blocked_lower_solve16 keeps in registers (KMAX).  Below, the index arithmetic of both (ugpm_kernels.hip) is restated in Python and
walked for every window the library accepts, S in [1, 160], and every instantiation the rule can return for it:
nothing is stored past ROWS or KMAX, and every decision that ROWS takes part in comes out as it does with 384."""
import json
import os
import subprocess

import pytest

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
S_ALL = range(1, 161)  # the issue's range is [17, 160] (overlap 8); smaller overlaps give smaller windows, down to one state
FULL_ROWS, FULL_KMAX, NB = 384, 16, 16


@pytest.fixture(scope="module")
def rule():
    subprocess.check_call(["make", "-C", HOST, "test/ugpm_footprint", "test/ugpm_footprint_san"])
    args = [str(S_ALL[0]), str(S_ALL[-1])]
    plain = subprocess.run([os.path.join(HOST, "test", "ugpm_footprint")] + args, capture_output=True, text=True, timeout=120)
    san = subprocess.run([os.path.join(HOST, "test", "ugpm_footprint_san")] + args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stderr == "", plain.stderr
    assert san.returncode == 0 and san.stderr == "", san.stderr
    assert san.stdout == plain.stdout
    out = [json.loads(line) for line in plain.stdout.splitlines()]
    head, rows = out[0], {r["S"]: r for r in out[1:]}
    assert sorted(rows) == list(S_ALL)
    return head, rows


def chol_walk(rows, n, rhs):
    """block_cholesky<rows> on an n x n system (rhs: one more row rides along), 512 threads: per block column the decisions ROWS takes
    part in; and the highest panel row and inverse-pivot slot written."""
    la = n - min(NB, n) + (1 if rhs else 0) <= rows  # nwave >= 2 in every caller
    decisions, top_row, top_dinv = [], -1, -1
    for kb in range(0, n, NB):
        nb = min(NB, n - kb)
        m = n - kb - nb
        me = m + (1 if rhs else 0)
        own = min(me, rows)
        if rhs:
            top_dinv = max(top_dinv, kb + nb - 1)
        if me <= 0:
            decisions.append((la, own, 0, False))
            break
        passes = []
        for p0 in range(0, me, rows):
            mp = min(rows, me - p0)
            top_row = max(top_row, mp - 1)  # the panel solve writes P[i], i < mp
            pad_end = ((m if rhs else mp) + 15) & ~15  # zeroed rows mp .. pad_end - 1
            if pad_end > mp:
                top_row = max(top_row, pad_end - 1)
            passes.append((p0, mp, p0 != 0 or me > rows))
        decisions.append((la, own, tuple(passes)))
    return decisions, top_row, top_dinv


def solve_blocks(n, jb=0):
    """blocked_lower_solve16: the largest t for which some wave v in 0..3 and block row i < ceil(n / 16) has k = jb + v + 4 t < i, plus one."""
    nblk = (n + 15) // 16
    ts = [t for t in range(64) for v in range(4) if jb + v + 4 * t < nblk - 1]
    return max(ts) + 1 if ts else 0


def test_every_instantiation_is_one_the_rule_names(rule):
    head, rows = rule
    inst = head["instantiations"]
    assert head["max_states"] == S_ALL[-1]
    for S, r in rows.items():
        for z in (r["sized"], r["full"]):
            assert [z["gram_rows"], z["gram_kmax"]] in inst["gram"] and z["lm_rows"] in inst["lm"] and z["solve_kmax"] in inst["solve"], (S, z)
        assert r["full"] == dict(gram_rows=FULL_ROWS, gram_kmax=FULL_KMAX, lm_rows=FULL_ROWS, solve_kmax=FULL_KMAX)


def test_panel_rows_fit_and_decisions_are_those_of_384(rule):
    _, rows = rule
    for S in S_ALL:
        for z in (rows[S]["sized"], rows[S]["full"]):
            # gram_kernel: block_cholesky of S x S without a right-hand side, then ceil16(S) rows of the solve's X in the same buffer
            for s in range(1, S + 1) if z is rows[S]["sized"] else (S,):  # a batch's smaller windows run the largest one's instantiation
                dec, top, _ = chol_walk(z["gram_rows"], s, False)
                assert dec == chol_walk(FULL_ROWS, s, False)[0], (S, s)
                assert max(top + 1, (s + 15) // 16 * 16) <= z["gram_rows"], (S, s)
            assert rows[S]["need"]["gram_rows"] == max(chol_walk(FULL_ROWS, S, False)[1] + 1, (S + 15) // 16 * 16)
            # lm_step_kernel: ns = 3 S (rotation fit) or S (one velocity channel); the right-hand side rides along for ns < 384
            for s in range(1, S + 1) if z is rows[S]["sized"] else (S,):
                for ns in (3 * s, s):
                    fused = ns < FULL_ROWS  # and ns <= 512 threads, ns <= 480
                    dec, top, dinv = chol_walk(z["lm_rows"], ns, fused)
                    assert dec == chol_walk(FULL_ROWS, ns, fused)[0], (S, ns)
                    assert top + 1 <= z["lm_rows"], (S, ns, top)
                    assert dinv + 1 <= min(z["lm_rows"] + NB, FULL_ROWS), (S, ns, dinv)  # CholLds::dinv_n
                    assert z["lm_rows"] >= 34 if fused else z["lm_rows"] * 17 >= ns  # block_backward's staging rows / the unfused solve's x
        if 3 * S < FULL_ROWS:
            assert rows[S]["need"]["lm_rows"] == max(chol_walk(FULL_ROWS, 3 * S, True)[1] + 1, 34)


def test_blocks_per_wave_fit(rule):
    _, rows = rule
    for S in S_ALL:
        nblk = (S + 15) // 16
        assert rows[S]["need"]["gram_blocks"] == max(solve_blocks(S, jb) for jb in range(nblk)) == solve_blocks(S)
        assert rows[S]["need"]["solve_blocks"] == solve_blocks(6 * S)
        for z in (rows[S]["sized"], rows[S]["full"]):
            assert solve_blocks(S) <= z["gram_kmax"], S
            assert solve_blocks(6 * S) <= z["solve_kmax"], S  # corr_diag_kernel starts at jb >= 0, infer_kernel at 0: jb = 0 needs the most


def test_choice_grows_with_the_window_and_switch_points(rule):
    """The largest window of a batch decides, so a larger max_S must never select a smaller capacity; the switch points are where
    tests/test_ugpm_footprint_gpu.py puts its cases."""
    _, rows = rule
    for key in ("gram_rows", "lm_rows", "solve_kmax"):
        v = [rows[S]["sized"][key] for S in S_ALL]
        assert v == sorted(v)
    switches = sorted({S for S in S_ALL[:-1] if rows[S]["sized"] != rows[S + 1]["sized"]})
    assert switches == [69, 88, 96]
    assert rows[66]["sized"] == dict(gram_rows=96, gram_kmax=3, lm_rows=192, solve_kmax=8)
    assert rows[160]["sized"] == dict(gram_rows=160, gram_kmax=3, lm_rows=FULL_ROWS, solve_kmax=FULL_KMAX)
