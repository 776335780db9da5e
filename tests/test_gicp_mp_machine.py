"""CPU test of the resumable Gauss-Newton shell of FastGICPMultiPoints (go-rio_amd/csrc/gicp_mp_machine.h) through its stand-alone driver
go-rio_amd/host/test/gicp_mp_machine.cpp, which links nothing of HIP or the library and is built twice, plain and with
-fsanitize=address,undefined.  The restatement (tests/gicp_mp_restatement.py) runs its align loop here pass by pass; the 28 sums of every
pass go to the driver in a file, and the machine must ask for every pass at the restatement's pose and end where it ends -- compared as
bits: the shell is a handful of double operations on libm's sin, sqrt and atan2, which both sides call.  Cases: two scenes to convergence,
one cut by max_iterations, the all-empty exit, and a non-finite step (a NaN put into g of the second pass)."""
import json
import os
import subprocess

import numpy as np
import pytest

import gicp_mp_restatement as R
import gicp_mp_scenes as M

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
F, D = np.float32, np.float64
END = dict(converged=1, max_iterations=2, all_empty=3, non_finite=4)


def sums_of(P):
    s = np.zeros(28, D)
    t = 0
    for r in range(6):
        for c in range(r, 6):
            s[t] = P.H[r, c]
            t += 1
    s[21:27] = P.g
    s[27] = P.n_used
    return s


def walk(name, spoil=None, **over):
    """the loop of gicp_mp_restatement.align with its poses and sums recorded; spoil = (pass, entry): that sum becomes NaN before the shell sees it"""
    sc = M.scenes()[name]
    p = M.params_of(name)
    p.update(over)
    src, tgt, g = sc["source"], sc["target"], np.asarray(sc["guess"], F)
    cs = R.covariances(src, p["k_correspondences"], p["regularization"])
    ct = R.covariances(tgt, p["k_correspondences"], p["regularization"])
    x0 = np.concatenate([R.so3_log(g[:3, :3].astype(D)).astype(F), g[:3, 3]]).astype(F)
    poses, sums, end, nr = [], [], "max_iterations", 0
    H = np.zeros((6, 6), D)
    for i in range(p["max_iterations"]):
        nr = i
        poses.append(R.trans_of(x0))
        P = R.one_pass(src, cs, tgt, ct, poses[-1], p["neighbor_search_radius"])
        s = sums_of(P)
        if spoil and spoil[0] == i:
            s[spoil[1]] = np.nan
        sums.append(s)
        Hs = np.zeros((6, 6), D)
        t = 0
        for r in range(6):
            for c in range(r, 6):
                Hs[r, c] = Hs[c, r] = s[t]
                t += 1
        H = Hs
        if s[27] < 1.0:
            end = "all_empty"
            break
        delta = R.ldlt6_solve(Hs, s[21:27]).astype(F)
        if not np.isfinite(delta).all():
            end = "non_finite"
            break
        Rn = R._mul3(R.so3_exp(-delta[:3].astype(D)), R.so3_exp(x0[:3].astype(D)))
        x0 = np.concatenate([R.so3_log(Rn).astype(F), x0[3:] - delta[3:]]).astype(F)
        if R.convergence_ratio(delta, p["rotation_epsilon"], p["transformation_epsilon"]) < 1.0:
            end = "converged"
            break
    return dict(name=name, guess=g, params=p, poses=poses, sums=sums, end=end, nr=nr, T=R.trans_of(x0), H=H)


@pytest.fixture(scope="module")
def cases():
    out = dict(id_64_300=walk("id_64_300"), guess_255_300_r025=walk("guess_255_300_r025"), all_empty=walk("all_empty"), cut=walk("id_64_300", max_iterations=2),
               non_finite=walk("id_64_300", spoil=(1, 23)), none=walk("id_64_300", max_iterations=0))
    for name in ("id_64_300", "guess_255_300_r025", "all_empty"):  # the walk IS the restatement's align
        ref = M.reference(name)
        w = out[name]
        assert w["T"].tobytes() == ref["T"].tobytes() and len(w["sums"]) == ref["passes"] and w["nr"] == ref["iterations"] and (w["end"] == "converged") == ref["converged"]
    assert [out[k]["end"] for k in ("id_64_300", "all_empty", "cut", "non_finite", "none")] == ["converged", "all_empty", "max_iterations", "non_finite", "max_iterations"]
    assert len(out["non_finite"]["sums"]) == 2 and len(out["cut"]["sums"]) == 2 and len(out["none"]["sums"]) == 0
    return out


@pytest.fixture(scope="module")
def rows(cases, tmp_path_factory):
    subprocess.check_call(["make", "-C", HOST, "test/gicp_mp_machine", "test/gicp_mp_machine_san"], stdout=subprocess.DEVNULL)
    path = str(tmp_path_factory.mktemp("mp_machine") / "cases.txt")
    with open(path, "w") as f:
        for key, c in cases.items():
            p = c["params"]
            f.write("case %s %d %s %s %d\n" % (key, p["max_iterations"], float(p["rotation_epsilon"]).hex(), float(p["transformation_epsilon"]).hex(), len(c["sums"])))
            f.write(" ".join(float(v).hex() for v in c["guess"].reshape(-1)) + "\n")
            for s in c["sums"]:
                f.write(" ".join(float(v).hex() for v in s) + "\n")
    out = {}
    for name in ("gicp_mp_machine", "gicp_mp_machine_san"):
        r = subprocess.run([os.path.join(HOST, "test", name), path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    assert out["gicp_mp_machine"] == out["gicp_mp_machine_san"]
    return {r["case"]: r for r in map(json.loads, out["gicp_mp_machine"].strip().splitlines())}


def test_machine_walks_the_restatements_poses(cases, rows):
    assert set(rows) == set(cases)
    for key, c in cases.items():
        r = rows[key]
        n = len(c["sums"])
        assert r["fed"] == n and r["done"] == 1 and r["end"] == END[c["end"]], key  # it took every pass on offer and wanted no more
        assert r["n_linearize"] == n and r["nr_iterations"] == c["nr"] and r["converged"] == (1 if c["end"] == "converged" else 0), key
        for i, (got, want) in enumerate(zip(r["poses"], c["poses"])):
            assert got == np.asarray(want, F)[:3, :].reshape(-1).view(np.uint32).tolist(), (key, i)
        T = np.eye(4, dtype=F)
        T[:3, :] = np.asarray(c["T"], F)[:3, :]
        assert r["T"] == T.reshape(-1).view(np.uint32).tolist(), key
        assert r["H"] == c["H"].reshape(-1).view(np.uint64).tolist(), key
