"""CPU test of the resumable BFGS of GICP_OMP (gorio_bfgs::Machine, go-rio_amd/csrc/gicp_bfgs.h) through its stand-alone driver
go-rio_amd/host/test/gicp_bfgs_machine.cpp, which links nothing of HIP or the library.  The driver is built twice, plain and with
-fsanitize=address,undefined; both binaries must print the same and stay silent on stderr.  For every objective the request sequence and
the outcome of a machine run alone must equal those of the same machine interleaved with all the others, and those of the callback Solver;
the NumPy solver of tests/gicp_omp_restatement.py, written from the same specification, must ask for the same evaluations in the same
order and end with the same status and iteration count."""
import json
import os
import subprocess

import numpy as np
import pytest

import gicp_omp_restatement as R

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "go-rio_amd", "host")
C = np.array([1.0, 2.0, 4.0, 0.5, 3.0, 8.0])
T = np.array([0.3, -0.2, 0.1, 0.05, -0.4, 0.25])
ROS0 = np.array([-1.2, 1.0, -1.2, 1.0, -1.2, 1.0])


def quadratic(x):
    d = x - T
    f = 0.0
    for i in range(6):
        f += 0.5 * C[i] * d[i] * d[i]
    return f, C * d


def rosenbrock(x):
    f, g = 0.0, np.zeros(6)
    for i in range(5):
        a, b = x[i + 1] - x[i] * x[i], 1.0 - x[i]
        f += 100.0 * a * a + b * b
        g[i] += -400.0 * a * x[i] - 2.0 * b
        g[i + 1] += 200.0 * a
    return f, g


def constant(x):
    return 7.0, np.zeros(6)


def all_nan(x):
    return float("nan"), np.full(6, np.nan)


# name: (fdf, f or None, start, inner cap, gradient tolerance, bracket / section budget)
CASES = {
    "quadratic": (quadratic, None, np.zeros(6), 400, 1e-10, 100),
    "rosenbrock": (rosenbrock, None, ROS0, 400, 1e-8, 100),
    "zero_gradient": (quadratic, None, T, 20, 1e-2, 100),
    "fp0_zero": (constant, None, np.zeros(6), 20, 1e-2, 100),
    "cap": (rosenbrock, None, ROS0, 3, 1e-8, 100),
    "nan": (quadratic, lambda x: quadratic(x)[0] if abs(x[0]) < 1e-3 else float("nan"), np.zeros(6), 20, 1e-2, 100),
    "all_nan": (all_nan, None, np.zeros(6), 20, 1e-2, 100),
    "cap_1": (rosenbrock, None, ROS0, 1, 1e-8, 100),
    "budget_1": (rosenbrock, None, ROS0, 400, 1e-8, 1),
}
RUNS = ("alone", "interleaved", "solver")


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", HOST, "test/gicp_bfgs_machine", "test/gicp_bfgs_machine_san"], stdout=subprocess.DEVNULL)
    out = {}
    for name in ("gicp_bfgs_machine", "gicp_bfgs_machine_san"):
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    return out


@pytest.fixture(scope="module")
def results(outputs):
    res = {}
    for r in map(json.loads, outputs["gicp_bfgs_machine"].strip().splitlines()):
        res[(r["case"], r["run"])] = r
    return res


def test_sanitized_build_prints_the_same(outputs):
    assert outputs["gicp_bfgs_machine"] == outputs["gicp_bfgs_machine_san"]
    assert outputs["gicp_bfgs_machine"].count("\n") == len(CASES) * len(RUNS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_alone_interleaved_and_solver_agree(results, name):
    alone = results[(name, "alone")]
    assert alone["evaluations"] == len(alone["requests"]) >= 1 and alone["requests"][0][0] == 2  # minimizeInit asks for fdf at the start
    for run in RUNS[1:]:
        other = results[(name, run)]
        for key in ("status", "inner", "evaluations", "x", "requests"):  # x and the requests' points are hex floats: bit for bit
            assert other[key] == alone[key], (name, run, key)


def test_outcomes(results):
    get = lambda name: results[(name, "alone")]  # noqa: E731
    q = get("quadratic")
    assert q["status"] == R.SUCCESS and np.abs(np.array(q["xd"]) - T).max() < 1e-10
    r = get("rosenbrock")
    assert r["status"] in (R.SUCCESS, R.NO_PROGRESS) and np.abs(np.array(r["xd"]) - 1.0).max() < 1e-4
    for name, start in (("zero_gradient", T), ("fp0_zero", np.zeros(6)), ("all_nan", np.zeros(6))):  # the first step reports no progress: one evaluation
        z = get(name)
        assert (z["status"], z["inner"], z["evaluations"]) == (R.NO_PROGRESS, 1, 1) and np.array_equal(np.array(z["xd"]), start)
    assert (get("cap")["status"], get("cap")["inner"]) == (R.RUNNING, 3)
    assert (get("cap_1")["status"], get("cap_1")["inner"]) == (R.RUNNING, 1)
    assert get("nan")["status"] == R.FAILED and np.array_equal(np.array(get("nan")["xd"]), np.zeros(6))
    b = get("budget_1")  # every line search spends its budget in the bracketing pass: never more than f, df and the step's fdf per iteration
    assert b["inner"] >= 1 and b["evaluations"] <= 1 + 3 * b["inner"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_machine_and_restatement_take_the_same_steps(results, name):
    fdf, f_only, x0, cap, tol, budget = CASES[name]
    modes = []

    class Recorded:
        def f(self, x):
            modes.append(0)
            return f_only(x) if f_only else fdf(x)[0]

        def df(self, x):
            modes.append(1)
            return fdf(x)[1]

        def fdf(self, x):
            modes.append(2)
            return fdf(x)

    s = R.Bfgs(Recorded(), bracket_iters=budget, section_iters=budget)  # the loop of R.minimize with the budget of the case
    s.init(x0)
    n, status = 0, R.RUNNING
    while True:
        n += 1
        status = s.step()
        if status:
            break
        status = s.test_gradient(tol)
        if not (status == R.RUNNING and n < cap):
            break
    r = results[(name, "alone")]
    assert (status, n, len(modes)) == (r["status"], r["inner"], r["evaluations"])
    assert modes == [q[0] for q in r["requests"]]
    # The points agree to the resolution of a line search in double, accumulated over the steps (see tests/test_gicp_bfgs_plan.py): 1e-7.
    assert np.abs(s.x - np.array(r["xd"])).max() <= 1e-7 * max(1.0, np.abs(s.x).max())
