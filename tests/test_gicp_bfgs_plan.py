"""CPU test of GICP_OMP's BFGS minimiser (go-rio_amd/csrc/gicp_bfgs.h) through its stand-alone driver
go-rio_amd/host/test/gicp_bfgs_plan.cpp, which links nothing of HIP or the library.  The driver is built twice, plain and with
-fsanitize=address,undefined; both binaries must print the same and stay silent on stderr.  Its closed-form cases are checked against
their known minimisers and against the NumPy solver of tests/gicp_omp_restatement.py, written from the same specification in DESIGN.md:
equal statuses, iteration and evaluation counts."""
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


class Fun:
    def __init__(self, fdf, f=None):
        self._fdf, self._f = fdf, f

    def fdf(self, x):
        return self._fdf(x)

    def f(self, x):
        return self._f(x) if self._f else self._fdf(x)[0]

    def df(self, x):
        return self._fdf(x)[1]


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


CASES = {
    "quadratic": (Fun(quadratic), np.zeros(6), 400, 1e-10),
    "rosenbrock": (Fun(rosenbrock), ROS0, 400, 1e-8),
    "zero_gradient": (Fun(quadratic), T, 20, 1e-2),
    "fp0_zero": (Fun(constant), np.zeros(6), 20, 1e-2),
    "cap": (Fun(rosenbrock), ROS0, 3, 1e-8),
    "nan": (Fun(quadratic, lambda x: quadratic(x)[0] if abs(x[0]) < 1e-3 else float("nan")), np.zeros(6), 20, 1e-2),
}


@pytest.fixture(scope="module")
def outputs():
    subprocess.check_call(["make", "-C", HOST, "test/gicp_bfgs_plan", "test/gicp_bfgs_plan_san"], stdout=subprocess.DEVNULL)
    out = {}
    for name in ("gicp_bfgs_plan", "gicp_bfgs_plan_san"):
        r = subprocess.run([os.path.join(HOST, "test", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (name, r.stderr[-2000:])
        out[name] = r.stdout
    return out


def test_sanitized_build_prints_the_same(outputs):
    assert outputs["gicp_bfgs_plan"] == outputs["gicp_bfgs_plan_san"] and outputs["gicp_bfgs_plan"].count("\n") == len(CASES)


@pytest.fixture(scope="module")
def results(outputs):
    return {r["case"]: r for r in map(json.loads, outputs["gicp_bfgs_plan"].strip().splitlines())}


def test_closed_form_minimisers(results):
    q = results["quadratic"]
    assert q["status"] == R.SUCCESS and np.abs(np.array(q["x"]) - T).max() < 1e-10 and q["gnorm"] < 1e-10
    r = results["rosenbrock"]  # stops on Success or where rounding hides further descent; either way at the minimiser (1, ..., 1)
    assert r["status"] in (R.SUCCESS, R.NO_PROGRESS) and np.abs(np.array(r["x"]) - 1.0).max() < 1e-4 and r["f"] < 1e-9
    z = results["zero_gradient"]
    assert z["status"] == R.NO_PROGRESS and z["inner"] == 1 and z["evaluations"] == 1 and np.array_equal(np.array(z["x"]), T)
    c = results["fp0_zero"]
    assert c["status"] == R.NO_PROGRESS and c["inner"] == 1 and np.array_equal(np.array(c["x"]), np.zeros(6)) and np.isfinite(c["f"])
    assert results["cap"]["status"] == R.RUNNING and results["cap"]["inner"] == 3
    assert results["nan"]["status"] == R.FAILED and np.array_equal(np.array(results["nan"]["x"]), np.zeros(6))


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_and_restatement_take_the_same_steps(results, name):
    fun, x0, cap, tol = CASES[name]
    count = {"n": 0}

    class Counted:
        def f(self, x):
            count["n"] += 1
            return fun.f(x)

        def df(self, x):
            count["n"] += 1
            return fun.df(x)

        def fdf(self, x):
            count["n"] += 1
            return fun.fdf(x)

    x, status, inner = R.minimize(Counted(), x0, cap, tol)
    r = results[name]
    assert (status, inner, count["n"]) == (r["status"], r["inner"], r["evaluations"])
    # The counts are the strict check.  The points agree to the resolution of a line search in double, sqrt(DBL_EPSILON) = 1.5e-8 of the
    # step scale (f stops telling two trial points apart below it), accumulated over up to 264 steps whose dot products NumPy and the
    # header sum in different orders: 1e-7.
    assert np.abs(x - np.array(r["x"])).max() <= 1e-7 * max(1.0, np.abs(x).max())
