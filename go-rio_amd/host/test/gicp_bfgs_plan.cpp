// Drives the BFGS minimiser of GICP_OMP (go-rio_amd/csrc/gicp_bfgs.h) on closed-form functions: host code only, nothing of HIP or the library.
// One JSON line per case: status, inner iterations, callbacks, final point, final value and gradient norm.
//   quadratic     f = 1/2 sum c_i (x_i - t_i)^2
//   rosenbrock    the chained Rosenbrock function in six variables from (-1.2, 1, -1.2, 1, -1.2, 1)
//   zero_gradient the quadratic started at its minimiser: g = 0, the first step reports no progress and never divides by |g|
//   fp0_zero      a constant function: f, g = 0 everywhere (fp0 == 0 at the start)
//   cap           rosenbrock stopped by the inner-iteration cap of 3
//   nan           an objective that turns NaN away from the start: the solver reports failure instead of looping
#include <cmath>
#include <cstdio>

#include "../../csrc/gicp_bfgs.h"

using namespace gorio_bfgs;

static const double kC[6] = {1.0, 2.0, 4.0, 0.5, 3.0, 8.0}, kT[6] = {0.3, -0.2, 0.1, 0.05, -0.4, 0.25};

static Callbacks quadratic() {
  Callbacks cb;
  cb.fdf = [](const double* x, double* f, double* g) {
    *f = 0.0;
    for (int i = 0; i < 6; ++i) { const double d = x[i] - kT[i]; *f += 0.5 * kC[i] * d * d; g[i] = kC[i] * d; }
  };
  cb.f = [cb](const double* x) { double f, g[6]; cb.fdf(x, &f, g); return f; };
  cb.df = [cb](const double* x, double* g) { double f; cb.fdf(x, &f, g); };
  return cb;
}

static Callbacks rosenbrock() {
  Callbacks cb;
  cb.fdf = [](const double* x, double* f, double* g) {
    *f = 0.0;
    for (int i = 0; i < 6; ++i) g[i] = 0.0;
    for (int i = 0; i < 5; ++i) {
      const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
      *f += 100.0 * a * a + b * b;
      g[i] += -400.0 * a * x[i] - 2.0 * b;
      g[i + 1] += 200.0 * a;
    }
  };
  cb.f = [cb](const double* x) { double f, g[6]; cb.fdf(x, &f, g); return f; };
  cb.df = [cb](const double* x, double* g) { double f; cb.fdf(x, &f, g); };
  return cb;
}

static Callbacks constant() {
  Callbacks cb;
  cb.fdf = [](const double*, double* f, double* g) { *f = 7.0; for (int i = 0; i < 6; ++i) g[i] = 0.0; };
  cb.f = [](const double*) { return 7.0; };
  cb.df = [](const double*, double* g) { for (int i = 0; i < 6; ++i) g[i] = 0.0; };
  return cb;
}

static Callbacks turns_nan() {
  Callbacks cb = quadratic();
  Callbacks q = cb;
  cb.f = [q](const double* x) { return std::fabs(x[0]) < 1e-3 ? q.f(x) : NAN; };
  return cb;
}

static void run(const char* name, Callbacks cb, const double* start, int max_inner, double tol) {
  double x[6];
  for (int i = 0; i < 6; ++i) x[i] = start[i];
  Solver s(cb);
  int inner = 0;
  const int status = minimize(s, x, max_inner, tol, &inner);
  std::printf("{\"case\": \"%s\", \"status\": %d, \"inner\": %d, \"evaluations\": %d, \"x\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], \"f\": %.17g, \"gnorm\": %.17g}\n", name,
              status, inner, s.evaluations, x[0], x[1], x[2], x[3], x[4], x[5], s.value(), norm6(s.gradient()));
}

int main() {
  const double zero[6] = {0, 0, 0, 0, 0, 0};
  const double ros[6] = {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0};
  run("quadratic", quadratic(), zero, 400, 1e-10);
  run("rosenbrock", rosenbrock(), ros, 400, 1e-8);
  run("zero_gradient", quadratic(), kT, 20, 1e-2);
  run("fp0_zero", constant(), zero, 20, 1e-2);
  run("cap", rosenbrock(), ros, 3, 1e-8);
  run("nan", turns_nan(), zero, 20, 1e-2);
  return 0;
}
