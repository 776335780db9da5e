// Drives the resumable BFGS of GICP_OMP (gorio_bfgs::Machine, go-rio_amd/csrc/gicp_bfgs.h) on closed-form functions: host code only, nothing
// of HIP or the library.  Every case is run three ways, each answered by a plain function:
//   alone        one machine, its requests answered one after the other
//   interleaved  all machines of all cases started together and advanced round-robin, one answer per unfinished machine per round -- the
//                way gorio_apd_gicp_omp_align_batch drives its handles
//   solver       the callback Solver / minimize() of the same header, its callbacks wrapped to record what they are asked
// One JSON line per (case, run): the request sequence (mode 0 f, 1 df, 2 fdf, and x in hex floats) and the outcome (status, inner
// iterations, final x in hex floats).  The cases are those of gicp_bfgs_plan.cpp plus:
//   all_nan      an objective that is NaN everywhere, value and gradient
//   cap_1        rosenbrock stopped by an inner-iteration cap of 1
//   budget_1     rosenbrock with a bracket / section budget of 1 (rule L5: the step re-evaluates at x)
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../csrc/gicp_bfgs.h"

using namespace gorio_bfgs;

static const double kC[6] = {1.0, 2.0, 4.0, 0.5, 3.0, 8.0}, kT[6] = {0.3, -0.2, 0.1, 0.05, -0.4, 0.25};

typedef void (*Objective)(const double* x, double* f, double* g);

static void quadratic(const double* x, double* f, double* g) {
  *f = 0.0;
  for (int i = 0; i < 6; ++i) { const double d = x[i] - kT[i]; *f += 0.5 * kC[i] * d * d; g[i] = kC[i] * d; }
}
static void rosenbrock(const double* x, double* f, double* g) {
  *f = 0.0;
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
  for (int i = 0; i < 5; ++i) {
    const double a = x[i + 1] - x[i] * x[i], b = 1.0 - x[i];
    *f += 100.0 * a * a + b * b;
    g[i] += -400.0 * a * x[i] - 2.0 * b;
    g[i + 1] += 200.0 * a;
  }
}
static void constant(const double*, double* f, double* g) {
  *f = 7.0;
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
}
static void all_nan(const double*, double* f, double* g) {
  *f = NAN;
  for (int i = 0; i < 6; ++i) g[i] = NAN;
}

struct Case {
  const char* name;
  Objective fdf;
  bool f_turns_nan;  // the value alone (mode 0) is NaN away from the start, as in gicp_bfgs_plan.cpp's "nan"
  double start[6];
  int max_inner;
  double tol;
  int budget;  // bracket_iters = section_iters
};

static const Case kCases[] = {
    {"quadratic", quadratic, false, {0, 0, 0, 0, 0, 0}, 400, 1e-10, 100},
    {"rosenbrock", rosenbrock, false, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 400, 1e-8, 100},
    {"zero_gradient", quadratic, false, {0.3, -0.2, 0.1, 0.05, -0.4, 0.25}, 20, 1e-2, 100},
    {"fp0_zero", constant, false, {0, 0, 0, 0, 0, 0}, 20, 1e-2, 100},
    {"cap", rosenbrock, false, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 3, 1e-8, 100},
    {"nan", quadratic, true, {0, 0, 0, 0, 0, 0}, 20, 1e-2, 100},
    {"all_nan", all_nan, false, {0, 0, 0, 0, 0, 0}, 20, 1e-2, 100},
    {"cap_1", rosenbrock, false, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 1, 1e-8, 100},
    {"budget_1", rosenbrock, false, {-1.2, 1.0, -1.2, 1.0, -1.2, 1.0}, 400, 1e-8, 1},
};
static const int kNumCases = (int)(sizeof(kCases) / sizeof(kCases[0]));

// the answer to one request, by a plain function
static void answer(const Case& c, int mode, const double* x, double* f, double* g) {
  c.fdf(x, f, g);
  if (mode == Machine::kF && c.f_turns_nan && !(std::fabs(x[0]) < 1e-3)) *f = NAN;
}

struct Trace {
  std::string requests;  // [mode, "x0 .. x5"] entries
  int count = 0;
  void add(int mode, const double* x) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "%s[%d, \"%a %a %a %a %a %a\"]", count ? ", " : "", mode, x[0], x[1], x[2], x[3], x[4], x[5]);
    requests += buf;
    ++count;
  }
};

static void print(const Case& c, const char* run, const Trace& t, int status, int inner, const double* x) {
  std::printf("{\"case\": \"%s\", \"run\": \"%s\", \"status\": %d, \"inner\": %d, \"evaluations\": %d, \"x\": \"%a %a %a %a %a %a\", \"xd\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g], \"requests\": [%s]}\n",
              c.name, run, status, inner, t.count, x[0], x[1], x[2], x[3], x[4], x[5], x[0], x[1], x[2], x[3], x[4], x[5], t.requests.c_str());
}

static void start(Machine& m, const Case& c) {
  m.parameters.bracket_iters = c.budget;
  m.parameters.section_iters = c.budget;
  m.start(c.start, c.max_inner, c.tol);
}

// one answer; false when the machine had finished already
static bool advance(Machine& m, const Case& c, Trace& t) {
  double x[6], f = 0.0, g[6] = {0, 0, 0, 0, 0, 0};
  const int mode = m.request(x);
  if (mode == Machine::kFinished) return false;
  t.add(mode, x);
  answer(c, mode, x, &f, g);
  m.resume(f, g);
  return true;
}

int main() {
  // alone
  for (int k = 0; k < kNumCases; ++k) {
    Machine m;
    Trace t;
    start(m, kCases[k]);
    while (advance(m, kCases[k], t)) {}
    print(kCases[k], "alone", t, m.status(), m.inner(), m.x());
  }
  // interleaved: every machine alive at once, one answer each per round
  {
    std::vector<Machine> ms(kNumCases);
    std::vector<Trace> ts(kNumCases);
    for (int k = 0; k < kNumCases; ++k) start(ms[k], kCases[k]);
    for (bool any = true; any;) {
      any = false;
      for (int k = 0; k < kNumCases; ++k) any = advance(ms[k], kCases[k], ts[k]) || any;
    }
    for (int k = 0; k < kNumCases; ++k) print(kCases[k], "interleaved", ts[k], ms[k].status(), ms[k].inner(), ms[k].x());
  }
  // the callback Solver on the same objectives
  for (int k = 0; k < kNumCases; ++k) {
    const Case& c = kCases[k];
    Trace t;
    Callbacks cb;
    cb.f = [&](const double* x) { double f, g[6]; t.add(Machine::kF, x); answer(c, Machine::kF, x, &f, g); return f; };
    cb.df = [&](const double* x, double* g) { double f; t.add(Machine::kDf, x); answer(c, Machine::kDf, x, &f, g); };
    cb.fdf = [&](const double* x, double* f, double* g) { t.add(Machine::kFdf, x); answer(c, Machine::kFdf, x, f, g); };
    Solver s(cb);
    s.parameters.bracket_iters = c.budget;
    s.parameters.section_iters = c.budget;
    double x[6];
    for (int i = 0; i < 6; ++i) x[i] = c.start[i];
    int inner = 0;
    const int status = minimize(s, x, c.max_inner, c.tol, &inner);
    if (s.evaluations != t.count) return 1;
    print(c, "solver", t, status, inner, x);
  }
  return 0;
}
