// gicp_bfgs.h -- the BFGS minimiser behind GICP_OMP's inner solve (estimateRigidTransformationBFGS, GO:193-246), host only.
//
// pcl/registration/bfgs.h (PCL 1.10's port of GSL's vector_bfgs2 with Fletcher's line search) is not part of this tree: what follows is
// written from the rule-by-rule specification in DESIGN.md ("GICP_OMP: the BFGS specification"), which is RECALLED from the published
// algorithm and unpinned.  Nothing here knows about HIP: the objective arrives as three callbacks -- f(x), df(x, g), fdf(x, f, g) -- so
// the solver runs against closed-form functions in host/test/gicp_bfgs_plan.cpp and against the device functor in apd_gicp_omp.hip.
#pragma once
#include <cmath>
#include <cfloat>
#include <functional>

namespace gorio_bfgs {

constexpr int N = 6;

// BFGSSpace::Status values the caller tests (GO:226-236); kFailed has no counterpart there: a non-finite objective value or step
enum Status { kRunning = -1, kSuccess = 0, kNoProgress = 1, kFailed = 2 };

struct Params {
  int bracket_iters = 100, section_iters = 100;
  double rho = 0.01, sigma = 0.01, tau1 = 9.0, tau2 = 0.05, tau3 = 0.5, step_size = 1.0;
  int order = 3;
};

struct Callbacks {
  std::function<double(const double*)> f;
  std::function<void(const double*, double*)> df;
  std::function<void(const double*, double*, double*)> fdf;
};

inline double dot6(const double* a, const double* b) {
  double s = 0.0;
  for (int i = 0; i < N; ++i) s += a[i] * b[i];
  return s;
}
inline double norm6(const double* a) { return std::sqrt(dot6(a, a)); }

// roots of a x^2 + b x + c in ascending order; returns how many (rule Q)
inline int solve_quadratic(double a, double b, double c, double* x0, double* x1) {
  if (a == 0.0) {
    if (b == 0.0) return 0;
    *x0 = -c / b;
    return 1;
  }
  const double disc = b * b - 4.0 * a * c;
  if (disc > 0.0) {
    if (b == 0.0) {
      const double r = std::sqrt(-c / a);
      *x0 = -r;
      *x1 = r;
    } else {
      const double sgnb = b > 0.0 ? 1.0 : -1.0;
      const double temp = -0.5 * (b + sgnb * std::sqrt(disc));
      const double r1 = temp / a, r2 = c / temp;
      *x0 = r1 < r2 ? r1 : r2;
      *x1 = r1 < r2 ? r2 : r1;
    }
    return 2;
  }
  if (disc == 0.0) {
    *x0 = *x1 = -0.5 * b / a;
    return 2;
  }
  return 0;
}

inline double interp_quad(double f0, double fp0, double f1, double zl, double zh) {  // rule I2
  const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
  const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
  const double c = 2.0 * (f1 - f0 - fp0);
  double zmin = zl, fmin = fl;
  if (fh < fmin) { zmin = zh; fmin = fh; }
  if (c > 0.0) {
    const double z = -fp0 / c;
    if (z > zl && z < zh) {
      const double f = f0 + z * (fp0 + z * (f1 - f0 - fp0));
      if (f < fmin) { zmin = z; fmin = f; }
    }
  }
  return zmin;
}

inline double cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }

inline double interp_cubic(double f0, double fp0, double f1, double fp1, double zl, double zh) {  // rule I3
  const double eta = 3.0 * (f1 - f0) - 2.0 * fp0 - fp1;
  const double xi = fp0 + fp1 - 2.0 * (f1 - f0);
  const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
  double zmin = zl, fmin = cubic(c0, c1, c2, c3, zl);
  auto check = [&](double z) {
    const double y = cubic(c0, c1, c2, c3, z);
    if (y < fmin) { zmin = z; fmin = y; }
  };
  check(zh);
  double z0 = 0.0, z1 = 0.0;
  const int n = solve_quadratic(3.0 * c3, 2.0 * c2, c1, &z0, &z1);
  if (n == 2) {
    if (z0 > zl && z0 < zh) check(z0);
    if (z1 > zl && z1 < zh) check(z1);
  } else if (n == 1) {
    if (z0 > zl && z0 < zh) check(z0);
  }
  return zmin;
}

inline double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax, int order) {  // rule I
  double zmin = (xmin - a) / (b - a), zmax = (xmax - a) / (b - a);
  if (zmin > zmax) { const double t = zmin; zmin = zmax; zmax = t; }
  double z;
  if (order > 2 && !std::isnan(fpb)) z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax);
  else z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax);
  return a + z * (b - a);
}

class Solver {
 public:
  Params parameters;
  int evaluations = 0;  // callbacks made so far (each of f, df, fdf counts one)

  explicit Solver(Callbacks cb) : cb_(std::move(cb)) {}

  // minimizeInit (rule S)
  int init(const double* x) {
    iter_ = 0;
    delta_f_ = 0.0;
    for (int i = 0; i < N; ++i) dx_[i] = 0.0;
    eval_fdf(x, &f_, g_);
    for (int i = 0; i < N; ++i) { x0_[i] = x[i]; g0_[i] = g_[i]; x_[i] = x[i]; }
    g0norm_ = norm6(g0_);
    for (int i = 0; i < N; ++i) p_[i] = g_[i] * (-1.0 / g0norm_);
    pnorm_ = norm6(p_);
    fp0_ = -g0norm_;
    change_direction();
    return kSuccess;
  }

  // minimizeOneStep (rule T); x is read and, on kSuccess, replaced by the new iterate
  int step(double* x) {
    double alpha = 0.0, alpha1;
    const double f0 = f_;
    // (a NaN here -- a zero gradient at the start makes p = 0 / 0 -- is "no progress" too: every comparison below would be false)
    if (pnorm_ == 0.0 || g0norm_ == 0.0 || fp0_ == 0.0 || std::isnan(pnorm_) || std::isnan(fp0_)) {
      for (int i = 0; i < N; ++i) dx_[i] = 0.0;
      return kNoProgress;
    }
    if (delta_f_ < 0.0) {
      const double del = std::fmax(-delta_f_, 10.0 * DBL_EPSILON * std::fabs(f0));
      alpha1 = std::fmin(1.0, 2.0 * del / (-fp0_));
    } else {
      alpha1 = std::fabs(parameters.step_size);
    }
    const int status = line_search(alpha1, &alpha);
    if (status != kSuccess) return status;
    // updatePosition: x, f, g at the accepted alpha (from the cache when the line search ended on a full evaluation)
    {
      double fa, dfa;
      wrap_fdf(alpha, &fa, &dfa);
      f_ = fa;
      for (int i = 0; i < N; ++i) { x_[i] = xa_[i]; g_[i] = ga_[i]; x[i] = xa_[i]; }
    }
    if (!std::isfinite(f_)) return kFailed;
    delta_f_ = f_ - f0;
    {  // memoryless BFGS direction: p = g - A dx - B dg
      double dx0[N], dg0[N];
      for (int i = 0; i < N; ++i) { dx0[i] = x_[i] - x0_[i]; dx_[i] = dx0[i]; dg0[i] = g_[i] - g0_[i]; }
      const double dxg = dot6(dx0, g_), dgg = dot6(dg0, g_), dxdg = dot6(dx0, dg0), dgnorm = norm6(dg0);
      double A = 0.0, B = 0.0;
      if (dxdg != 0.0) {
        B = dxg / dxdg;
        A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
      }
      for (int i = 0; i < N; ++i) p_[i] = g_[i] - A * dx0[i] - B * dg0[i];
    }
    for (int i = 0; i < N; ++i) { g0_[i] = g_[i]; x0_[i] = x_[i]; }
    g0norm_ = norm6(g0_);
    pnorm_ = norm6(p_);
    const double pg = dot6(p_, g_);
    const double dir = pg >= 0.0 ? -1.0 : 1.0;
    for (int i = 0; i < N; ++i) p_[i] *= dir / pnorm_;
    pnorm_ = norm6(p_);
    fp0_ = dot6(p_, g0_);
    change_direction();
    ++iter_;
    return kSuccess;
  }

  // testGradient (rule G)
  int test_gradient(double epsilon) const {
    if (epsilon < 0.0) return kFailed;
    return norm6(g_) < epsilon ? kSuccess : kRunning;
  }

  double value() const { return f_; }
  const double* gradient() const { return g_; }

 private:
  Callbacks cb_;
  int iter_ = 0;
  double f_ = 0.0, delta_f_ = 0.0, fp0_ = 0.0, g0norm_ = 0.0, pnorm_ = 0.0;
  double x_[N], g_[N], x0_[N], g0_[N], p_[N], dx_[N];
  // the evaluation cache along x_ + alpha p_ (rule C)
  double xa_[N], ga_[N], f_alpha_ = 0.0, df_alpha_ = 0.0;
  double x_key_ = 0.0, f_key_ = 0.0, g_key_ = 0.0, df_key_ = 0.0;

  double eval_f(const double* x) { ++evaluations; return cb_.f(x); }
  void eval_df(const double* x, double* g) { ++evaluations; cb_.df(x, g); }
  void eval_fdf(const double* x, double* f, double* g) { ++evaluations; cb_.fdf(x, f, g); }

  void change_direction() {
    for (int i = 0; i < N; ++i) { xa_[i] = x_[i]; ga_[i] = g_[i]; }
    f_alpha_ = f_;
    x_key_ = f_key_ = g_key_ = df_key_ = 0.0;
    df_alpha_ = dot6(ga_, p_);
  }
  void move_to(double alpha) {
    if (alpha == x_key_) return;
    for (int i = 0; i < N; ++i) xa_[i] = x_[i] + alpha * p_[i];
    x_key_ = alpha;
  }
  double wrap_f(double alpha) {
    if (alpha == f_key_) return f_alpha_;
    move_to(alpha);
    f_alpha_ = eval_f(xa_);
    f_key_ = alpha;
    return f_alpha_;
  }
  double wrap_df(double alpha) {
    if (alpha == df_key_) return df_alpha_;
    move_to(alpha);
    if (alpha != g_key_) {
      eval_df(xa_, ga_);
      g_key_ = alpha;
    }
    df_alpha_ = dot6(ga_, p_);
    df_key_ = alpha;
    return df_alpha_;
  }
  void wrap_fdf(double alpha, double* f, double* df) {
    if (alpha == f_key_ && alpha == df_key_) {
      *f = f_alpha_;
      *df = df_alpha_;
      return;
    }
    if (alpha == f_key_ || alpha == df_key_) {
      *f = wrap_f(alpha);
      *df = wrap_df(alpha);
      return;
    }
    move_to(alpha);
    eval_fdf(xa_, &f_alpha_, ga_);
    f_key_ = g_key_ = alpha;
    df_alpha_ = dot6(ga_, p_);
    df_key_ = alpha;
    *f = f_alpha_;
    *df = df_alpha_;
  }

  // Fletcher's bracketing and sectioning (rule L)
  int line_search(double alpha1, double* alpha_new) {
    const double rho = parameters.rho, sigma = parameters.sigma, tau1 = parameters.tau1, tau2 = parameters.tau2, tau3 = parameters.tau3;
    const int order = parameters.order;
    double f0, fp0, falpha, falpha_prev, fpalpha = 0.0, fpalpha_prev, delta, alpha_next;
    double alpha = alpha1, alpha_prev = 0.0;
    double a, b, fa, fb, fpa, fpb;
    int i = 0;
    wrap_fdf(0.0, &f0, &fp0);
    falpha_prev = f0;
    fpalpha_prev = fp0;
    a = 0.0; b = alpha; fa = f0; fb = 0.0; fpa = fp0; fpb = 0.0;
    while (i++ < parameters.bracket_iters) {
      if (!std::isfinite(alpha)) return kFailed;
      falpha = wrap_f(alpha);
      if (std::isnan(falpha)) return kFailed;
      if (falpha > f0 + alpha * rho * fp0 || falpha >= falpha_prev) {
        a = alpha_prev; fa = falpha_prev; fpa = fpalpha_prev;
        b = alpha; fb = falpha; fpb = NAN;
        break;
      }
      fpalpha = wrap_df(alpha);
      if (std::fabs(fpalpha) <= -sigma * fp0) {
        *alpha_new = alpha;
        return kSuccess;
      }
      if (fpalpha >= 0.0) {
        a = alpha; fa = falpha; fpa = fpalpha;
        b = alpha_prev; fb = falpha_prev; fpb = fpalpha_prev;
        break;
      }
      delta = alpha - alpha_prev;
      alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + tau1 * delta, order);
      alpha_prev = alpha; falpha_prev = falpha; fpalpha_prev = fpalpha;
      alpha = alpha_next;
    }
    while (i++ < parameters.section_iters) {
      delta = b - a;
      alpha = interpolate(a, fa, fpa, b, fb, fpb, a + tau2 * delta, b - tau3 * delta, order);
      if (!std::isfinite(alpha)) return kFailed;
      falpha = wrap_f(alpha);
      if (std::isnan(falpha)) return kFailed;
      if ((a - alpha) * fpa <= DBL_EPSILON) return kNoProgress;  // roundoff prevents progress
      if (falpha > f0 + rho * alpha * fp0 || falpha >= fa) {
        b = alpha; fb = falpha; fpb = NAN;
      } else {
        fpalpha = wrap_df(alpha);
        if (std::fabs(fpalpha) <= -sigma * fp0) {
          *alpha_new = alpha;
          return kSuccess;
        }
        if (((b - a) >= 0.0 && fpalpha >= 0.0) || ((b - a) <= 0.0 && fpalpha <= 0.0)) {
          b = a; fb = fa; fpb = fpa;
          a = alpha; fa = falpha; fpa = fpalpha;
        } else {
          a = alpha; fa = falpha; fpa = fpalpha;
        }
      }
    }
    return kSuccess;  // iteration budget spent: *alpha_new keeps the caller's 0, the step re-evaluates at x and restarts along -g (rule L5)
  }
};

// The loop of GO:219-235 around the solver: returns the last status, `inner` = minimizeOneStep calls made.
inline int minimize(Solver& s, double* x, int max_inner_iterations, double gradient_tol, int* inner) {
  s.init(x);
  int n = 0, result = kRunning;
  do {
    ++n;
    result = s.step(x);
    if (result) break;
    result = s.test_gradient(gradient_tol);
  } while (result == kRunning && n < max_inner_iterations);
  *inner = n;
  return result;
}

}  // namespace gorio_bfgs
