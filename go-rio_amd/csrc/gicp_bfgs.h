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

// The minimiser as a resumable machine: minimizeInit, then the loop of GO:219-235 (minimizeOneStep, testGradient, the iteration cap), suspended
// wherever it needs the objective.  start() runs up to the first evaluation; request() names the evaluation wanted (kF, kDf, kFdf: the
// modes of the device functor) and the point, or kFinished; resume() feeds the answer and runs on to the next evaluation or to the end.
// The body is ONE function whose position is kept in pc_ (a switch with a case behind every suspension), so every local of the step and
// of the line search is a member.  Solver / minimize() below answer the requests through callbacks; apd_gicp_omp.hip answers them from the
// device, one handle at a time or many in lock-step.
class Machine {
 public:
  enum Request { kF = 0, kDf = 1, kFdf = 2, kFinished = 3 };
  Params parameters;

  void start(const double* x, int max_inner_iterations, double gradient_tol) {
    for (int i = 0; i < N; ++i) { x_[i] = x[i]; xa_[i] = x[i]; }
    max_inner_ = max_inner_iterations;
    tol_ = gradient_tol;
    pc_ = 0;
    req_ = kFinished;
    n_ = 0;
    result_ = kRunning;
    advance();
  }
  // the evaluation wanted: its mode, and the point in x (untouched when finished)
  int request(double* x) const {
    if (req_ != kFinished)
      for (int i = 0; i < N; ++i) x[i] = xa_[i];
    return req_;
  }
  // f is read for kF and kFdf, g (6 values) for kDf and kFdf
  void resume(double f, const double* g) {
    if (req_ == kFinished) return;
    if (req_ != kDf) ans_f_ = f;
    if (req_ != kF)
      for (int i = 0; i < N; ++i) ans_g_[i] = g[i];
    advance();
  }
  bool finished() const { return req_ == kFinished; }
  int status() const { return result_; }  // the last status of the loop of GO:219-235
  int inner() const { return n_; }        // minimizeOneStep calls made
  const double* x() const { return x_; }  // the iterate: the start until a step succeeds
  double value() const { return f_; }
  const double* gradient() const { return g_; }

 private:
  int pc_ = 0, req_ = kFinished, max_inner_ = 0, n_ = 0, result_ = kRunning;
  double tol_ = 0.0, ans_f_ = 0.0, ans_g_[N] = {0, 0, 0, 0, 0, 0};
  int iter_ = 0;
  double f_ = 0.0, delta_f_ = 0.0, fp0_ = 0.0, g0norm_ = 0.0, pnorm_ = 0.0;
  double x_[N], g_[N], x0_[N], g0_[N], p_[N], dx_[N];
  // the evaluation cache along x_ + alpha p_ (rule C)
  double xa_[N], ga_[N], f_alpha_ = 0.0, df_alpha_ = 0.0;
  double x_key_ = 0.0, f_key_ = 0.0, g_key_ = 0.0, df_key_ = 0.0;
  // locals of minimizeOneStep (s_) and of the line search (l_)
  double s_alpha_ = 0.0, s_alpha1_ = 0.0, s_f0_ = 0.0, s_fa_ = 0.0, s_dfa_ = 0.0;
  int s_status_ = kSuccess;
  double l_f0_ = 0.0, l_fp0_ = 0.0, l_falpha_ = 0.0, l_falpha_prev_ = 0.0, l_fpalpha_ = 0.0, l_fpalpha_prev_ = 0.0, l_delta_ = 0.0, l_alpha_next_ = 0.0;
  double l_alpha_ = 0.0, l_alpha_prev_ = 0.0, l_a_ = 0.0, l_b_ = 0.0, l_fa_ = 0.0, l_fb_ = 0.0, l_fpa_ = 0.0, l_fpb_ = 0.0;
  int l_i_ = 0;

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
  int test_gradient(double epsilon) const {  // testGradient (rule G)
    if (epsilon < 0.0) return kFailed;
    return norm6(g_) < epsilon ? kSuccess : kRunning;
  }

// suspend with a request for MODE at xa_; execution continues behind the case label with the answer in ans_f_ / ans_g_
#define GORIO_BFGS_EVAL(MODE, LABEL) \
  do {                               \
    req_ = MODE;                     \
    pc_ = LABEL;                     \
    return;                          \
    case LABEL:;                     \
  } while (0)
// the cached evaluations of rule C: OUT = f(A), OUT = f'(A), (F, DF) = both
#define GORIO_BFGS_WRAP_F(A, OUT, LABEL) \
  do {                                   \
    if ((A) == f_key_) {                 \
      OUT = f_alpha_;                    \
    } else {                             \
      move_to(A);                        \
      GORIO_BFGS_EVAL(kF, LABEL);        \
      f_alpha_ = ans_f_;                 \
      f_key_ = (A);                      \
      OUT = f_alpha_;                    \
    }                                    \
  } while (0)
#define GORIO_BFGS_WRAP_DF(A, OUT, LABEL)                 \
  do {                                                    \
    if ((A) == df_key_) {                                 \
      OUT = df_alpha_;                                    \
    } else {                                              \
      move_to(A);                                         \
      if ((A) != g_key_) {                                \
        GORIO_BFGS_EVAL(kDf, LABEL);                      \
        for (int i = 0; i < N; ++i) ga_[i] = ans_g_[i];   \
        g_key_ = (A);                                     \
      }                                                   \
      df_alpha_ = dot6(ga_, p_);                          \
      df_key_ = (A);                                      \
      OUT = df_alpha_;                                    \
    }                                                     \
  } while (0)
#define GORIO_BFGS_WRAP_FDF(A, F, DF, L1, L2, L3)         \
  do {                                                    \
    if ((A) == f_key_ && (A) == df_key_) {                \
      F = f_alpha_;                                       \
      DF = df_alpha_;                                     \
    } else if ((A) == f_key_ || (A) == df_key_) {         \
      GORIO_BFGS_WRAP_F(A, F, L1);                        \
      GORIO_BFGS_WRAP_DF(A, DF, L2);                      \
    } else {                                              \
      move_to(A);                                         \
      GORIO_BFGS_EVAL(kFdf, L3);                          \
      f_alpha_ = ans_f_;                                  \
      for (int i = 0; i < N; ++i) ga_[i] = ans_g_[i];     \
      f_key_ = g_key_ = (A);                              \
      df_alpha_ = dot6(ga_, p_);                          \
      df_key_ = (A);                                      \
      F = f_alpha_;                                       \
      DF = df_alpha_;                                     \
    }                                                     \
  } while (0)

  void advance() {
    const double rho = parameters.rho, sigma = parameters.sigma, tau1 = parameters.tau1, tau2 = parameters.tau2, tau3 = parameters.tau3;
    const int order = parameters.order;
    switch (pc_) {
      case 0:
        // minimizeInit (rule S); start() has put the start into x_ and xa_
        iter_ = 0;
        delta_f_ = 0.0;
        for (int i = 0; i < N; ++i) dx_[i] = 0.0;
        GORIO_BFGS_EVAL(kFdf, 1);
        f_ = ans_f_;
        for (int i = 0; i < N; ++i) { g_[i] = ans_g_[i]; x0_[i] = x_[i]; g0_[i] = g_[i]; }
        g0norm_ = norm6(g0_);
        for (int i = 0; i < N; ++i) p_[i] = g_[i] * (-1.0 / g0norm_);
        pnorm_ = norm6(p_);
        fp0_ = -g0norm_;
        change_direction();
        // the loop of GO:219-235
        n_ = 0;
        result_ = kRunning;
        do {
          ++n_;
          // minimizeOneStep (rule T)
          s_alpha_ = 0.0;
          s_f0_ = f_;
          // (a NaN here -- a zero gradient at the start makes p = 0 / 0 -- is "no progress" too: every comparison below would be false)
          if (pnorm_ == 0.0 || g0norm_ == 0.0 || fp0_ == 0.0 || std::isnan(pnorm_) || std::isnan(fp0_)) {
            for (int i = 0; i < N; ++i) dx_[i] = 0.0;
            result_ = kNoProgress;
            break;
          }
          if (delta_f_ < 0.0) {
            const double del = std::fmax(-delta_f_, 10.0 * DBL_EPSILON * std::fabs(s_f0_));
            s_alpha1_ = std::fmin(1.0, 2.0 * del / (-fp0_));
          } else {
            s_alpha1_ = std::fabs(parameters.step_size);
          }
          // Fletcher's bracketing and sectioning (rule L): s_status_, and s_alpha_ where it accepts a point
          l_fpalpha_ = 0.0;
          l_alpha_ = s_alpha1_;
          l_alpha_prev_ = 0.0;
          l_i_ = 0;
          GORIO_BFGS_WRAP_FDF(0.0, l_f0_, l_fp0_, 2, 3, 4);
          l_falpha_prev_ = l_f0_;
          l_fpalpha_prev_ = l_fp0_;
          l_a_ = 0.0; l_b_ = l_alpha_; l_fa_ = l_f0_; l_fb_ = 0.0; l_fpa_ = l_fp0_; l_fpb_ = 0.0;
          while (l_i_++ < parameters.bracket_iters) {
            if (!std::isfinite(l_alpha_)) { s_status_ = kFailed; goto line_search_done; }
            GORIO_BFGS_WRAP_F(l_alpha_, l_falpha_, 5);
            if (std::isnan(l_falpha_)) { s_status_ = kFailed; goto line_search_done; }
            if (l_falpha_ > l_f0_ + l_alpha_ * rho * l_fp0_ || l_falpha_ >= l_falpha_prev_) {
              l_a_ = l_alpha_prev_; l_fa_ = l_falpha_prev_; l_fpa_ = l_fpalpha_prev_;
              l_b_ = l_alpha_; l_fb_ = l_falpha_; l_fpb_ = NAN;
              break;
            }
            GORIO_BFGS_WRAP_DF(l_alpha_, l_fpalpha_, 6);
            if (std::fabs(l_fpalpha_) <= -sigma * l_fp0_) {
              s_alpha_ = l_alpha_;
              s_status_ = kSuccess;
              goto line_search_done;
            }
            if (l_fpalpha_ >= 0.0) {
              l_a_ = l_alpha_; l_fa_ = l_falpha_; l_fpa_ = l_fpalpha_;
              l_b_ = l_alpha_prev_; l_fb_ = l_falpha_prev_; l_fpb_ = l_fpalpha_prev_;
              break;
            }
            l_delta_ = l_alpha_ - l_alpha_prev_;
            l_alpha_next_ = interpolate(l_alpha_prev_, l_falpha_prev_, l_fpalpha_prev_, l_alpha_, l_falpha_, l_fpalpha_, l_alpha_ + l_delta_, l_alpha_ + tau1 * l_delta_, order);
            l_alpha_prev_ = l_alpha_; l_falpha_prev_ = l_falpha_; l_fpalpha_prev_ = l_fpalpha_;
            l_alpha_ = l_alpha_next_;
          }
          while (l_i_++ < parameters.section_iters) {
            l_delta_ = l_b_ - l_a_;
            l_alpha_ = interpolate(l_a_, l_fa_, l_fpa_, l_b_, l_fb_, l_fpb_, l_a_ + tau2 * l_delta_, l_b_ - tau3 * l_delta_, order);
            if (!std::isfinite(l_alpha_)) { s_status_ = kFailed; goto line_search_done; }
            GORIO_BFGS_WRAP_F(l_alpha_, l_falpha_, 7);
            if (std::isnan(l_falpha_)) { s_status_ = kFailed; goto line_search_done; }
            if ((l_a_ - l_alpha_) * l_fpa_ <= DBL_EPSILON) { s_status_ = kNoProgress; goto line_search_done; }  // roundoff prevents progress
            if (l_falpha_ > l_f0_ + rho * l_alpha_ * l_fp0_ || l_falpha_ >= l_fa_) {
              l_b_ = l_alpha_; l_fb_ = l_falpha_; l_fpb_ = NAN;
            } else {
              GORIO_BFGS_WRAP_DF(l_alpha_, l_fpalpha_, 8);
              if (std::fabs(l_fpalpha_) <= -sigma * l_fp0_) {
                s_alpha_ = l_alpha_;
                s_status_ = kSuccess;
                goto line_search_done;
              }
              if (((l_b_ - l_a_) >= 0.0 && l_fpalpha_ >= 0.0) || ((l_b_ - l_a_) <= 0.0 && l_fpalpha_ <= 0.0)) {
                l_b_ = l_a_; l_fb_ = l_fa_; l_fpb_ = l_fpa_;
                l_a_ = l_alpha_; l_fa_ = l_falpha_; l_fpa_ = l_fpalpha_;
              } else {
                l_a_ = l_alpha_; l_fa_ = l_falpha_; l_fpa_ = l_fpalpha_;
              }
            }
          }
          s_status_ = kSuccess;  // iteration budget spent: s_alpha_ keeps its 0, the step re-evaluates at x and restarts along -g (rule L5)
        line_search_done:
          if (s_status_ != kSuccess) {
            result_ = s_status_;
            break;
          }
          // updatePosition: x, f, g at the accepted alpha (from the cache when the line search ended on a full evaluation)
          GORIO_BFGS_WRAP_FDF(s_alpha_, s_fa_, s_dfa_, 9, 10, 11);
          f_ = s_fa_;
          for (int i = 0; i < N; ++i) { x_[i] = xa_[i]; g_[i] = ga_[i]; }
          if (!std::isfinite(f_)) {
            result_ = kFailed;
            break;
          }
          delta_f_ = f_ - s_f0_;
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
            for (int i = 0; i < N; ++i) { g0_[i] = g_[i]; x0_[i] = x_[i]; }
            g0norm_ = norm6(g0_);
            pnorm_ = norm6(p_);
            const double pg = dot6(p_, g_);
            const double dir = pg >= 0.0 ? -1.0 : 1.0;
            for (int i = 0; i < N; ++i) p_[i] *= dir / pnorm_;
            pnorm_ = norm6(p_);
            fp0_ = dot6(p_, g0_);
          }
          change_direction();
          ++iter_;
          result_ = test_gradient(tol_);
        } while (result_ == kRunning && n_ < max_inner_);
        req_ = kFinished;
        pc_ = 12;
        return;
      case 12:
      default:
        req_ = kFinished;
        return;
    }
  }
#undef GORIO_BFGS_WRAP_FDF
#undef GORIO_BFGS_WRAP_DF
#undef GORIO_BFGS_WRAP_F
#undef GORIO_BFGS_EVAL
};

// The machine answered through callbacks.  `evaluations` counts the callbacks made (each of f, df, fdf counts one).
class Solver {
 public:
  Params parameters;
  int evaluations = 0;

  explicit Solver(Callbacks cb) : cb_(std::move(cb)) {}

  double value() const { return m_.value(); }
  const double* gradient() const { return m_.gradient(); }

  // runs the machine from x to its end; x becomes the final iterate
  int run(double* x, int max_inner_iterations, double gradient_tol, int* inner) {
    m_.parameters = parameters;
    m_.start(x, max_inner_iterations, gradient_tol);
    double xe[N], f, g[N];
    for (;;) {
      const int mode = m_.request(xe);
      if (mode == Machine::kFinished) break;
      ++evaluations;
      f = 0.0;
      if (mode == Machine::kF) f = cb_.f(xe);
      else if (mode == Machine::kDf) cb_.df(xe, g);
      else cb_.fdf(xe, &f, g);
      m_.resume(f, g);
    }
    for (int i = 0; i < N; ++i) x[i] = m_.x()[i];
    *inner = m_.inner();
    return m_.status();
  }

 private:
  Callbacks cb_;
  Machine m_;
};

// The loop of GO:219-235 around the solver: returns the last status, `inner` = minimizeOneStep calls made.
inline int minimize(Solver& s, double* x, int max_inner_iterations, double gradient_tol, int* inner) { return s.run(x, max_inner_iterations, gradient_tol, inner); }

}  // namespace gorio_bfgs
