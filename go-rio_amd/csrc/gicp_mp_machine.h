// gicp_mp_machine.h -- the Gauss-Newton shell of FastGICPMultiPoints (GORIO_METHOD_GICP_MP, apd_gicp_mp.hip) as a resumable machine,
// host only.  The loop of the align is taken apart into "give me the pose of the next pass" and "here are the 28 sums of that pass", so
// that one align (a batch of one) and the lock-step rounds of gorio_apd_gicp_mp_align_batch run the same arithmetic in the same order.
// Nothing here knows about HIP: apd_gicp_mp.hip includes it, and host/test/gicp_mp_machine.cpp feeds it sums from a file.
//
// The sums of a pass: [0..20] H (upper triangle, row-major), [21..26] g, [27] the source points that had a neighbour.
// Two deviations from the reference end an align early and unconverged (include/gorio_apd.h): a pass in which no point has a neighbour
// (nothing to solve), and a non-finite step (the reference's solver substitutes a random one).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

namespace gorio_mp {

// Eigen::LDLT<6x6>(A).solve(rhs): ldlt6_solve of apd_kernels.hip on the host
inline void mp_ldlt6_solve(const double* A_in, const double* rhs, double* x) {
  double A[36], y[6], col[6];
  int perm[6];
  for (int i = 0; i < 36; ++i) A[i] = A_in[i];
  for (int i = 0; i < 6; ++i) perm[i] = i;
  for (int k = 0; k < 6; ++k) {
    int piv = k;
    double best = std::fabs(A[k * 6 + k]);
    for (int i = k + 1; i < 6; ++i)
      if (std::fabs(A[i * 6 + i]) > best) {
        best = std::fabs(A[i * 6 + i]);
        piv = i;
      }
    if (piv != k) {
      for (int c = 0; c < 6; ++c) std::swap(A[k * 6 + c], A[piv * 6 + c]);
      for (int r = 0; r < 6; ++r) std::swap(A[r * 6 + k], A[r * 6 + piv]);
      std::swap(perm[k], perm[piv]);
    }
    const double d = A[k * 6 + k];
    if (d == 0.0) continue;
    for (int i = k + 1; i < 6; ++i) col[i] = A[i * 6 + k];
    for (int i = k + 1; i < 6; ++i) {
      const double l = col[i] / d;
      for (int j = k + 1; j <= i; ++j) A[i * 6 + j] -= l * col[j];
      A[i * 6 + k] = l;
    }
    for (int i = k + 1; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j) A[i * 6 + j] = A[j * 6 + i];
  }
  for (int i = 0; i < 6; ++i) y[i] = rhs[perm[i]];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j) y[i] -= A[i * 6 + j] * y[j];
  for (int i = 0; i < 6; ++i) y[i] = (A[i * 6 + i] != 0.0) ? y[i] / A[i * 6 + i] : 0.0;
  for (int i = 5; i >= 0; --i)
    for (int j = i + 1; j < 6; ++j) y[i] -= A[j * 6 + i] * y[j];
  for (int i = 0; i < 6; ++i) x[perm[i]] = y[i];
}

// exp: Rodrigues in double, R = I + A K + B K^2 with K = skew(w), K^2 = w w^T - theta^2 I.  theta^2 < 1e-12: A = 1 - theta^2 / 6, B = 1 / 2 -
// theta^2 / 24; otherwise A = sin(theta) / theta, B = 2 sin^2(theta / 2) / theta^2.  R row-major 3 x 3.
inline void mp_exp(const double* w, double* R) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  double A, B;
  if (th2 < 1e-12) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    const double th = std::sqrt(th2), sh = std::sin(0.5 * th);
    A = std::sin(th) / th;
    B = 2.0 * sh * sh / th2;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = ((r == c ? 1.0 : 0.0) + A * K[r * 3 + c]) + B * (w[r] * w[c] - (r == c ? th2 : 0.0));
}

// log: v = (R32 - R23, R13 - R31, R21 - R12) / 2 = sin(theta) axis, c = (trace - 1) / 2, theta = atan2(|v|, c), w = f v with f = theta /
// |v|, or 1 + theta^2 / 6 when |v| < 1e-6.  Rotations near pi (|v| small with c < 0) are outside the domain of this class's steps.
inline void mp_log(const double* R, double* w) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double s = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double th = std::atan2(s, c);
  const double f = s < 1e-6 ? 1.0 + th * th / 6.0 : th / s;
  for (int a = 0; a < 3; ++a) w[a] = f * v[a];
}

// trans of MPI:131-133, 158-160: [float(exp(x.head)) | x.tail], 12 floats
inline void mp_trans(const float* x, float* T12) {
  const double w[3] = {(double)x[0], (double)x[1], (double)x[2]};
  double R[9];
  mp_exp(w, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T12[r * 4 + c] = (float)R[r * 3 + c];
    T12[r * 4 + 3] = x[3 + r];
  }
}

// is_converged (MPI:118-127) in float: the scale 1 / epsilon is rounded to float before it multiplies
inline bool mp_converged(const float* delta, double rot_eps, double trans_eps) {
  const double w[3] = {(double)delta[0], (double)delta[1], (double)delta[2]};
  double R[9];
  mp_exp(w, R);
  const float ri = (float)(1.0 / rot_eps), ti = (float)(1.0 / trans_eps);
  float worst = 0.f;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) worst = std::max(worst, ri * std::fabs((float)R[r * 3 + c] - (r == c ? 1.f : 0.f)));
  for (int a = 0; a < 3; ++a) worst = std::max(worst, ti * std::fabs(delta[3 + a]));
  return worst < 1.f;
}

inline void mp_unpack_H(const double* sums, double* H) {
  int t = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      H[r * 6 + c] = sums[t];
      H[c * 6 + r] = sums[t++];
    }
}

// One align.  begin(), then while (!done()): next_pose() -> run the pass at that pose -> consume(its sums).  results() at any time after.
struct MpMachine {
  enum End { kRunning = 0, kConverged = 1, kMaxIterations = 2, kAllEmpty = 3, kNonFinite = 4 };
  float x0[6] = {0, 0, 0, 0, 0, 0};  // so(3) log of the rotation, translation
  double H[36];                      // of the last pass
  int pass = 0;                      // index of the pass pending (= passes run so far)
  int nr = 0;                        // nr_iterations as the reference's loop variable leaves it
  int max_iterations = 0;
  double rot_eps = 0.0, trans_eps = 0.0;
  End end = kRunning;

  void begin(const float* guess16, int max_iter, double rotation_epsilon, double transformation_epsilon) {
    double R[9], w[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)guess16[r * 4 + c];
    mp_log(R, w);
    for (int a = 0; a < 3; ++a) {
      x0[a] = (float)w[a];
      x0[3 + a] = guess16[a * 4 + 3];
    }
    std::memset(H, 0, sizeof(H));
    pass = 0;
    nr = 0;
    max_iterations = max_iter;
    rot_eps = rotation_epsilon;
    trans_eps = transformation_epsilon;
    end = max_iter > 0 ? kRunning : kMaxIterations;
  }
  bool done() const { return end != kRunning; }
  bool converged() const { return end == kConverged; }

  // the float pose [R | t] (12 floats, rows) of the pass pending
  void next_pose(float* T12) {
    nr = pass;
    mp_trans(x0, T12);
  }

  // the 28 sums of the pass at next_pose(): solve, update, test
  void consume(const double* sums) {
    ++pass;
    mp_unpack_H(sums, H);
    if (sums[27] < 1.0) {  // no source point has a neighbour: nothing to solve
      end = kAllEmpty;
      return;
    }
    double dd[6];
    mp_ldlt6_solve(H, sums + 21, dd);
    float delta[6];
    bool finite = true;
    for (int a = 0; a < 6; ++a) {
      delta[a] = (float)dd[a];
      finite = finite && std::isfinite(delta[a]);
    }
    if (!finite) {
      end = kNonFinite;
      return;
    }
    {
      const double nd[3] = {-(double)delta[0], -(double)delta[1], -(double)delta[2]}, xw[3] = {(double)x0[0], (double)x0[1], (double)x0[2]};
      double Rd[9], Rx[9], Rn[9], w[3];
      mp_exp(nd, Rd);
      mp_exp(xw, Rx);
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = (Rd[r * 3] * Rx[c] + Rd[r * 3 + 1] * Rx[3 + c]) + Rd[r * 3 + 2] * Rx[6 + c];
      mp_log(Rn, w);
      for (int a = 0; a < 3; ++a) {
        x0[a] = (float)w[a];
        x0[3 + a] = x0[3 + a] - delta[3 + a];
      }
    }
    if (mp_converged(delta, rot_eps, trans_eps)) end = kConverged;
    else if (pass >= max_iterations) end = kMaxIterations;
  }

  void results(float* T16, double* H_out, int* conv, int* nr_iterations, int* n_linearize) const {
    float T12[12];
    mp_trans(x0, T12);
    for (int i = 0; i < 12; ++i) T16[i] = T12[i];
    T16[12] = 0.f; T16[13] = 0.f; T16[14] = 0.f; T16[15] = 1.f;
    if (H_out) std::memcpy(H_out, H, sizeof(H));
    if (conv) *conv = converged() ? 1 : 0;
    if (nr_iterations) *nr_iterations = nr;
    if (n_linearize) *n_linearize = pass;
  }
};

}  // namespace gorio_mp
