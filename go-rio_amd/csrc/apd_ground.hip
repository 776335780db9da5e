// apd_ground.hip -- Patchwork++ ground segmentation (include/gorio_ground.h) as the preprocessing nodelet runs it (PREP:505-519).
// Included by apd_api.hip after apd_prep.hip.
//
// PWP = include/patchworkpp/patchworkpp.hpp of the Go-RIO sources.  estimate_ground (PWP:684-890) is, per scan:
//   RNR + CZM binning      ground_classify_kernel   one lane per point: noise flag, patch id, the point's range covariance
//   segments               ground_segment_kernel    one workgroup per scan: the patches' points compacted in input order
//   per-patch chain        ground_patch_kernel      one workgroup per patch: sort by (z, input index), LPR + seeds, 1 + num_iter
//                                                   plane fits with the R-GPF selections between them (PWP:1024-1128)
//   decisions, TGR, A-GLE  host                     O(patches) on the per-patch status values (PWP:745-850, 894-1018)
//   final plane            ground_final_fit_kernel  one workgroup per scan over all of cloud_ground (PWP:866-867)
//   under-ground pass      host                     PWP:872-884, with the point after every erased point left untested
// The patches of a scan are independent inside the chain: the first fit of a patch is over its seeds, and with num_lpr >= 1 and
// th_seeds > 0 (ground_check_params refuses anything else) the seeds are never empty -- the lowest point the LPR averages lies at or
// below the LPR height, or no point is averaged, the height is 0 and every point lies below the zone-0 margin (margin x sensor
// height, negative for a sensor above the ground).  So the stale
// pc_mean_ / cov_ that an empty fit inherits (see fit_plane) never crosses patches.  No workgroup waits for another.  With num_lpr = 0
// the reference's LPR height is 0 (PWP:646), a patch above th_seeds has no seeds and its first fit reads the previous patch's moments.
//
// One plane estimate (estimate_plane PWP:461-479, estimate_plane_cov PWP:497-580), fit_plane below:
//   * pcl::computeMeanAndCovarianceMatrix: the nine float accumulators of PCL 1.10, summed by ONE lane in point order, un-fused
//     (-ffp-contract=off), divided by (float)m -- bit-identical to the float restatement.  m = 0 leaves mean and covariance as
//     they were (PCL returns 0 and writes nothing).
//   * JacobiSVD of the 3 x 3 float covariance: here a cyclic Jacobi eigen-decomposition in float (the covariance is symmetric
//     positive semi-definite, so its singular values are |eigenvalues|), sorted descending, normal = the third column with n_z >= 0.
//   * id = 1: the Ceres LM fit of (n, d) in double, residual ((n.p + d)/|n|)^2 / (n^T C_p n), with Ceres 2.1's defaults as
//     SURVEY.md Appendix D restates them (max_num_iterations = 30, function / gradient / parameter tolerance
//     1e-6 / 1e-10 / 1e-8).  Each LM iteration is one workgroup reduction of J^T J, J^T r and the cost at the trial point (the
//     Jacobian there is kept in case the step is accepted); lane 0 solves the damped 4 x 4 system.  The model cost change is
//     -(g.s + s^T A s / 2) on the scaled normal equations, which is what Ceres' per-residual sum is algebraically.
#include <hip/hip_runtime.h>

namespace gorio {

constexpr int kGroundMaxPatches = 512;
constexpr int kGroundMaxFits = 9;
constexpr int kGroundLdsSort = 8192;  // patches up to this size sort in LDS; larger ones sort in the global scratch (2 n keys per scan)

struct GroundFrame {
  int pt_off, n;      // first point of the scan in the point-indexed buffers, point count
  int patch_off, n_patches;
  int key_off;        // first slot of the scan in the global sort scratch
  int num_iter, num_lpr, num_min_pts, id, enable_rnr;
  double sensor_height, th_seeds, th_dist, margin, min_range, max_range, rnr_angle, rnr_intensity;
  double min_ranges[4], ring_sizes[4], sector_sizes[4];
  int sectors[4], rings[4], zone_patch_off[4];
};

struct GroundFit {
  float mean[3], cov[9], sv[3], normal[3], d;
  int m, iters, term;
};

struct GroundPatch {
  int count, seg_off, n_ground, n_fits;
  int m[kGroundMaxFits], iters[kGroundMaxFits], term[kGroundMaxFits];
  GroundFit last;
};

struct GroundFinal {
  int list_off, count, id, pad_;
  float stale_mean[3], stale_cov[9];
};

// ------------------------------------------------------------------------------------------------ binning (PWP:657-681, 1160-1185)
// grid (ceil(max n / 256), scans), block 256.  pid: -2 RNR noise, -1 outside (min_range, max_range], else the patch id.
// C6[i]: the range covariance C_p = (R S)(R S)^T of estimate_plane_cov (PWP:501-518), upper triangle, for points in a patch.
__global__ __launch_bounds__(256) void ground_classify_kernel(const GroundFrame* __restrict__ frames, const float4* __restrict__ pts, int* __restrict__ pid,
                                                              double* __restrict__ C6) {
  const GroundFrame& f = frames[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  const float4 p = pts[f.pt_off + i];
  // reflected_noise_removal, PWP:661-665: sqrt of a float sum, then atan2 and the comparisons in double
  float rxy2 = p.x * p.x;
  rxy2 = rxy2 + p.y * p.y;
  const double rn = (double)sqrtf(rxy2);
  const double z = (double)p.z;
  const double ver = atan2(z, rn) * 180 / M_PI;
  if (f.enable_rnr && ver < f.rnr_angle && z < -f.sensor_height - 0.8 && (double)p.w < f.rnr_intensity) {
    pid[f.pt_off + i] = -2;
    return;
  }
  // pc2czm, PWP:1168-1181: xy2radius / xy2theta in double
  const double x = (double)p.x, y = (double)p.y;
  const double r = sqrt(x * x + y * y);
  if (!(r <= f.max_range && r > f.min_range)) {
    pid[f.pt_off + i] = -1;
    return;
  }
  const double a = atan2(y, x);
  const double theta = a > 0 ? a : 2 * M_PI + a;
  const int zone = r < f.min_ranges[1] ? 0 : r < f.min_ranges[2] ? 1 : r < f.min_ranges[3] ? 2 : 3;
  const int ring = min((int)((r - f.min_ranges[zone]) / f.ring_sizes[zone]), f.rings[zone] - 1);
  const int sector = min((int)(theta / f.sector_sizes[zone]), f.sectors[zone] - 1);
  pid[f.pt_off + i] = f.zone_patch_off[zone] + ring * f.sectors[zone] + sector;
  // PWP:504-518: dist and the two angles from float arithmetic, the rest in double
  float d2 = p.x * p.x;
  d2 = d2 + p.y * p.y;
  d2 = d2 + p.z * p.z;
  const double dist = (double)sqrtf(d2);
  const double sx = dist * 0.86 / 400, sy = dist * sin(0.5 / 180 * M_PI), sz = dist * sin(1.0 / 180 * M_PI);
  const double el = (double)(float)atan2((double)sqrtf(rxy2), z), az = (double)(float)atan2(y, x);
  const double ce = cos(el), se = sin(el), ca = cos(az), sa = sin(az);
  // R = Rz(az) Ry(el); A = R S
  const double A[3][3] = {{ca * ce * sx, -sa * sy, ca * se * sz}, {sa * ce * sx, ca * sy, sa * se * sz}, {-se * sx, 0.0 * sy, ce * sz}};
  double* c = C6 + 6 * (size_t)(f.pt_off + i);
  int q = 0;
  for (int r0 = 0; r0 < 3; ++r0)
    for (int r1 = r0; r1 < 3; ++r1) c[q++] = (A[r0][0] * A[r1][0] + A[r0][1] * A[r1][1]) + A[r0][2] * A[r1][2];
}

// ------------------------------------------------------------------------------------------------ segments in input order
// grid scans, block 1024 (16 waves).  Wave w owns the contiguous chunk w of the scan; pass A counts its points per patch, the
// counts are scanned in (patch, wave) order, pass B writes every point at its patch's next slot.  The result is each patch's
// points in input order, patch after patch: seg[] = scan-local indices, rec[p].count / seg_off.
__global__ __launch_bounds__(1024) void ground_segment_kernel(const GroundFrame* __restrict__ frames, const int* __restrict__ pid, int* __restrict__ seg,
                                                              GroundPatch* __restrict__ rec) {
  const GroundFrame& f = frames[blockIdx.x];
  __shared__ int wc[16][kGroundMaxPatches];
  const int P = f.n_patches;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int t = threadIdx.x; t < 16 * kGroundMaxPatches; t += 1024) (&wc[0][0])[t] = 0;
  __syncthreads();
  const int chunk = (f.n + 15) / 16;
  const int c0 = min(f.n, w * chunk), c1 = min(f.n, c0 + chunk);
  const unsigned long long lt = (1ull << lane) - 1;
  for (int pass = 0; pass < 2; ++pass) {
    for (int b = c0; b < c1; b += 64) {
      const int i = b + lane;
      const int my = i < c1 ? pid[f.pt_off + i] : -1;
      unsigned long long todo = __ballot(my >= 0);
      while (todo) {
        const int leader = __builtin_ctzll(todo);
        const int pb = __shfl(my, leader, 64);
        const unsigned long long m = __ballot(my == pb);
        if (pass == 1 && my == pb) seg[f.pt_off + wc[w][pb] + __popcll(m & lt)] = i;
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) wc[w][pb] += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        todo &= ~m;
      }
    }
    __syncthreads();
    if (pass == 0 && threadIdx.x == 0) {  // wc[w][p] <- first slot of wave w's points of patch p
      int run = 0;
      for (int p = 0; p < P; ++p) {
        rec[f.patch_off + p].seg_off = run;
        for (int v = 0; v < 16; ++v) {
          const int c = wc[v][p];
          wc[v][p] = run;
          run += c;
        }
        rec[f.patch_off + p].count = run - rec[f.patch_off + p].seg_off;
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ workgroup plane fit
struct FitShared {
  double red[4][16];
  double bc[16];        // broadcast of a reduction
  double x[4], xn[4];   // LM parameters, trial parameters
  int cmd, wcount[4];
  float mean[3], cov[9], sv[3], normal[3], d;  // pc_mean_, cov_, singular_values_, normal_, d_ (persist across the fits of a patch)
  int m;
};

__device__ __forceinline__ int wg_count(bool pred, FitShared& s) {  // all 256 lanes
  const int c = __popcll(__ballot(pred));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s.wcount[w] = c;
  __syncthreads();
  return (s.wcount[0] + s.wcount[1]) + (s.wcount[2] + s.wcount[3]);
}

// Symmetric 3 x 3 eigen-decomposition in float: cyclic Jacobi over (0,1), (0,2), (1,2), a rotation when |a_pq| > 2^-23 max(|a_pp|,
// |a_qq|) and |a_pq| >= 1e-37, until a sweep rotates nothing (at most 16 sweeps).  tests/patchwork_restatement.py svd3 is the
// same sequence of float operations.
__device__ void svd3f(const float (&cin)[9], float (&sv)[3], float (&u2)[3]) {
  float a[3][3], v[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      a[r][c] = cin[3 * r + c];
      v[r][c] = r == c ? 1.0f : 0.0f;
    }
  const int PP[3] = {0, 0, 1}, QQ[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool rotated = false;
    for (int e = 0; e < 3; ++e) {
      const int p = PP[e], q = QQ[e];
      const float apq = a[p][q], app = a[p][p], aqq = a[q][q];
      const float thr = fmaxf(fabsf(app), fabsf(aqq)) * 1.1920929e-7f;
      if (fabsf(apq) <= thr || fabsf(apq) < 1e-37f) continue;
      rotated = true;
      const float theta = (aqq - app) / (2.0f * apq);
      float t = 1.0f / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
      if (theta < 0.0f) t = -t;
      const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c;
      for (int k = 0; k < 3; ++k) {  // columns p, q of A and V
        const float akp = a[k][p], akq = a[k][q];
        a[k][p] = c * akp - s * akq;
        a[k][q] = s * akp + c * akq;
        const float vkp = v[k][p], vkq = v[k][q];
        v[k][p] = c * vkp - s * vkq;
        v[k][q] = s * vkp + c * vkq;
      }
      for (int k = 0; k < 3; ++k) {  // rows p, q of A
        const float apk = a[p][k], aqk = a[q][k];
        a[p][k] = c * apk - s * aqk;
        a[q][k] = s * apk + c * aqk;
      }
    }
    if (!rotated) break;
  }
  float e[3] = {fabsf(a[0][0]), fabsf(a[1][1]), fabsf(a[2][2])};
  int o[3] = {0, 1, 2};  // stable descending order of |eigenvalue|
  if (e[o[1]] > e[o[0]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  if (e[o[2]] > e[o[1]]) { const int t = o[1]; o[1] = o[2]; o[2] = t; }
  if (e[o[1]] > e[o[0]]) { const int t = o[0]; o[0] = o[1]; o[1] = t; }
  for (int k = 0; k < 3; ++k) {
    sv[k] = e[o[k]];
    u2[k] = v[k][o[2]];
  }
}

// One point's residual of PlaneFitCost (PWP:63-84) and its analytic gradient w.r.t. (n, d).
__device__ __forceinline__ double plane_residual(const double* x, float px, float py, float pz, const double* __restrict__ c, double (&J)[4]) {
  const double p0 = px, p1 = py, p2 = pz;
  const double a = ((x[0] * p0 + x[1] * p1) + x[2] * p2) + x[3];
  const double q = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  const double sq = sqrt(q);
  const double cn0 = (c[0] * x[0] + c[1] * x[1]) + c[2] * x[2];
  const double cn1 = (c[1] * x[0] + c[3] * x[1]) + c[4] * x[2];
  const double cn2 = (c[2] * x[0] + c[4] * x[1]) + c[5] * x[2];
  const double w = (x[0] * cn0 + x[1] * cn1) + x[2] * cn2;
  const double dist = a / sq;
  const double r = dist * dist / w;
  const double g = 2.0 * dist / w;
  const double h = 2.0 * r / w;
  J[0] = g * ((p0 - dist * x[0] / sq) / sq) - h * cn0;
  J[1] = g * ((p1 - dist * x[1] / sq) / sq) - h * cn1;
  J[2] = g * ((p2 - dist * x[2] / sq) / sq) - h * cn2;
  J[3] = g / sq;
  return r;
}

// sums over the fit's points at parameters x: [0..9] J^T J (upper triangle, row major), [10..13] J^T r, [14] r^T r -> s.bc
__device__ void wg_lm_sums(const double* x, const int* __restrict__ list, const unsigned char* __restrict__ mask, int count, const float4* __restrict__ pts, int pt_off,
                           const double* __restrict__ C6, FitShared& s) {
  double acc[15];
#pragma unroll
  for (int q = 0; q < 15; ++q) acc[q] = 0.0;
  double xl[4] = {x[0], x[1], x[2], x[3]};
  for (int k = threadIdx.x; k < count; k += 256) {
    if (mask && !mask[k]) continue;
    const int i = pt_off + list[k];
    const float4 p = pts[i];
    double J[4];
    const double r = plane_residual(xl, p.x, p.y, p.z, C6 + 6 * (size_t)i, J);
    int q = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = a; b < 4; ++b) acc[q++] += J[a] * J[b];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[10 + a] += J[a] * r;
    acc[14] += r * r;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 15; ++q) {
    const double v = wave_sum(acc[q]);
    if (lane == 0) s.red[w][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 15) s.bc[threadIdx.x] = (s.red[0][threadIdx.x] + s.red[1][threadIdx.x]) + (s.red[2][threadIdx.x] + s.red[3][threadIdx.x]);
  __syncthreads();
}

__device__ __forceinline__ double jtj_at(const double* S, int a, int b) {  // S[0..9] upper triangle of the symmetric 4 x 4
  if (a > b) { const int t = a; a = b; b = t; }
  const int base[4] = {0, 4, 7, 9};
  return S[base[a] + (b - a)];
}

// Cholesky solve of the SPD 4 x 4 system L L^T y = b; false when a pivot is not positive.
__device__ bool chol4_solve(const double (&A)[4][4], const double (&b)[4], double (&y)[4]) {
  double L[4][4] = {};
  for (int j = 0; j < 4; ++j) {
    double s = A[j][j];
    for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    for (int i = j + 1; i < 4; ++i) {
      double t = A[i][j];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / L[j][j];
    }
  }
  double z[4];
  for (int i = 0; i < 4; ++i) {
    double t = b[i];
    for (int k = 0; k < i; ++k) t -= L[i][k] * z[k];
    z[i] = t / L[i][i];
  }
  for (int i = 3; i >= 0; --i) {
    double t = z[i];
    for (int k = i + 1; k < 4; ++k) t -= L[k][i] * y[k];
    y[i] = t / L[i][i];
  }
  return true;
}

// One plane estimate over list[k] for k < count with mask[k] != 0 (mask NULL: all), in list order.  All 256 lanes.  Results in
// s.mean / cov / sv / normal / d; returns the point count, LM iterations and termination through *out (lane 0).
__device__ void fit_plane(const int* __restrict__ list, const unsigned char* __restrict__ mask, int count, const float4* __restrict__ pts, int pt_off,
                          const double* __restrict__ C6, int id, float* stage /* 3 x 256 floats */, FitShared& s, int& m_out, int& it_out, int& term_out) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // pcl::computeMeanAndCovarianceMatrix (PCL 1.10, dense cloud): the members staged 256 at a time, accumulated by lane 0 in order
  float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int m = 0;
  for (int base = 0; base < count; base += 256) {
    const int k = base + threadIdx.x;
    const bool in = k < count && (!mask || mask[k]);
    const unsigned long long b = __ballot(in);
    if (lane == 0) s.wcount[w] = __popcll(b);
    __syncthreads();
    int pos = __popcll(b & ((1ull << lane) - 1));
    for (int v = 0; v < w; ++v) pos += s.wcount[v];
    const int tot = (s.wcount[0] + s.wcount[1]) + (s.wcount[2] + s.wcount[3]);
    if (in) {
      const float4 p = pts[pt_off + list[k]];
      stage[pos] = p.x;
      stage[256 + pos] = p.y;
      stage[512 + pos] = p.z;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int j = 0; j < tot; ++j) {
        const float x = stage[j], y = stage[256 + j], z = stage[512 + j];
        acc[0] += x * x;
        acc[1] += x * y;
        acc[2] += x * z;
        acc[3] += y * y;
        acc[4] += y * z;
        acc[5] += z * z;
        acc[6] += x;
        acc[7] += y;
        acc[8] += z;
      }
    }
    m += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (m > 0) {
      const float fm = (float)m;
      for (int q = 0; q < 9; ++q) acc[q] /= fm;
      s.mean[0] = acc[6];
      s.mean[1] = acc[7];
      s.mean[2] = acc[8];
      s.cov[0] = acc[0] - acc[6] * acc[6];
      s.cov[1] = acc[1] - acc[6] * acc[7];
      s.cov[2] = acc[2] - acc[6] * acc[8];
      s.cov[4] = acc[3] - acc[7] * acc[7];
      s.cov[5] = acc[4] - acc[7] * acc[8];
      s.cov[8] = acc[5] - acc[8] * acc[8];
      s.cov[3] = s.cov[1];
      s.cov[6] = s.cov[2];
      s.cov[7] = s.cov[5];
    }  // else: PCL leaves cov_ and pc_mean_ as they were
    float c[9], n[3], sv[3];
    for (int q = 0; q < 9; ++q) c[q] = s.cov[q];
    svd3f(c, sv, n);
    if (n[2] < 0.0f) {  // PWP:475 / 527
      n[0] = -n[0];
      n[1] = -n[1];
      n[2] = -n[2];
    }
    float dd = n[0] * s.mean[0];
    dd = dd + n[1] * s.mean[1];
    dd = dd + n[2] * s.mean[2];
    for (int q = 0; q < 3; ++q) {
      s.sv[q] = sv[q];
      s.normal[q] = n[q];
    }
    s.d = -dd;
    s.x[0] = n[0];
    s.x[1] = n[1];
    s.x[2] = n[2];
    s.x[3] = s.d;
    s.m = m;
  }
  __syncthreads();
  int iters = 0, term = 0;
  if (id == 1 && m > 0) {
    // the Ceres 2.1 LM policy of SURVEY.md Appendix D with max_num_iterations = 30 and Ceres' default tolerances
    const double ftol = 1e-6, gtol = 1e-10, ptol = 1e-8;
    double cost = 0, radius = 1e4, dec = 2.0, xnorm = 0, mcc = 0, step_norm = 0;
    double scale[4], A[4][4], g[4], diag[4];
    bool reuse = false;
    wg_lm_sums(s.x, list, mask, count, pts, pt_off, C6, s);
    auto take = [&](const double* S) {  // scaled normal equations from unscaled sums (lane 0)
      for (int a = 0; a < 4; ++a) {
        g[a] = S[10 + a] * scale[a];
        for (int b = 0; b < 4; ++b) A[a][b] = (jtj_at(S, a, b) * scale[a]) * scale[b];
      }
    };
    auto gmax = [&](const double* S) {
      double v = 0;
      for (int a = 0; a < 4; ++a) v = fmax(v, fabs(S[10 + a]));
      return v;
    };
    if (threadIdx.x == 0) {
      cost = 0.5 * s.bc[14];
      s.cmd = 0;
      if (gmax(s.bc) <= gtol) {
        term = 3;
        s.cmd = 1;
      } else {
        for (int a = 0; a < 4; ++a) scale[a] = 1.0 / (1.0 + sqrt(jtj_at(s.bc, a, a)));
        take(s.bc);
        xnorm = sqrt(((s.x[0] * s.x[0] + s.x[1] * s.x[1]) + s.x[2] * s.x[2]) + s.x[3] * s.x[3]);
      }
    }
    __syncthreads();
    while (s.cmd == 0) {
      __syncthreads();
      if (threadIdx.x == 0) {
        while (true) {
          if (iters >= 30) { term = 4; s.cmd = 1; break; }
          if (radius < 1e-32) { term = 5; s.cmd = 1; break; }
          ++iters;
          if (!reuse)
            for (int a = 0; a < 4; ++a) diag[a] = fmin(fmax(A[a][a], 1e-6), 1e32);
          double lhs[4][4], step[4];
          for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) lhs[a][b] = A[a][b] + (a == b ? diag[a] / radius : 0.0);
          bool valid = chol4_solve(lhs, g, step);
          if (valid) {
            for (int a = 0; a < 4; ++a) {
              step[a] = -step[a];
              if (!isfinite(step[a])) valid = false;
            }
          }
          if (valid) {
            double gs = 0, sas = 0;
            for (int a = 0; a < 4; ++a) {
              gs += g[a] * step[a];
              double t = 0;
              for (int b = 0; b < 4; ++b) t += A[a][b] * step[b];
              sas += step[a] * t;
            }
            mcc = -(gs + sas / 2.0);
            if (!(mcc > 0.0)) valid = false;
          }
          if (!valid) {
            radius /= dec;
            dec *= 2.0;
            reuse = true;
            continue;
          }
          step_norm = 0;
          for (int a = 0; a < 4; ++a) {
            const double da = step[a] * scale[a];
            s.xn[a] = s.x[a] + da;
            step_norm += da * da;
          }
          step_norm = sqrt(step_norm);
          break;
        }
      }
      __syncthreads();
      if (s.cmd != 0) break;
      wg_lm_sums(s.xn, list, mask, count, pts, pt_off, C6, s);
      if (threadIdx.x == 0) {
        const double cost_new = 0.5 * s.bc[14];
        const double cc = cost - cost_new;
        if (step_norm <= ptol * (xnorm + ptol)) {
          term = 2;
          s.cmd = 1;
        } else if (fabs(cc) <= ftol * cost) {
          term = 1;
          s.cmd = 1;
        } else {
          const double rho = cc / mcc;
          if (rho > 1e-3) {
            for (int a = 0; a < 4; ++a) s.x[a] = s.xn[a];
            xnorm = sqrt(((s.x[0] * s.x[0] + s.x[1] * s.x[1]) + s.x[2] * s.x[2]) + s.x[3] * s.x[3]);
            cost = cost_new;
            if (gmax(s.bc) <= gtol) {
              term = 3;
              s.cmd = 1;
            } else {
              take(s.bc);
              const double t = 2.0 * rho - 1.0;
              radius = fmin(1e16, radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
              dec = 2.0;
              reuse = false;
            }
          } else {
            radius /= dec;
            dec *= 2.0;
            reuse = true;
          }
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    if (id == 1) {  // PWP:560-579, also after an empty fit (the SVD plane, no residual block)
      double pl[4] = {s.x[0], s.x[1], s.x[2], s.x[3]};
      if (pl[2] < 0)
        for (int a = 0; a < 4; ++a) pl[a] = -pl[a];
      const double nn = sqrt(pl[0] * pl[0] + pl[1] * pl[1] + pl[2] * pl[2]);
      for (int a = 0; a < 4; ++a) pl[a] /= nn;
      s.normal[0] = (float)pl[0];
      s.normal[1] = (float)pl[1];
      s.normal[2] = (float)pl[2];
      s.d = (float)pl[3];
    }
    m_out = m;
    it_out = iters;
    term_out = term;
  }
  __syncthreads();
}

__device__ __forceinline__ void store_fit(const FitShared& s, GroundFit& o, int m, int it, int term) {
  for (int q = 0; q < 3; ++q) {
    o.mean[q] = s.mean[q];
    o.sv[q] = s.sv[q];
    o.normal[q] = s.normal[q];
  }
  for (int q = 0; q < 9; ++q) o.cov[q] = s.cov[q];
  o.d = s.d;
  o.m = m;
  o.iters = it;
  o.term = term;
}

__device__ __forceinline__ unsigned long long z_key(float z, int idx) {  // (z, index) ascending; -0 sorts with +0 as a.z < b.z treats them
  unsigned int u = __float_as_uint(z == 0.0f ? 0.0f : z);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned int)idx;
}

__device__ void bitonic_sort(unsigned long long* a, int L) {  // L a power of two; all 256 lanes
  for (int k = 2; k <= L; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < L; i += 256) {
        const int ij = i ^ j;
        if (ij > i) {
          const unsigned long long ai = a[i], aj = a[ij];
          const bool up = (i & k) == 0;
          if ((ai > aj) == up) {
            a[i] = aj;
            a[ij] = ai;
          }
        }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ int pow2_at_least(int c) {
  int L = 1;
  while (L < c) L <<= 1;
  return L;
}

// ------------------------------------------------------------------------------------------------ per-patch chain (PWP:727-776, 1024-1128)
// grid = patches of all scans (blk[b] = {scan, patch}), block 256.  Rewrites the patch's segment of seg[] in sorted order and sets
// mask[] over it to the final R-GPF selection (regionwise_ground_ = 1, regionwise_nonground_ = 0).
__global__ __launch_bounds__(256) void ground_patch_kernel(const GroundFrame* __restrict__ frames, const int2* __restrict__ blk, const float4* __restrict__ pts,
                                                           const double* __restrict__ C6, int* __restrict__ seg, unsigned char* __restrict__ mask,
                                                           unsigned long long* __restrict__ gkeys, GroundPatch* __restrict__ rec) {
  __shared__ unsigned long long keys[kGroundLdsSort];
  __shared__ FitShared s;
  __shared__ double lpr_s;
  const int2 fb = blk[blockIdx.x];
  const GroundFrame& f = frames[fb.x];
  GroundPatch& R = rec[f.patch_off + fb.y];
  const int count = R.count;
  if (count < f.num_min_pts) {  // PWP:734-738
    if (threadIdx.x == 0) {
      R.n_fits = 0;
      R.n_ground = 0;
    }
    return;
  }
  int* list = seg + f.pt_off + R.seg_off;
  unsigned char* msk = mask + f.pt_off + R.seg_off;
  // std::sort by point_z_cmp (PWP:742), ties by lowest input index
  const int L = pow2_at_least(count);
  unsigned long long* a = keys;
  if (count > kGroundLdsSort) {
    int off = 0;
    for (int p = 0; p < fb.y; ++p) {
      const int c = rec[f.patch_off + p].count;
      if (c > kGroundLdsSort && c >= f.num_min_pts) off += pow2_at_least(c);
    }
    a = gkeys + f.key_off + off;
  }
  for (int k = threadIdx.x; k < L; k += 256) a[k] = k < count ? z_key(pts[f.pt_off + list[k]].z, list[k]) : ~0ull;
  __syncthreads();
  bitonic_sort(a, L);
  for (int k = threadIdx.x; k < count; k += 256) list[k] = (int)(unsigned int)(a[k] & 0xffffffffu);
  __syncthreads();
  float* stage = reinterpret_cast<float*>(keys);  // the LDS keys are dead from here on
  const int zone = fb.y < f.zone_patch_off[1] ? 0 : fb.y < f.zone_patch_off[2] ? 1 : fb.y < f.zone_patch_off[3] ? 2 : 3;
  // extract_initial_seeds, 2-argument form (PWP:621-655)
  int init_idx = 0;
  if (zone == 0) {  // sorted ascending: the leading run below the margin is every point below it
    for (int base = 0; base < count; base += 256) {
      const int k = base + threadIdx.x;
      init_idx += wg_count(k < count && (double)pts[f.pt_off + list[k]].z < f.margin * f.sensor_height, s);
    }
  }
  if (threadIdx.x == 0) {
    double sum = 0;
    int cnt = 0;
    for (int k = init_idx; k < count && cnt < f.num_lpr; ++k) {
      sum += (double)pts[f.pt_off + list[k]].z;
      cnt++;
    }
    lpr_s = cnt != 0 ? sum / cnt : 0;
    for (int q = 0; q < 9; ++q) s.cov[q] = 0.0f;
    for (int q = 0; q < 3; ++q) s.mean[q] = 0.0f;
  }
  __syncthreads();
  const double seed_thr = lpr_s + f.th_seeds;
  for (int k = threadIdx.x; k < count; k += 256) msk[k] = (double)pts[f.pt_off + list[k]].z < seed_thr ? 1 : 0;
  __syncthreads();
  int m, it, term;
  fit_plane(list, msk, count, pts, f.pt_off, C6, f.id, stage, s, m, it, term);
  if (threadIdx.x == 0) {
    R.m[0] = m;
    R.iters[0] = it;
    R.term[0] = term;
  }
  // R-GPF (PWP:1086-1127): float distance ((x n0) + (y n1)) + (z n2), compared in double
  const double zmax = -f.sensor_height + 0.5;
  for (int i = 0; i < f.num_iter; ++i) {
    const float n0 = s.normal[0], n1 = s.normal[1], n2 = s.normal[2];
    const double dthr = f.th_dist - (double)s.d;
    __syncthreads();
    for (int k = threadIdx.x; k < count; k += 256) {
      const float4 p = pts[f.pt_off + list[k]];
      float res = p.x * n0;
      res = res + p.y * n1;
      res = res + p.z * n2;
      msk[k] = ((double)res < dthr && (double)p.z < zmax) ? 1 : 0;
    }
    __syncthreads();
    fit_plane(list, msk, count, pts, f.pt_off, C6, f.id, stage, s, m, it, term);
    if (threadIdx.x == 0) {
      R.m[i + 1] = m;
      R.iters[i + 1] = it;
      R.term[i + 1] = term;
    }
  }
  if (threadIdx.x == 0) {
    R.n_fits = f.num_iter + 1;
    R.n_ground = m;
    store_fit(s, R.last, m, it, term);
  }
}

// ------------------------------------------------------------------------------------------------ final plane (PWP:866-867)
// grid scans, block 256: the plane over cloud_ground (glist, in cloud_ground order), starting from the stale pc_mean_ / cov_ the host
// picked for an empty cloud_ground.
__global__ __launch_bounds__(256) void ground_final_fit_kernel(const GroundFrame* __restrict__ frames, const GroundFinal* __restrict__ jobs, const int* __restrict__ glist,
                                                               const float4* __restrict__ pts, const double* __restrict__ C6, GroundFit* __restrict__ out) {
  __shared__ float stage[3 * 256];
  __shared__ FitShared s;
  const GroundFrame& f = frames[blockIdx.x];
  const GroundFinal& j = jobs[blockIdx.x];
  if (threadIdx.x == 0) {
    for (int q = 0; q < 9; ++q) s.cov[q] = j.stale_cov[q];
    for (int q = 0; q < 3; ++q) s.mean[q] = j.stale_mean[q];
  }
  __syncthreads();
  int m, it, term;
  fit_plane(glist + j.list_off, nullptr, j.count, pts, f.pt_off, C6, j.id, stage, s, m, it, term);
  if (threadIdx.x == 0) store_fit(s, out[blockIdx.x], m, it, term);
}

// ------------------------------------------------------------------------------------------------ a scan that is already on the device
// The scan pipeline (include/gorio_scan.h) keeps its cloud as float columns on the device.  grid ceil(n / 256), block 256.
__global__ __launch_bounds__(256) void ground_pack_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const float* __restrict__ inten, int n,
                                                          float4* __restrict__ pts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) pts[i] = make_float4(x[i], y[i], z[i], inten[i]);
}

// PWP:872-884, the test only: below[i] = (normal . p_i + d < -1) in double on the float plane, the products summed left to right as the host
// loop of ground_run sums them (the library is built with floating-point contraction off).  The erase order stays on the host.
__global__ __launch_bounds__(256) void ground_below_kernel(const float4* __restrict__ pts, int n, const GroundFit* __restrict__ fit, unsigned char* __restrict__ below) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const double x = p.x, y = p.y, z = p.z;
  const double dist = fit->normal[0] * x + fit->normal[1] * y + fit->normal[2] * z + fit->d;
  below[i] = dist < -1.0 ? 1 : 0;
}


// one scan as float columns on the device (the scan pipeline): ground_run then reads no host point and uploads none
struct GroundDeviceScan {
  const float *x, *y, *z, *inten;
};

// ground_pack_kernel / ground_below_kernel for the frames of a batch of device scans: grid (ceil(max n / 256), frames), block 256; frame
// blockIdx.y packs into / tests its own stretch of pts and tests against its own fit.  The arithmetic is that of the single kernels.
__global__ __launch_bounds__(256) void ground_pack_frames_kernel(const GroundFrame* __restrict__ frames, const GroundDeviceScan* __restrict__ scans, float4* __restrict__ pts) {
  const GroundFrame& f = frames[blockIdx.y];
  const GroundDeviceScan s = scans[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < f.n) pts[f.pt_off + i] = make_float4(s.x[i], s.y[i], s.z[i], s.inten[i]);
}
__global__ __launch_bounds__(256) void ground_below_frames_kernel(const GroundFrame* __restrict__ frames, const float4* __restrict__ pts, const GroundFit* __restrict__ fits,
                                                                  unsigned char* __restrict__ below) {
  const GroundFrame& f = frames[blockIdx.y];
  const GroundFit* fit = fits + blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  const float4 p = pts[f.pt_off + i];
  const double x = p.x, y = p.y, z = p.z;
  const double dist = fit->normal[0] * x + fit->normal[1] * y + fit->normal[2] * z + fit->d;
  below[f.pt_off + i] = dist < -1.0 ? 1 : 0;
}

}  // namespace gorio
using gorio::GroundDeviceScan;

// ================================================================================================ host side (include/gorio_ground.h)
#include "../../include/gorio_ground.h"

struct gorio_ground {
  int device = 0;
  hipStream_t stream = nullptr;
  gorio_ground_params p;
  int n_patches = 0;
  int zone_patch_off[4] = {0, 0, 0, 0}, ring_off[4] = {0, 0, 0, 0};
  double min_ranges[4], ring_sizes[4], sector_sizes[4];
  // adaptive state (PWP:380-381, 393-394, 344)
  double elevation_thr[4], flatness_thr[4], sensor_height;
  std::vector<double> upd_elev[4], upd_flat[4];
  float last_mean[3] = {0, 0, 0}, last_cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // pc_mean_ / cov_ of the last estimate in sequential order
  // device buffers (a batch uses the first handle's)
  gorio::DevBuf<float4> d_pts;  // per point: one group of capacity pt_cap
  gorio::DevBuf<int> d_pid, d_seg, d_glist;
  gorio::DevBuf<unsigned char> d_mask;
  gorio::DevBuf<double> d_C6;
  gorio::DevBuf<unsigned long long> d_keys;
  size_t pt_cap = 0;
  gorio::DevBuf<gorio::GroundPatch> d_rec;  // per patch: one group of capacity rec_cap
  gorio::DevBuf<int2> d_blk;
  size_t rec_cap = 0;
  gorio::DevBuf<gorio::GroundFrame> d_frames;  // per frame of a batch: one group of capacity frame_cap
  gorio::DevBuf<gorio::GroundFinal> d_final;
  gorio::DevBuf<gorio::GroundFit> d_fit;
  gorio::DevBuf<gorio::GroundDeviceScan> d_scans;  // a batch of device scans: the column pointers of every frame
  size_t frame_cap = 0;
  // diagnostics of the last estimate
  gorio_ground_frame_diag fdiag;
  std::vector<gorio_ground_patch_diag> pdiag;
  std::vector<int> label, order;
};

namespace {
thread_local std::string g_ground_err;
int ground_fail(int code, const std::string& m) {
  g_ground_err = m;
  return code;
}

int ground_check_params(const gorio_ground_params& p) {
  if (p.enable_RVPF) return ground_fail(GORIO_ERR_INVALID, "enable_RVPF is not supported (off in the reference and in every caller)");
  if (p.num_iter < 1 || p.num_iter > GORIO_GROUND_MAX_FITS - 1) return ground_fail(GORIO_ERR_INVALID, "num_iter must be in [1, 8]");
  if (p.num_min_pts < 1) return ground_fail(GORIO_ERR_INVALID, "num_min_pts must be >= 1");
  // PWP:646-653: with num_lpr = 0 the LPR height is 0, and with th_seeds <= 0 not even the lowest point lies below it + th_seeds
  if (p.num_lpr < 1 || !(p.th_seeds > 0))
    return ground_fail(GORIO_ERR_INVALID,
                       "num_lpr must be >= 1 and th_seeds > 0: otherwise a patch can have no seeds, and its empty first fit would read the previous patch's "
                       "pc_mean_ / cov_, which the per-patch kernels do not carry");
  if (!(p.min_range >= 0 && p.min_range < p.max_range)) return ground_fail(GORIO_ERR_INVALID, "need 0 <= min_range < max_range");
  if (p.max_flatness_storage < 0 || p.max_elevation_storage < 0) return ground_fail(GORIO_ERR_INVALID, "storage sizes must be >= 0");
  int np = 0;
  for (int z = 0; z < 4; ++z) {
    if (p.num_sectors_each_zone[z] < 1 || p.num_rings_each_zone[z] < 1) return ground_fail(GORIO_ERR_INVALID, "every zone needs >= 1 ring and >= 1 sector");
    np += p.num_sectors_each_zone[z] * p.num_rings_each_zone[z];
    if (np > gorio::kGroundMaxPatches) return ground_fail(GORIO_ERR_INVALID, "at most 512 patches");
  }
  return GORIO_OK;
}

void ground_geometry(gorio_ground* h) {  // constructor, PWP:254-272
  const gorio_ground_params& p = h->p;
  const double z2 = (7 * p.min_range + p.max_range) / 8.0, z3 = (3 * p.min_range + p.max_range) / 4.0, z4 = (p.min_range + p.max_range) / 2.0;
  const double mr[4] = {p.min_range, z2, z3, z4};
  const double rs[4] = {(z2 - p.min_range) / p.num_rings_each_zone[0], (z3 - z2) / p.num_rings_each_zone[1], (z4 - z3) / p.num_rings_each_zone[2],
                        (p.max_range - z4) / p.num_rings_each_zone[3]};
  int po = 0, ro = 0;
  for (int z = 0; z < 4; ++z) {
    h->min_ranges[z] = mr[z];
    h->ring_sizes[z] = rs[z];
    h->sector_sizes[z] = 2 * M_PI / p.num_sectors_each_zone[z];
    h->zone_patch_off[z] = po;
    h->ring_off[z] = ro;
    po += p.num_sectors_each_zone[z] * p.num_rings_each_zone[z];
    ro += p.num_rings_each_zone[z];
  }
  h->n_patches = po;
}

// calc_mean_stdev, PWP:1131-1140: nothing written for 0 or 1 values; stdev accumulates onto the caller's value
void calc_mean_stdev(const std::vector<double>& v, double& mean, double& stdev) {
  if (v.size() <= 1) return;
  double s = 0.0;
  for (double a : v) s += a;
  mean = s / v.size();
  for (size_t i = 0; i < v.size(); i++) stdev += (v[i] - mean) * (v[i] - mean);
  stdev /= v.size() - 1;
  stdev = sqrt(stdev);
}

struct Candidate {
  int patch;
  double flatness, line_variable;
  std::vector<int> ground;
};

// Everything after the per-patch chain up to the final fit, for one scan: decisions, A-GLE pushes, TGR, threshold updates.
void ground_decide(gorio_ground* h, const gorio::GroundPatch* rec, const int* pid, const int* seg, const unsigned char* mask, int n, std::vector<int>& ground,
                   std::vector<int>& nonground) {
  const gorio_ground_params& p = h->p;
  ground.clear();
  nonground.clear();
  h->pdiag.assign(h->n_patches, gorio_ground_patch_diag{});
  int n_noise = 0, n_oor = 0;
  for (int i = 0; i < n; ++i)  // RNR noise first (PWP:664-668), then what pc2czm leaves out (PWP:1182-1184)
    if (pid[i] == -2) nonground.push_back(i), ++n_noise;
  for (int i = 0; i < n; ++i)
    if (pid[i] == -1) nonground.push_back(i), ++n_oor;
  std::vector<Candidate> candidates;
  std::vector<double> ringwise_flatness;
  int concentric_idx = 0;
  for (int zone = 0; zone < 4; ++zone) {
    const int S = p.num_sectors_each_zone[zone];
    for (int ring = 0; ring < p.num_rings_each_zone[zone]; ++ring) {
      for (int sector = 0; sector < S; ++sector) {
        const int pi = h->zone_patch_off[zone] + ring * S + sector;
        const gorio::GroundPatch& R = rec[pi];
        gorio_ground_patch_diag& D = h->pdiag[pi];
        D.zone = zone;
        D.ring = ring;
        D.sector = sector;
        D.concentric_idx = concentric_idx;
        D.n_points = R.count;
        D.segment_offset = R.seg_off;
        const int* list = seg + R.seg_off;
        if (R.count < p.num_min_pts) {  // PWP:734-738
          D.decision = GORIO_GROUND_SKIPPED;
          nonground.insert(nonground.end(), list, list + R.count);
          continue;
        }
        const gorio::GroundFit& F = R.last;
        std::memcpy(h->last_mean, F.mean, sizeof(F.mean));
        std::memcpy(h->last_cov, F.cov, sizeof(F.cov));
        std::vector<int> rg, rn;
        for (int k = 0; k < R.count; ++k) (mask[R.seg_off + k] ? rg : rn).push_back(list[k]);
        // PWP:751-756
        const double uprightness = F.normal[2], elevation = F.mean[2];
        const double flatness = (double)fminf(fminf(F.sv[0], F.sv[1]), F.sv[2]);
        const double line_variable = F.sv[1] != 0 ? (double)(F.sv[0] / F.sv[1]) : std::numeric_limits<double>::max();
        double heading = 0.0;
        for (int i = 0; i < 3; i++) heading += F.mean[i] * F.normal[i];
        D.n_ground = (int)rg.size();
        D.uprightness = uprightness;
        D.elevation = elevation;
        D.flatness = flatness;
        D.line_variable = line_variable;
        D.heading = heading;
        std::memcpy(D.mean, F.mean, sizeof(F.mean));
        std::memcpy(D.cov, F.cov, sizeof(F.cov));
        std::memcpy(D.singular_values, F.sv, sizeof(F.sv));
        std::memcpy(D.normal, F.normal, sizeof(F.normal));
        D.d = F.d;
        D.n_fits = R.n_fits;
        for (int q = 0; q < R.n_fits; ++q) {
          D.fit_points[q] = R.m[q];
          D.lm_iterations[q] = R.iters[q];
          D.lm_termination[q] = R.term[q];
        }
        // PWP:772-822 (elevation_thr_ / flatness_thr_ are only read for the rings of interest)
        const bool is_near_zone = concentric_idx < GORIO_GROUND_RINGS_OF_INTEREST;
        const bool is_upright = uprightness > p.uprightness_thr;
        const bool is_not_elevated = is_near_zone && elevation < h->elevation_thr[concentric_idx];
        const bool is_flat = is_near_zone && flatness < h->flatness_thr[concentric_idx];
        const bool is_heading_outside = heading < 0.0;
        if (is_upright && is_not_elevated && is_near_zone) {
          h->upd_elev[concentric_idx].push_back(elevation);
          h->upd_flat[concentric_idx].push_back(flatness);
          ringwise_flatness.push_back(flatness);
        }
        if (!is_upright) {
          D.decision = GORIO_GROUND_NOT_UPRIGHT;
          nonground.insert(nonground.end(), rg.begin(), rg.end());
        } else if (!is_near_zone) {
          D.decision = GORIO_GROUND_FAR;
          ground.insert(ground.end(), rg.begin(), rg.end());
        } else if (!is_heading_outside) {
          D.decision = GORIO_GROUND_HEADING;
          nonground.insert(nonground.end(), rg.begin(), rg.end());
        } else if (is_not_elevated || is_flat) {
          D.decision = GORIO_GROUND_FLAT;
          ground.insert(ground.end(), rg.begin(), rg.end());
        } else {
          candidates.push_back(Candidate{pi, flatness, line_variable, rg});
        }
        nonground.insert(nonground.end(), rn.begin(), rn.end());
      }
      if (!candidates.empty()) {  // PWP:838-856; ringwise_flatness is only cleared here
        if (p.enable_TGR) {  // temporal_ground_revert, PWP:952-1018
          double mean_flatness = 0.0, stdev_flatness = 0.0;
          calc_mean_stdev(ringwise_flatness, mean_flatness, stdev_flatness);
          for (const Candidate& c : candidates) {
            const double mu_flatness = mean_flatness + 1.5 * stdev_flatness;
            double prob_flatness = 1 / (1 + exp((c.flatness - mu_flatness) / (mu_flatness / 10)));
            if (c.ground.size() > 1500 && c.flatness < p.th_dist * p.th_dist) prob_flatness = 1.0;
            double prob_line = 1.0;
            if (c.line_variable > 8.0) prob_line = 0.0;
            const bool revert = prob_line * prob_flatness > 0.5;
            if (concentric_idx < GORIO_GROUND_RINGS_OF_INTEREST) {
              h->pdiag[c.patch].decision = revert ? GORIO_GROUND_TGR_REVERT : GORIO_GROUND_TGR_REJECT;
              (revert ? ground : nonground).insert((revert ? ground : nonground).end(), c.ground.begin(), c.ground.end());
            }
          }
        } else {
          for (const Candidate& c : candidates) {
            h->pdiag[c.patch].decision = GORIO_GROUND_TGR_REJECT;
            nonground.insert(nonground.end(), c.ground.begin(), c.ground.end());
          }
        }
        candidates.clear();
        ringwise_flatness.clear();
      }
      concentric_idx++;
    }
  }
  // update_elevation_thr, PWP:894-922
  for (int i = 0; i < GORIO_GROUND_RINGS_OF_INTEREST; i++) {
    if (h->upd_elev[i].empty()) continue;
    double mean = 0.0, stdev = 0.0;
    calc_mean_stdev(h->upd_elev[i], mean, stdev);
    if (i == 0) {
      h->elevation_thr[i] = mean + 3 * stdev;
      h->sensor_height = -mean;
    } else
      h->elevation_thr[i] = mean + 2 * stdev;
    const int exceed = (int)h->upd_elev[i].size() - p.max_elevation_storage;
    if (exceed > 0) h->upd_elev[i].erase(h->upd_elev[i].begin(), h->upd_elev[i].begin() + exceed);
  }
  // update_flatness_thr, PWP:924-950: stops at the first ring with fewer than 2 values
  for (int i = 0; i < GORIO_GROUND_RINGS_OF_INTEREST; i++) {
    if (h->upd_flat[i].empty()) break;
    if (h->upd_flat[i].size() <= 1) break;
    double mean = 0.0, stdev = 0.0;
    calc_mean_stdev(h->upd_flat[i], mean, stdev);
    h->flatness_thr[i] = mean + stdev;
    const int exceed = (int)h->upd_flat[i].size() - p.max_flatness_storage;
    if (exceed > 0) h->upd_flat[i].erase(h->upd_flat[i].begin(), h->upd_flat[i].begin() + exceed);
  }
  h->fdiag = gorio_ground_frame_diag{};
  h->fdiag.n_points = n;
  h->fdiag.n_noise = n_noise;
  h->fdiag.n_out_of_range = n_oor;
  h->fdiag.n_patches = h->n_patches;
  h->fdiag.n_ground = (int)ground.size();
}

// dev != nullptr: scan q is dev[q], its coordinates finite by construction; xyz / inten / stride are not read.  One device scan takes the
// single pack and under-ground kernels, several take their per-frame forms: one launch each, whatever the count.
int ground_run(gorio_ground* const* hs, int count, const float* const* xyz, const float* const* inten, const int* n, const int* stride, int id, int* const* order_out,
               int* n_ground, int* n_out, const GroundDeviceScan* dev = nullptr) {
  if (!hs || count <= 0 || (!dev && (!xyz || !inten || !stride)) || !n || !order_out || !n_ground || !n_out) return ground_fail(GORIO_ERR_INVALID, "estimate: null argument");
  if (id != 0 && id != 1) return ground_fail(GORIO_ERR_INVALID, "estimate: id must be 0 (estimate_plane) or 1 (estimate_plane_cov)");
  gorio_ground* lead = hs[0];
  if (!lead) return ground_fail(GORIO_ERR_INVALID, "estimate: null handle at index 0");
  std::unordered_set<const gorio_ground*> distinct;
  size_t ntot = 0, ptot = 0;
  for (int q = 0; q < count; ++q) {
    const std::string at = count > 1 ? " (batch index " + std::to_string(q) + ")" : "";
    if (!hs[q]) return ground_fail(GORIO_ERR_INVALID, "estimate: null handle" + at);
    if (hs[q]->device != lead->device) return ground_fail(GORIO_ERR_INVALID, "estimate: all handles of a batch must live on one device" + at);
    if (!distinct.insert(hs[q]).second) return ground_fail(GORIO_ERR_INVALID, "estimate: the same handle appears twice in a batch" + at);
    if (dev ? (!order_out[q] || n[q] <= 0) : (!xyz[q] || !inten[q] || !order_out[q] || n[q] <= 0 || stride[q] < 12 || stride[q] % 4))
      return ground_fail(GORIO_ERR_INVALID, "estimate: bad cloud arguments" + at);
    const size_t st = dev ? 0 : stride[q] / 4;
    for (int i = 0; !dev && i < n[q]; ++i) {
      const float* pt = xyz[q] + st * i;
      if (!std::isfinite(pt[0]) || !std::isfinite(pt[1]) || !std::isfinite(pt[2])) return ground_fail(GORIO_ERR_INVALID, "estimate: non-finite coordinate at point " + std::to_string(i) + at);
    }
    ntot += n[q];
    ptot += hs[q]->n_patches;
  }
  if (ntot > (size_t)INT_MAX / 2) return ground_fail(GORIO_ERR_INVALID, "estimate: too many points");
  GORIO_HIP_CHECK(ground_fail, hipSetDevice(lead->device));
  {
    const size_t cap = ntot + ntot / 4;
    GORIO_HIP_CHECK(ground_fail, gorio::reserve_group(lead->pt_cap, ntot, cap, lead->d_pts, cap, lead->d_pid, cap, lead->d_seg, cap, lead->d_glist, cap, lead->d_mask, cap, lead->d_C6, 6 * cap,
                                    lead->d_keys, 2 * cap));
  }
  GORIO_HIP_CHECK(ground_fail, gorio::reserve_group(lead->rec_cap, ptot, ptot, lead->d_rec, ptot, lead->d_blk, ptot));
  GORIO_HIP_CHECK(ground_fail, gorio::reserve_group(lead->frame_cap, count, count, lead->d_frames, count, lead->d_final, count, lead->d_fit, count, lead->d_scans, count));
  std::vector<float4> pts(dev ? 0 : ntot);
  std::vector<gorio::GroundFrame> fr(count);
  std::vector<int2> blk;
  blk.reserve(ptot);
  int pt_off = 0, patch_off = 0, max_n = 0;
  for (int q = 0; q < count; ++q) {
    const gorio_ground* h = hs[q];
    const size_t st = dev ? 0 : stride[q] / 4, si = st;
    for (int i = 0; !dev && i < n[q]; ++i) {
      const float* pt = xyz[q] + st * i;
      pts[pt_off + i] = make_float4(pt[0], pt[1], pt[2], inten[q][si * i]);
    }
    gorio::GroundFrame& f = fr[q];
    f.pt_off = pt_off;
    f.n = n[q];
    f.patch_off = patch_off;
    f.n_patches = h->n_patches;
    f.key_off = 2 * pt_off;
    f.num_iter = h->p.num_iter;
    f.num_lpr = h->p.num_lpr;
    f.num_min_pts = h->p.num_min_pts;
    f.id = id;
    f.enable_rnr = h->p.enable_RNR;
    f.sensor_height = h->sensor_height;
    f.th_seeds = h->p.th_seeds;
    f.th_dist = h->p.th_dist;
    f.margin = h->p.adaptive_seed_selection_margin;
    f.min_range = h->p.min_range;
    f.max_range = h->p.max_range;
    f.rnr_angle = h->p.RNR_ver_angle_thr;
    f.rnr_intensity = h->p.RNR_intensity_thr;
    for (int z = 0; z < 4; ++z) {
      f.min_ranges[z] = h->min_ranges[z];
      f.ring_sizes[z] = h->ring_sizes[z];
      f.sector_sizes[z] = h->sector_sizes[z];
      f.sectors[z] = h->p.num_sectors_each_zone[z];
      f.rings[z] = h->p.num_rings_each_zone[z];
      f.zone_patch_off[z] = h->zone_patch_off[z];
    }
    for (int p = 0; p < h->n_patches; ++p) blk.push_back(make_int2(q, p));
    pt_off += n[q];
    patch_off += h->n_patches;
    max_n = std::max(max_n, n[q]);
  }
  hipStream_t st = lead->stream;
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_frames, fr.data(), sizeof(gorio::GroundFrame) * count, hipMemcpyHostToDevice, st));
  if (dev && count == 1) {
    gorio::ground_pack_kernel<<<(n[0] + 255) / 256, 256, 0, st>>>(dev->x, dev->y, dev->z, dev->inten, n[0], lead->d_pts);
    GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  } else if (dev) {
    GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_scans, dev, sizeof(GroundDeviceScan) * count, hipMemcpyHostToDevice, st));
    gorio::ground_pack_frames_kernel<<<dim3((max_n + 255) / 256, count), 256, 0, st>>>(lead->d_frames, lead->d_scans, lead->d_pts);
    GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  } else {
    GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_pts, pts.data(), sizeof(float4) * ntot, hipMemcpyHostToDevice, st));
  }
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_blk, blk.data(), sizeof(int2) * ptot, hipMemcpyHostToDevice, st));
  gorio::ground_classify_kernel<<<dim3((max_n + 255) / 256, count), 256, 0, st>>>(lead->d_frames, lead->d_pts, lead->d_pid, lead->d_C6);
  GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  gorio::ground_segment_kernel<<<count, 1024, 0, st>>>(lead->d_frames, lead->d_pid, lead->d_seg, lead->d_rec);
  GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  gorio::ground_patch_kernel<<<(unsigned)ptot, 256, 0, st>>>(lead->d_frames, lead->d_blk, lead->d_pts, lead->d_C6, lead->d_seg, lead->d_mask, lead->d_keys, lead->d_rec);
  GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  std::vector<int> pid(ntot), seg(ntot);
  std::vector<unsigned char> mask(ntot);
  std::vector<gorio::GroundPatch> rec(ptot);
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(pid.data(), lead->d_pid, sizeof(int) * ntot, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(seg.data(), lead->d_seg, sizeof(int) * ntot, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(mask.data(), lead->d_mask, ntot, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(rec.data(), lead->d_rec, sizeof(gorio::GroundPatch) * ptot, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(ground_fail, hipStreamSynchronize(st));
  std::vector<std::vector<int>> grounds(count), nongrounds(count);
  std::vector<gorio::GroundFinal> fin(count);
  std::vector<int> glist;
  for (int q = 0; q < count; ++q) {
    gorio_ground* h = hs[q];
    const gorio::GroundFrame& f = fr[q];
    ground_decide(h, rec.data() + f.patch_off, pid.data() + f.pt_off, seg.data() + f.pt_off, mask.data() + f.pt_off, f.n, grounds[q], nongrounds[q]);
    h->label.assign(pid.begin() + f.pt_off, pid.begin() + f.pt_off + f.n);
    const gorio::GroundPatch* R = rec.data() + f.patch_off;
    int used = 0;
    for (int p = 0; p < h->n_patches; ++p) used = std::max(used, R[p].seg_off + R[p].count);
    h->order.assign(f.n, -1);
    std::copy(seg.begin() + f.pt_off, seg.begin() + f.pt_off + used, h->order.begin());
    fin[q].list_off = (int)glist.size();
    fin[q].count = (int)grounds[q].size();
    fin[q].id = id;
    std::memcpy(fin[q].stale_mean, h->last_mean, sizeof(h->last_mean));
    std::memcpy(fin[q].stale_cov, h->last_cov, sizeof(h->last_cov));
    glist.insert(glist.end(), grounds[q].begin(), grounds[q].end());
  }
  if (!glist.empty()) GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_glist, glist.data(), sizeof(int) * glist.size(), hipMemcpyHostToDevice, st));
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(lead->d_final, fin.data(), sizeof(gorio::GroundFinal) * count, hipMemcpyHostToDevice, st));
  gorio::ground_final_fit_kernel<<<count, 256, 0, st>>>(lead->d_frames, lead->d_final, lead->d_glist, lead->d_pts, lead->d_C6, lead->d_fit);
  GORIO_HIP_CHECK(ground_fail, hipGetLastError());
  std::vector<gorio::GroundFit> fits(count);
  GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(fits.data(), lead->d_fit, sizeof(gorio::GroundFit) * count, hipMemcpyDeviceToHost, st));
  std::vector<unsigned char> below;  // a device scan: the under-ground test of every point (d_mask is free again, its patch flags are on the host)
  if (dev) {
    below.resize(ntot);
    if (count == 1) gorio::ground_below_kernel<<<(n[0] + 255) / 256, 256, 0, st>>>(lead->d_pts, n[0], lead->d_fit, lead->d_mask);
    else gorio::ground_below_frames_kernel<<<dim3((max_n + 255) / 256, count), 256, 0, st>>>(lead->d_frames, lead->d_pts, lead->d_fit, lead->d_mask);
    GORIO_HIP_CHECK(ground_fail, hipGetLastError());
    GORIO_HIP_CHECK(ground_fail, hipMemcpyAsync(below.data(), lead->d_mask, ntot, hipMemcpyDeviceToHost, st));
  }
  GORIO_HIP_CHECK(ground_fail, hipStreamSynchronize(st));
  for (int q = 0; q < count; ++q) {
    gorio_ground* h = hs[q];
    const gorio::GroundFit& F = fits[q];
    const int n_tot = n[q];
    std::memcpy(h->last_mean, F.mean, sizeof(F.mean));
    std::memcpy(h->last_cov, F.cov, sizeof(F.cov));
    gorio_ground_frame_diag& D = h->fdiag;
    D.final_fit_points = F.m;
    D.final_lm_iterations = F.iters;
    D.final_lm_termination = F.term;
    std::memcpy(D.final_mean, F.mean, sizeof(F.mean));
    std::memcpy(D.final_cov, F.cov, sizeof(F.cov));
    std::memcpy(D.final_singular_values, F.sv, sizeof(F.sv));
    std::memcpy(D.final_normal, F.normal, sizeof(F.normal));
    D.final_d = F.d;
    // PWP:872-884: erase(begin + i) while i still advances, so the point after an erased one is never tested
    std::vector<int>& ng = nongrounds[q];
    for (size_t i = 0; dev && i < ng.size(); ++i)
      if (below[fr[q].pt_off + ng[i]]) ng.erase(ng.begin() + i);
    const float* base = dev ? nullptr : xyz[q];
    const size_t sp = dev ? 0 : stride[q] / 4;
    for (size_t i = 0; !dev && i < ng.size(); ++i) {
      const float* pt = base + sp * ng[i];
      const double x = pt[0], y = pt[1], z = pt[2];
      const double dist = F.normal[0] * x + F.normal[1] * y + F.normal[2] * z + F.d;
      if (dist < -1.0) ng.erase(ng.begin() + i);
    }
    const std::vector<int>& g = grounds[q];
    std::copy(g.begin(), g.end(), order_out[q]);
    std::copy(ng.begin(), ng.end(), order_out[q] + g.size());
    n_ground[q] = (int)g.size();
    n_out[q] = (int)(g.size() + ng.size());
    D.n_erased = n_tot - n_out[q];
  }
  return GORIO_OK;
}
}  // namespace

extern "C" {

const char* gorio_ground_last_error(void) { return g_ground_err.c_str(); }

void gorio_ground_default_params(gorio_ground_params* p) {  // Params(), PWP:127-168, verbose off as in PREP:100-102
  if (!p) return;
  *p = gorio_ground_params{};
  p->enable_RNR = 1;
  p->enable_RVPF = 0;
  p->enable_TGR = 1;
  p->num_iter = 4;
  p->num_lpr = 20;
  p->num_min_pts = 10;
  p->RNR_ver_angle_thr = -15.0;
  p->RNR_intensity_thr = 0.1;
  p->sensor_height = 0.7;
  p->th_seeds = 0.5;
  p->th_dist = 1.0;
  p->th_seeds_v = 0.25;
  p->th_dist_v = 2.0;
  p->max_range = 50.0;
  p->min_range = 1.0;
  p->uprightness_thr = 0.5;
  p->adaptive_seed_selection_margin = -1.2;
  const int sec[4] = {3, 1, 1, 3}, rings[4] = {4, 4, 2, 2};
  for (int z = 0; z < 4; ++z) {
    p->num_sectors_each_zone[z] = sec[z];
    p->num_rings_each_zone[z] = rings[z];
    p->elevation_thr[z] = 0;
    p->flatness_thr[z] = 0;
  }
  p->max_flatness_storage = 1000;
  p->max_elevation_storage = 1000;
}

int gorio_ground_create(gorio_ground_t** out, int device, const gorio_ground_params* p) {
  if (!out || !p) return ground_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  const int rc = ground_check_params(*p);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ground_fail(GORIO_ERR_NO_DEVICE, "create: no usable HIP device (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return ground_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  GORIO_HIP_CHECK(ground_fail, hipSetDevice(device));
  gorio_ground* h = new (std::nothrow) gorio_ground();
  if (!h) return ground_fail(GORIO_ERR_ALLOC, "create: out of memory");
  h->device = device;
  h->p = *p;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return ground_fail(GORIO_ERR_NO_DEVICE, "create: no stream");
  }
  ground_geometry(h);
  for (int z = 0; z < 4; ++z) {
    h->elevation_thr[z] = p->elevation_thr[z];
    h->flatness_thr[z] = p->flatness_thr[z];
  }
  h->sensor_height = p->sensor_height;
  *out = h;
  return GORIO_OK;
}

void gorio_ground_destroy(gorio_ground_t* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int gorio_ground_estimate(gorio_ground_t* h, const float* xyz, const float* intensity, int n, int stride_bytes, int id, int* order_out, int* n_ground, int* n_out) {
  gorio_ground_t* const hs[1] = {h};
  return ground_run(hs, 1, &xyz, &intensity, &n, &stride_bytes, id, &order_out, n_ground, n_out);
}

int gorio_ground_estimate_batch(gorio_ground_t* const* handles, int count, const float* const* xyz, const float* const* intensity, const int* n, const int* stride_bytes,
                                int id, int* const* order_out, int* n_ground, int* n_out) {
  return ground_run(handles, count, xyz, intensity, n, stride_bytes, id, order_out, n_ground, n_out);
}

int gorio_ground_get_state(const gorio_ground_t* h, double elevation_thr[4], double flatness_thr[4], double* sensor_height, double* elevation_storage,
                           int elevation_count[4], double* flatness_storage, int flatness_count[4], int storage_stride) {
  if (!h) return ground_fail(GORIO_ERR_INVALID, "get_state: null handle");
  for (int r = 0; r < 4; ++r) {
    if (elevation_thr) elevation_thr[r] = h->elevation_thr[r];
    if (flatness_thr) flatness_thr[r] = h->flatness_thr[r];
    if (elevation_count) elevation_count[r] = (int)h->upd_elev[r].size();
    if (flatness_count) flatness_count[r] = (int)h->upd_flat[r].size();
  }
  if (sensor_height) *sensor_height = h->sensor_height;
  for (int r = 0; r < 4; ++r) {
    if ((elevation_storage && (int)h->upd_elev[r].size() > storage_stride) || (flatness_storage && (int)h->upd_flat[r].size() > storage_stride))
      return ground_fail(GORIO_ERR_INVALID, "get_state: a storage is longer than storage_stride");
    if (elevation_storage) std::copy(h->upd_elev[r].begin(), h->upd_elev[r].end(), elevation_storage + (size_t)r * storage_stride);
    if (flatness_storage) std::copy(h->upd_flat[r].begin(), h->upd_flat[r].end(), flatness_storage + (size_t)r * storage_stride);
  }
  return GORIO_OK;
}

int gorio_ground_set_state(gorio_ground_t* h, const double elevation_thr[4], const double flatness_thr[4], double sensor_height, const double* elevation_storage,
                           const int elevation_count[4], const double* flatness_storage, const int flatness_count[4], int storage_stride) {
  if (!h || !elevation_thr || !flatness_thr || !elevation_count || !flatness_count) return ground_fail(GORIO_ERR_INVALID, "set_state: null argument");
  for (int r = 0; r < 4; ++r) {
    if (elevation_count[r] < 0 || flatness_count[r] < 0 || elevation_count[r] > storage_stride || flatness_count[r] > storage_stride)
      return ground_fail(GORIO_ERR_INVALID, "set_state: counts must be in [0, storage_stride]");
    if ((elevation_count[r] && !elevation_storage) || (flatness_count[r] && !flatness_storage)) return ground_fail(GORIO_ERR_INVALID, "set_state: null storage");
  }
  for (int r = 0; r < 4; ++r) {
    h->elevation_thr[r] = elevation_thr[r];
    h->flatness_thr[r] = flatness_thr[r];
    h->upd_elev[r].assign(elevation_count[r] ? elevation_storage + (size_t)r * storage_stride : nullptr,
                          elevation_count[r] ? elevation_storage + (size_t)r * storage_stride + elevation_count[r] : nullptr);
    h->upd_flat[r].assign(flatness_count[r] ? flatness_storage + (size_t)r * storage_stride : nullptr,
                          flatness_count[r] ? flatness_storage + (size_t)r * storage_stride + flatness_count[r] : nullptr);
  }
  h->sensor_height = sensor_height;
  return GORIO_OK;
}

int gorio_ground_get_diagnostics(const gorio_ground_t* h, gorio_ground_frame_diag* frame, gorio_ground_patch_diag* patches, int patch_capacity, int* point_label,
                                 int* patch_order, int n_points) {
  if (!h) return ground_fail(GORIO_ERR_INVALID, "get_diagnostics: null handle");
  if (h->label.empty()) return ground_fail(GORIO_ERR_STATE, "get_diagnostics: no estimate yet");
  if (frame) *frame = h->fdiag;
  if (patches) {
    if (patch_capacity < h->n_patches) return ground_fail(GORIO_ERR_INVALID, "get_diagnostics: patch_capacity below the patch count");
    std::copy(h->pdiag.begin(), h->pdiag.end(), patches);
  }
  if ((point_label || patch_order) && n_points != (int)h->label.size()) return ground_fail(GORIO_ERR_INVALID, "get_diagnostics: n_points is not the last scan's size");
  if (point_label) std::copy(h->label.begin(), h->label.end(), point_label);
  if (patch_order) std::copy(h->order.begin(), h->order.end(), patch_order);
  return GORIO_OK;
}

}  // extern "C"
