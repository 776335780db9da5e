// apd_gicp_omp.hip -- GICP_OMP (pclomp::GeneralizedIterativeClosestPoint, REG:91-100) as method GORIO_METHOD_GICP_OMP of the registration
// handle.  Included at the end of apd_api.hip: upload, search index, k-NN lists, 1-NN search, fitness score and hand-offs are the handle's.
//   GOH = ndt_omp/include/pclomp/gicp_omp.h, GO = ndt_omp/include/pclomp/gicp_omp_impl.hpp
//
//   gomp_cov_kernel       covariances from the k-NN lists: float products summed in double, SVD rebuild with (1, 1, gicp_epsilon)   GO:82-120
//   gomp_output_kernel    output = guess * p in float, once per align, in original and in search-index order                        GO:402
//   gomp_update_kernel    gate, R C1 R^T + C2, cofactor inverse, float Mahalanobis matrix, pairs per block                         GO:441-460
//   gomp_functor_kernel   <0> operator() float path, <1> df, <2> fdf: one launch each, wave -> block -> block order in fp64        GO:249-371
//   gomp_update_batch_kernel, gomp_functor_batch_kernel, gomp_fold_batch_kernel: the same per-workgroup bodies (gomp_update_block,
//                         gomp_functor_block) over a job table -- one pending update or evaluation of one handle per job -- and the sums
//                         of every job's blocks in block order                                          gorio_apd_gicp_omp_align_batch
// The 1-NN search is nn_search_kernel / nn_search_pruned_kernel run on a descriptor whose source view is the `output` copy: the kernels read
// coordinates and nothing else of a source, so the index built for the stored source serves unchanged.
// The BFGS shell (gicp_bfgs.h) and the outer loop of GO:409-516 run on the host as one resumable machine per handle (GompMachine):
// gorio_apd_align drives one, one device evaluation per round trip; gorio_apd_gicp_omp_align_batch drives many in lock-step.
#include "gicp_bfgs.h"

namespace gorio {

struct GompR {
  double r[9];   // 3x3 of the double product transformation_ * guess (GO:417-423), row-major
  double thr2;   // corr_dist_threshold_^2 (GO:401)
};

__global__ __launch_bounds__(256) void gomp_cov_kernel(CloudView c, const int* __restrict__ knn, int k, double eps) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= c.n) return;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0, c00 = 0.0, c10 = 0.0, c11 = 0.0, c20 = 0.0, c21 = 0.0, c22 = 0.0;
  for (int t = 0; t < k; ++t) {
    int j = knn[(size_t)i * k + t];
    j = j < 0 ? 0 : (j >= c.n ? c.n - 1 : j);  // the lists hold indices of this cloud
    const float4 p = c.p4[j];
    m0 += (double)p.x; m1 += (double)p.y; m2 += (double)p.z;
    c00 += (double)(p.x * p.x);  // GO:89-96: float products, double sums
    c10 += (double)(p.y * p.x);
    c11 += (double)(p.y * p.y);
    c20 += (double)(p.z * p.x);
    c21 += (double)(p.z * p.y);
    c22 += (double)(p.z * p.z);
  }
  const double kd = (double)k;
  m0 /= kd; m1 /= kd; m2 /= kd;
  c00 = c00 / kd - m0 * m0;
  c10 = c10 / kd - m1 * m0;
  c11 = c11 / kd - m1 * m1;
  c20 = c20 / kd - m2 * m0;
  c21 = c21 / kd - m2 * m1;
  c22 = c22 / kd - m2 * m2;
  // JacobiSVD of a symmetric matrix: U = eigenvectors ordered by |eigenvalue| descending (the sign of a column cancels in u u^T)
  Eig3 e = sym3_eigen(c00, c10, c20, c11, c21, c22);
  if (fabs(e.w0) < fabs(e.w1)) swap_cols(e.w0, e.w1, e.v00, e.v10, e.v20, e.v01, e.v11, e.v21);
  if (fabs(e.w1) < fabs(e.w2)) swap_cols(e.w1, e.w2, e.v01, e.v11, e.v21, e.v02, e.v12, e.v22);
  if (fabs(e.w0) < fabs(e.w1)) swap_cols(e.w0, e.w1, e.v00, e.v10, e.v20, e.v01, e.v11, e.v21);
  double* o = c.cov6 + (size_t)i * 6;
  o[0] = (e.v00 * e.v00 + e.v01 * e.v01) + eps * e.v02 * e.v02;
  o[1] = (e.v00 * e.v10 + e.v01 * e.v11) + eps * e.v02 * e.v12;
  o[2] = (e.v00 * e.v20 + e.v01 * e.v21) + eps * e.v02 * e.v22;
  o[3] = (e.v10 * e.v10 + e.v11 * e.v11) + eps * e.v12 * e.v12;
  o[4] = (e.v10 * e.v20 + e.v11 * e.v21) + eps * e.v12 * e.v22;
  o[5] = (e.v20 * e.v20 + e.v21 * e.v21) + eps * e.v22 * e.v22;
  c.geo_w[i] = eps;  // sigma_3 / sigma_1 of the rebuilt matrix (read by no GICP_OMP code)
}

// s4_in / s4_out: the source's search-index copy (x, y, z, original index bits) by sorted position, or null (exhaustive search)
__global__ __launch_bounds__(256) void gomp_output_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, TfArg g, float* __restrict__ ox,
                                                          float* __restrict__ oy, float* __restrict__ oz, const float4* __restrict__ s4_in, float4* __restrict__ s4_out, int n_spad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    float a, b, c;
    transform_f(g.m, x[i], y[i], z[i], a, b, c);
    ox[i] = a; oy[i] = b; oz[i] = c;
  }
  if (s4_in && i < n_spad) {
    float4 v = s4_in[i];
    if (i < n) {  // positions >= n are padding
      float a, b, c;
      transform_f(g.m, v.x, v.y, v.z, a, b, c);
      v.x = a; v.y = b; v.z = c;
    }
    s4_out[i] = v;
  }
}

// Consumes (and re-arms) best_key; corr / sqd as linearize_kernel leaves them; maha[i][9] = the float cast of (R C1 R^T + C2)^-1, row-major;
// cnt[0] = pairs of the block's 256 points.  The work of ONE workgroup of 256 lanes on source points [256 block, 256 block + 256) of one
// handle, shared by the single and the batched kernel.
__device__ __forceinline__ void gomp_update_block(unsigned long long* __restrict__ best_key, int n, const double* __restrict__ c1, const double* __restrict__ c2, int n_tgt, const GompR& R,
                                                  int* __restrict__ corr, float* __restrict__ sqd, float* __restrict__ maha, int block, int* __restrict__ cnt) {
  __shared__ int s_cnt[4];
  const int i = block * 256 + threadIdx.x;
  bool pair = false;
  if (i < n) {
    const unsigned long long key = best_key[i];
    best_key[i] = ~0ull;
    const float d = __uint_as_float((unsigned int)(key >> 32));
    int j = (int)(unsigned int)(key & 0xffffffffu);
    const bool found = key != ~0ull && j >= 0 && j < n_tgt;
    sqd[i] = found ? d : INFINITY;
    pair = found && (double)d < R.thr2;  // GO:441
    corr[i] = pair ? j : -1;
    if (pair) {
      const double* a = c1 + (size_t)i * 6;
      const double* b = c2 + (size_t)j * 6;
      const double C1[9] = {a[0], a[1], a[2], a[1], a[3], a[4], a[2], a[4], a[5]};
      double M[9], T[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r * 3 + c] = (R.r[r * 3] * C1[c] + R.r[r * 3 + 1] * C1[3 + c]) + R.r[r * 3 + 2] * C1[6 + c];  // M = R C1
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) T[r * 3 + c] = (M[r * 3] * R.r[c * 3] + M[r * 3 + 1] * R.r[c * 3 + 1]) + M[r * 3 + 2] * R.r[c * 3 + 2];  // M R^T
      T[0] += b[0]; T[1] += b[1]; T[2] += b[2]; T[3] += b[1]; T[4] += b[3]; T[5] += b[4]; T[6] += b[2]; T[7] += b[4]; T[8] += b[5];
      // cofactor inverse: cof(i, j) = T(i+1, j+1) T(i+2, j+2) - T(i+1, j+2) T(i+2, j+1) (indices mod 3); inv(r, c) = cof(c, r) / det, det along column 0
      double cof[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, q1 = (c + 1) % 3, q2 = (c + 2) % 3;
          cof[r * 3 + c] = T[r1 * 3 + q1] * T[r2 * 3 + q2] - T[r1 * 3 + q2] * T[r2 * 3 + q1];
        }
      const double det = (cof[0] * T[0] + cof[3] * T[3]) + cof[6] * T[6];
      const double inv = 1.0 / det;
      float* o = maha + (size_t)i * 9;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) o[r * 3 + c] = (float)(cof[c * 3 + r] * inv);  // GO:456
    }
  }
  const unsigned long long bal = __ballot(pair);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(bal);
  __syncthreads();
  if (threadIdx.x == 0) cnt[0] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// grid: ceil(n / 256), block 256.  cnt[block] = pairs of the block
__global__ __launch_bounds__(256) void gomp_update_kernel(unsigned long long* __restrict__ best_key, int n, const double* __restrict__ c1, const double* __restrict__ c2, int n_tgt, GompR R,
                                                          int* __restrict__ corr, float* __restrict__ sqd, float* __restrict__ maha, int* __restrict__ cnt) {
  gomp_update_block(best_key, n, c1, c2, n_tgt, R, corr, sqd, maha, (int)blockIdx.x, cnt + blockIdx.x);
}

// MODE 0: Sum res . (M res) over the pairs on the float path of operator() (GO:269-275), 1 value.
// MODE 1: df (GO:305-320): Sum temp (3) and Sum p_src3 temp^T (9) on the double path, values [1..12].
// MODE 2: fdf (GO:352-365): the same plus Sum res . temp in [0].
// The work of ONE workgroup of 256 lanes, shared by the single and the batched kernel: source points [256 block, 256 block + 256) of one
// handle, reduced wave -> block (the four waves in a fixed order) into out[V0 .. V1) (13 slots).  s_red: 4 * 13 doubles of LDS.
template <int MODE>
__device__ __forceinline__ void gomp_functor_block(const float* __restrict__ ox, const float* __restrict__ oy, const float* __restrict__ oz, int n, const float4* __restrict__ tgt,
                                                   const int* __restrict__ corr, const float* __restrict__ maha, const TfArg& tf, int block, double* s_red, double* __restrict__ out) {
  constexpr int NV = 13;
  constexpr int V0 = MODE == 1 ? 1 : 0, V1 = MODE == 0 ? 1 : NV;  // the values [V0, V1) this mode produces
  const int i = block * 256 + threadIdx.x;
  double v[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) v[q] = 0.0;
  const int j = i < n ? corr[i] : -1;
  if (j >= 0) {
    const float px = ox[i], py = oy[i], pz = oz[i];
    const float4 t = tgt[j];
    const float* m = maha + (size_t)i * 9;
    float qx, qy, qz;
    transform_f(tf.m, px, py, pz, qx, qy, qz);
    if (MODE == 0) {
      const float r0 = qx - t.x, r1 = qy - t.y, r2 = qz - t.z;
      const float t0 = (m[0] * r0 + m[1] * r1) + m[2] * r2;
      const float t1 = (m[3] * r0 + m[4] * r1) + m[5] * r2;
      const float t2 = (m[6] * r0 + m[7] * r1) + m[8] * r2;
      const float ret = (r0 * t0 + r1 * t1) + r2 * t2;
      v[0] = (double)ret;
    } else {
      const double r0 = (double)(qx - t.x), r1 = (double)(qy - t.y), r2 = (double)(qz - t.z);  // pp[0] - p_tgt[0]: a float difference
      const double t0 = ((double)m[0] * r0 + (double)m[1] * r1) + (double)m[2] * r2;
      const double t1 = ((double)m[3] * r0 + (double)m[4] * r1) + (double)m[5] * r2;
      const double t2 = ((double)m[6] * r0 + (double)m[7] * r1) + (double)m[8] * r2;
      if (MODE == 2) v[0] = (r0 * t0 + r1 * t1) + r2 * t2;
      v[1] = t0; v[2] = t1; v[3] = t2;
      const double p0 = (double)px, p1 = (double)py, p2 = (double)pz;  // base_transformation_ is the identity (GO:398)
      v[4] = p0 * t0; v[5] = p0 * t1; v[6] = p0 * t2;
      v[7] = p1 * t0; v[8] = p1 * t1; v[9] = p1 * t2;
      v[10] = p2 * t0; v[11] = p2 * t1; v[12] = p2 * t2;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = V0; q < V1; ++q) {
    const double s = wave_sum(v[q]);
    if (lane == 0) s_red[wave * NV + q] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x >= V0 && (int)threadIdx.x < V1) {
    const int q = threadIdx.x;
    out[q] = ((s_red[q] + s_red[NV + q]) + s_red[2 * NV + q]) + s_red[3 * NV + q];
  }
}

// One launch: every workgroup reduces its 256 source points and stores one partial; the workgroup that draws the last ticket adds the
// partials in block order into out[0..12].  arrive is zeroed ahead of the launch.
template <int MODE>
__global__ __launch_bounds__(256) void gomp_functor_kernel(const float* __restrict__ ox, const float* __restrict__ oy, const float* __restrict__ oz, int n, const float4* __restrict__ tgt,
                                                           const int* __restrict__ corr, const float* __restrict__ maha, TfArg tf, double* __restrict__ partials,
                                                           unsigned int* __restrict__ arrive, double* __restrict__ out) {
  constexpr int NV = 13;
  constexpr int V0 = MODE == 1 ? 1 : 0, V1 = MODE == 0 ? 1 : NV;
  __shared__ double s_red[4 * NV + 1];
  gomp_functor_block<MODE>(ox, oy, oz, n, tgt, corr, maha, tf, (int)blockIdx.x, s_red, partials + (size_t)blockIdx.x * NV);
  // hand-over to the last workgroup: stores drained, one agent-scope release ahead of the ticket, one acquire behind the last one
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned int ticket = __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = ticket == gridDim.x - 1;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    s_red[4 * NV] = last ? 1.0 : 0.0;
  }
  __syncthreads();
  if (s_red[4 * NV] == 0.0) return;
  if ((int)threadIdx.x >= V0 && (int)threadIdx.x < V1) {
    const int q = threadIdx.x;
    double s = 0.0;
    for (unsigned int b = 0; b < gridDim.x; ++b) s += partials[(size_t)b * NV + q];
    out[q] = s;
  }
}

// One pending request of gorio_apd_gicp_omp_align_batch: an evaluation of the functor (mode 0, 1, 2) or an update (mode 3) of one handle.
// Its workgroups write the partial slots (13 doubles each; one int each for an update) [first, first + nblk).
struct GompJob {
  const float *ox, *oy, *oz;  // the `output` cloud
  const float4* tgt;
  int* corr;
  float* maha;
  // an update only
  unsigned long long* best_key;
  const double *c1, *c2;
  float* sqd;
  GompR R;
  TfArg tf;   // the transform of the request (an evaluation only)
  int n, n_tgt;
  int mode;
  int first;  // first partial slot
  int nblk;   // ceil(n / 256)
  int pad0_;
};

// grid: the sum over the launch's jobs of ceil(n_j / 256), block 256.  wg[blockIdx.x] = (job, job-local block) of the round table
// (batch_rounds.h); the index is uniform over the workgroup, so the job record comes in through scalar loads.  job < number of jobs and
// blk < jobs[job].nblk; the partial buffers hold first + nblk slots for every job.
__global__ __launch_bounds__(256) void gomp_functor_batch_kernel(const GompJob* __restrict__ jobs, const BlockRef* __restrict__ wg, double* __restrict__ partials) {
  __shared__ double s_red[4 * 13];
  const BlockRef w = wg[blockIdx.x];
  const GompJob& j = jobs[w.job];
  double* out = partials + (size_t)(j.first + w.blk) * 13;
  if (j.mode == 0) gomp_functor_block<0>(j.ox, j.oy, j.oz, j.n, j.tgt, j.corr, j.maha, j.tf, w.blk, s_red, out);
  else if (j.mode == 1) gomp_functor_block<1>(j.ox, j.oy, j.oz, j.n, j.tgt, j.corr, j.maha, j.tf, w.blk, s_red, out);
  else gomp_functor_block<2>(j.ox, j.oy, j.oz, j.n, j.tgt, j.corr, j.maha, j.tf, w.blk, s_red, out);
}

__global__ __launch_bounds__(256) void gomp_update_batch_kernel(const GompJob* __restrict__ jobs, const BlockRef* __restrict__ wg, int* __restrict__ cnt) {
  const BlockRef w = wg[blockIdx.x];
  const GompJob& j = jobs[w.job];
  gomp_update_block(j.best_key, j.n, j.c1, j.c2, j.n_tgt, j.R, j.corr, j.sqd, j.maha, w.blk, cnt + j.first + w.blk);
}

// grid: the round's jobs, block 64.  An evaluation: lane q adds the job's partials of value q in block order, as the last workgroup of
// gomp_functor_kernel does, into out[13 job + q] (the values the mode produces).  An update: the pairs of the job's blocks into pairs[job].
__global__ __launch_bounds__(64) void gomp_fold_batch_kernel(const GompJob* __restrict__ jobs, const double* __restrict__ partials, const int* __restrict__ cnt, double* __restrict__ out,
                                                             int* __restrict__ pairs) {
  const GompJob& j = jobs[blockIdx.x];
  const int q = threadIdx.x;
  if (j.mode == 3) {
    if (q == 0) {
      int total = 0;
      for (int b = 0; b < j.nblk; ++b) total += cnt[j.first + b];
      pairs[blockIdx.x] = total;
    }
    return;
  }
  const int v0 = j.mode == 1 ? 1 : 0, v1 = j.mode == 0 ? 1 : 13;
  if (q >= v0 && q < v1) fold_wave<13>(partials + (size_t)j.first * 13, j.nblk, out + (size_t)blockIdx.x * 13);
  if (q < 13 && (q < v0 || q >= v1)) out[(size_t)blockIdx.x * 13 + q] = 0.0;
  if (q == 0) pairs[blockIdx.x] = 0;
}

}  // namespace gorio

namespace {

float gomp_round_sin(float a) { return (float)std::sin((double)a); }  // the correctly rounded float results
float gomp_round_cos(float a) { return (float)std::cos((double)a); }

// row-major 3x3 float product, every sum left to right
void gomp_mul3f(const float* a, const float* b, float* c) {
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) {
      float s = a[r * 3] * b[q];
      s = s + a[r * 3 + 1] * b[3 + q];
      s = s + a[r * 3 + 2] * b[6 + q];
      c[r * 3 + q] = s;
    }
}

// applyState on an identity matrix (GO:522-533): float Rz Ry Rx, float translation; T = row-major 4x4
void gomp_apply_state(const double* x, float* T) {
  const float a = (float)x[3], b = (float)x[4], c = (float)x[5];
  const float sa = gomp_round_sin(a), ca = gomp_round_cos(a), sb = gomp_round_sin(b), cb = gomp_round_cos(b), sc = gomp_round_sin(c), cc = gomp_round_cos(c);
  const float Rx[9] = {1.f, 0.f, 0.f, 0.f, ca, -sa, 0.f, sa, ca};
  const float Ry[9] = {cb, 0.f, sb, 0.f, 1.f, 0.f, -sb, 0.f, cb};
  const float Rz[9] = {cc, -sc, 0.f, sc, cc, 0.f, 0.f, 0.f, 1.f};
  float zy[9], R[9];
  gomp_mul3f(Rz, Ry, zy);
  gomp_mul3f(zy, Rx, R);
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) T[r * 4 + q] = R[r * 3 + q];
    T[r * 4 + 3] = (float)x[r];
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// computeRDerivative (GO:125-177); R row-major 3x3
void gomp_r_derivative(const double* x, const double* R, double* g) {
  const double phi = x[3], theta = x[4], psi = x[5];
  const double cphi = std::cos(phi), sphi = std::sin(phi), ctheta = std::cos(theta), stheta = std::sin(theta), cpsi = std::cos(psi), spsi = std::sin(psi);
  const double dPhi[9] = {0., sphi * spsi + cphi * cpsi * stheta, cphi * spsi - cpsi * sphi * stheta,
                          0., -cpsi * sphi + cphi * spsi * stheta, -cphi * cpsi - sphi * spsi * stheta,
                          0., cphi * ctheta, -ctheta * sphi};
  const double dTheta[9] = {-cpsi * stheta, cpsi * ctheta * sphi, cphi * cpsi * ctheta,
                            -spsi * stheta, ctheta * sphi * spsi, cphi * ctheta * spsi,
                            -ctheta, -sphi * stheta, -cphi * stheta};
  const double dPsi[9] = {-ctheta * spsi, -cphi * cpsi - sphi * spsi * stheta, cpsi * sphi - cphi * spsi * stheta,
                          cpsi * ctheta, -cphi * spsi + cpsi * sphi * stheta, sphi * spsi + cphi * cpsi * stheta,
                          0., 0., 0.};
  auto inner = [&](const double* m1) {  // matricesInnerProd, GOH:324-334: r += mat1(j, i) * mat2(i, j)
    double r = 0.;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r += m1[j * 3 + i] * R[i * 3 + j];
    return r;
  };
  g[3] = inner(dPhi);
  g[4] = inner(dTheta);
  g[5] = inner(dPsi);
}

void gomp_mul4f(const float* a, const float* b, float* c) {  // row-major 4x4 float product, sums left to right
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      float s = a[r * 4] * b[q];
      for (int k = 1; k < 4; ++k) s = s + a[r * 4 + k] * b[k * 4 + q];
      c[r * 4 + q] = s;
    }
}

bool gomp_ready(const gorio_apd* h) { return h->gomp_pairs >= 0 && h->corr_valid; }

int gomp_reserve(gorio_apd* h) {
  const int n = h->src->n;
  const size_t nblk = (size_t)(n + 255) / 256;
  const size_t spad = (size_t)roundup(n, 512);
  const size_t cap = n + n / 8 + 256;
  HIP_TRY(h, reserve_group(h->gomp_cap, n, cap, h->gomp_out, 3 * cap, h->gomp_s4, cap + 1024, h->gomp_maha, 9 * cap, h->gomp_part, 13 * (cap / 256 + 2), h->gomp_cnt, cap / 256 + 2));
  (void)nblk; (void)spad;
  HIP_TRY(h, h->gomp_res.reserve(16));
  HIP_TRY(h, h->gomp_arrive.reserve(1));
  return GORIO_OK;
}

// everything an update needs: both clouds, their covariances by the GICP_OMP rule, the search index in pruned mode, the buffers
int gomp_prepare(gorio_apd* h) {
  int rc = check_ready(h);
  if (rc) return rc;
  if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "GICP_OMP has no sharded-source mode");
  rc = ensure_points(h, h->src->n);
  if (rc) return rc;
  rc = gorio_apd_calculate_covariances(h);
  if (rc) return rc;
  if (h->params.search == GORIO_SEARCH_PRUNED) {
    std::vector<std::pair<gorio_apd*, DevCloud*>> all = {{h, h->src.get()}, {h, h->tgt.get()}};
    rc = run_index_build(h, all);
    if (rc) return rc;
  }
  return gomp_reserve(h);
}

// output = guess * input (GO:402), in both orders the searches read
int gomp_set_guess(gorio_apd* h, const float* guess) {
  const DevCloud& s = *h->src;
  const int n = s.n;
  const bool pruned = h->params.search == GORIO_SEARCH_PRUNED;
  const int n_spad = pruned ? s.idx_spad : 0;
  TfArg g;
  for (int i = 0; i < 12; ++i) g.m[i] = guess[i];
  float* o = h->gomp_out;
  const size_t st = h->gomp_out.cap() / 3;
  const int cover = std::max(n, n_spad);
  gomp_output_kernel<<<(cover + 255) / 256, 256, 0, h->stream>>>(s.x, s.y, s.z, n, g, o, o + st, o + 2 * st, pruned ? s.idx_s4.get() : nullptr, h->gomp_s4, n_spad);
  HIP_TRY(h, hipGetLastError());
  for (int i = 0; i < 16; ++i) h->gomp_guess[i] = guess[i];
  return GORIO_OK;
}

// the rotation of transformation_ * guess in double (GO:417-423) and the squared gate of an update at transformation_ = Tr
GompR gomp_make_r(const gorio_apd* h, const float* Tr) {
  GompR R;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += (double)Tr[i * 4 + k] * (double)h->gomp_guess[k * 4 + j];
      R.r[i * 3 + j] = s;
    }
  R.thr2 = h->params.corr_dist_threshold * h->params.corr_dist_threshold;
  return R;
}

// one pass of GO:411-476 at transformation_ = Tr: search, gate, Mahalanobis matrices; *m = pairs
int gomp_update(gorio_apd* h, const float* Tr, int* m) {
  const int n = h->src->n;
  const int nbx = (n + 255) / 256;
  const GompR R = gomp_make_r(h, Tr);
  int rc = ensure_batch(h, 1);
  if (rc) return rc;
  PairDesc d;
  PairState s;
  const float* o = h->gomp_out;
  const size_t st = h->gomp_out.cap() / 3;
  fill_moved_search(h, d, s, h->d_state, (n + 63) / 64, o, o + st, o + 2 * st, h->gomp_s4, Tr);  // the searches read the `output` copy
  HIP_TRY(h, hipMemcpyAsync(h->d_desc, &d, sizeof(PairDesc), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_state, &s, sizeof(s), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // d and s live on this frame
  HIP_TRY(h, hipMemsetAsync(h->best_key, 0xff, sizeof(unsigned long long) * n, h->stream));
  launch_nn(h, h->d_desc, dim3(nbx, d.nn_splits, 1), roundup(n, 512), 1, h->tgt->n);
  gomp_update_kernel<<<nbx, 256, 0, h->stream>>>(h->best_key, n, h->src->cov6, h->tgt->cov6, h->tgt->n, R, h->corr, h->sqd, h->gomp_maha, h->gomp_cnt);
  HIP_TRY(h, hipGetLastError());
  std::vector<int> cnt(nbx);
  HIP_TRY(h, hipMemcpyAsync(cnt.data(), h->gomp_cnt, sizeof(int) * nbx, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  int total = 0;
  for (int b = 0; b < nbx; ++b) total += cnt[b];
  h->gomp_pairs = total;
  h->corr_valid = true;
  h->omega_valid = true;
  *m = total;
  return GORIO_OK;
}

// the functor's value and gradient from the 13 sums of an evaluation at x over the m pairs held (GO:275, 321-327, 366-370)
void gomp_finish_evaluation(gorio_apd* h, const double* x, int mode, const double* r, double* f, double* g) {
  const int m = h->gomp_pairs;
  ++h->gomp_evals;
  if (mode != 1 && f) *f = r[0] / (double)m;
  if (mode != 0 && g) {
    const double sc = 2.0 / (double)m;
    double R[9];
    for (int i = 0; i < 3; ++i) g[i] = r[1 + i] * sc;
    for (int i = 0; i < 9; ++i) R[i] = r[4 + i] * sc;
    gomp_r_derivative(x, R, g);
  }
}

// one functor evaluation at x over the pairs held: mode 0 f, 1 df, 2 fdf
int gomp_evaluate(gorio_apd* h, const double* x, int mode, double* f, double* g) {
  const int n = h->src->n;
  const int nbx = (n + 255) / 256;
  float T[16];
  gomp_apply_state(x, T);
  TfArg tf;
  for (int i = 0; i < 12; ++i) tf.m[i] = T[i];
  const float* o = h->gomp_out;
  const size_t st = h->gomp_out.cap() / 3;
  HIP_TRY(h, hipMemsetAsync(h->gomp_arrive, 0, sizeof(unsigned int), h->stream));
  if (mode == 0) gomp_functor_kernel<0><<<nbx, 256, 0, h->stream>>>(o, o + st, o + 2 * st, n, h->tgt->p4, h->corr, h->gomp_maha, tf, h->gomp_part, h->gomp_arrive, h->gomp_res);
  else if (mode == 1) gomp_functor_kernel<1><<<nbx, 256, 0, h->stream>>>(o, o + st, o + 2 * st, n, h->tgt->p4, h->corr, h->gomp_maha, tf, h->gomp_part, h->gomp_arrive, h->gomp_res);
  else gomp_functor_kernel<2><<<nbx, 256, 0, h->stream>>>(o, o + st, o + 2 * st, n, h->tgt->p4, h->corr, h->gomp_maha, tf, h->gomp_part, h->gomp_arrive, h->gomp_res);
  HIP_TRY(h, hipGetLastError());
  double r[13] = {0};
  HIP_TRY(h, hipMemcpyAsync(r, h->gomp_res, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  gomp_finish_evaluation(h, x, mode, r, f, g);
  return GORIO_OK;
}

// computeTransformation, GO:375-520, as a machine that stops wherever it needs the device: for one pass of GO:411-476 at transformation_
// (kUpdate), or for one functor evaluation of the BFGS inner solve (kEvaluate).  The caller answers with update_done() / evaluation_done().
struct GompMachine {
  enum State { kUpdate, kEvaluate, kFinished };
  gorio_apd* h = nullptr;
  State state = kFinished;
  float guess[16], Tr[16], prev[16];
  bool conv = false;
  int nr = 0;
  int mode = 0;  // of the evaluation wanted: 0 f, 1 df, 2 fdf
  double x[6];   // where
  gorio_bfgs::Machine bfgs;  // rho, sigma, tau1, tau2, tau3, order of GO:212-217 are the defaults of gorio_bfgs::Params

  void begin(gorio_apd* handle, const float* g) {
    h = handle;
    for (int i = 0; i < 16; ++i) guess[i] = g[i];
    h->gomp_outer = 0; h->gomp_inner = 0; h->gomp_evals = 0; h->gomp_status = gorio_bfgs::kRunning;
    for (int i = 0; i < 16; ++i) Tr[i] = prev[i] = (i % 5 == 0) ? 1.f : 0.f;  // align(): transformation_ = previous_transformation_ = identity
    conv = false;
    nr = 0;
    state = kUpdate;
  }
  bool done() const { return state == kFinished; }
  // m = pairs of the update at Tr
  void update_done(int m) {
    for (int i = 0; i < 16; ++i) prev[i] = Tr[i];  // GO:479
    if (m < 4) {  // NotEnoughPointsException, GO:187-191 -> break, GO:499-503
      h->err = "GICP_OMP: fewer than 4 correspondences";
      state = kFinished;
      return;
    }
    const double x0[6] = {(double)Tr[3], (double)Tr[7], (double)Tr[11], (double)(float)std::atan2((double)Tr[9], (double)Tr[10]), (double)(float)std::asin((double)-Tr[8]),
                          (double)(float)std::atan2((double)Tr[4], (double)Tr[0])};  // GO:194-200, float results rounded once
    bfgs.start(x0, h->gomp_max_inner, 1e-2);
    next_request();
  }
  // f, g: the functor at x (what gomp_finish_evaluation makes of the sums)
  void evaluation_done(double f, const double* g) {
    bfgs.resume(f, g);
    next_request();
  }
  void results(float* T_out, int* converged, int* nr_iterations, int* n_linearize) const {
    gomp_mul4f(prev, guess, T_out);  // GO:516
    if (converged) *converged = conv ? 1 : 0;
    if (nr_iterations) *nr_iterations = nr;
    if (n_linearize) *n_linearize = h->gomp_evals;
  }

 private:
  void next_request() {
    mode = bfgs.request(x);
    if (mode != gorio_bfgs::Machine::kFinished) {
      state = kEvaluate;
      return;
    }
    const gorio_apd_params& p = h->params;
    const int inner = bfgs.inner(), result = bfgs.status();
    h->gomp_inner += inner;
    h->gomp_status = result;
    if (!(result == gorio_bfgs::kNoProgress || result == gorio_bfgs::kSuccess || inner == h->gomp_max_inner)) {  // SolverDidntConvergeException, GO:243-245
      h->err = "GICP_OMP: BFGS solver didn't converge";
      state = kFinished;
      return;
    }
    gomp_apply_state(bfgs.x(), Tr);  // GO:240-241
    double delta = 0.;  // GO:485-497
    for (int k = 0; k < 4; ++k)
      for (int l = 0; l < 4; ++l) {
        const double ratio = (k < 3 && l < 3) ? 1. / p.rotation_epsilon : 1. / p.transformation_epsilon;
        const double c_delta = ratio * (double)std::fabs(prev[k * 4 + l] - Tr[k * 4 + l]);
        if (c_delta > delta) delta = c_delta;
      }
    ++nr;
    ++h->gomp_outer;
    if (nr >= p.max_iterations || delta < 1) {
      conv = true;
      for (int i = 0; i < 16; ++i) prev[i] = Tr[i];
      state = kFinished;
      return;
    }
    state = kUpdate;
  }
};

int gomp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!guess || !T_out) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = gomp_prepare(h);
  if (rc) return rc;
  rc = gomp_set_guess(h, guess);
  if (rc) return rc;
  GompMachine mc;
  mc.begin(h, guess);
  while (!mc.done()) {
    if (mc.state == GompMachine::kUpdate) {
      int m = 0;
      rc = gomp_update(h, mc.Tr, &m);
      if (rc) return rc;
      mc.update_done(m);
    } else {
      double f = NAN, g[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
      rc = gomp_evaluate(h, mc.x, mc.mode, &f, g);
      if (rc) return rc;
      mc.evaluation_done(f, g);
    }
  }
  mc.results(T_out, converged, nr_iterations, n_linearize);
  if (H_out) std::memset(H_out, 0, sizeof(double) * 36);
  resolve_stage_events(h);
  return GORIO_OK;
}

struct GompRounds {  // the round table of run_rounds
  using Job = GompJob;
  static constexpr int kSums = 13;
  static constexpr bool kCounts = true, kSecondList = false;  // an update's pairs: an int per block, folded to an int per job
  static void fold(int njobs, hipStream_t stream, const GompJob* jobs, const double* part, const int* cnt, double* out, int* pairs) { gomp_fold_batch_kernel<<<njobs, 64, 0, stream>>>(jobs, part, cnt, out, pairs); }
};

// gorio_apd_gicp_omp_align_batch: N machines in lock-step.  Every round each unfinished handle has exactly one request pending; the
// updates of a round share one search launch and one update launch, the evaluations one functor launch, everything one fold launch, one
// copy back and one synchronisation.  The tables and the sums live in the lead handle (hs[0]), whose stream carries the rounds.
int gomp_align_batch(gorio_apd** hs, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations, int* n_evaluations) {
  gorio_apd* lead = hs[0];
  // ---- search indices and covariances: a cloud several handles hold is made once
  int rc = batch_prepare_search(hs, count);
  if (rc) return rc;
  {
    std::unordered_set<DevCloud*> seen;
    std::vector<std::pair<gorio_apd*, DevCloud*>> stale;
    for (int q = 0; q < count; ++q)
      for (DevCloud* c : {hs[q]->src.get(), hs[q]->tgt.get()})
        if (c->cov_count != c->n && seen.insert(c).second) stale.emplace_back(hs[q], c);
    while (!stale.empty()) {  // run_covariances estimates with ONE gicp_epsilon, its lead's: one call per value
      gorio_apd* first = stale.front().first;
      std::vector<std::pair<gorio_apd*, DevCloud*>> todo, rest;
      for (auto& t : stale) (t.first->gomp_eps == first->gomp_eps ? todo : rest).push_back(t);
      rc = hand_over(lead, first, run_covariances(first, todo));
      if (rc) return rc;
      stale.swap(rest);
    }
  }
  size_t max_blocks = 0;
  rc = batch_arm_handles(hs, count, [&](int q) {
    max_blocks += (size_t)(hs[q]->src->n + 255) / 256;
    const int rc2 = gomp_reserve(hs[q]);
    return rc2 ? rc2 : gomp_set_guess(hs[q], guesses + (size_t)16 * q);
  });
  if (rc) return rc;
  if (batch_rounds::too_many_wg(max_blocks, 16)) return fail(lead, GORIO_ERR_INVALID, "gicp_omp_align_batch: too many source points in one batch");
  if ((rc = ensure_batch(lead, count))) return rc;
  std::vector<GompMachine> mc(count);
  for (int q = 0; q < count; ++q) mc[q].begin(hs[q], guesses + (size_t)16 * q);
  std::vector<PairDesc> descs(count);
  std::vector<PairState> states(count);
  RoundCounters ctr;
  ctr.launches = count;  // one gomp_output_kernel launch per handle so far
  // job k of the round belongs to handle order[k]: the updates (the leading class) first, then the evaluations
  auto pending = [&](int q) { return mc[q].state == GompMachine::kUpdate ? 0 : mc[q].state == GompMachine::kEvaluate ? 1 : -1; };
  auto fill = [&](int, int q, GompJob& j) {
    gorio_apd* h = hs[q];
    const GompMachine& m = mc[q];
    float* o = h->gomp_out;
    const size_t st = h->gomp_out.cap() / 3;
    j.ox = o; j.oy = o + st; j.oz = o + 2 * st;
    j.tgt = h->tgt->p4;
    j.corr = h->corr;
    j.maha = h->gomp_maha;
    j.n = h->src->n;
    j.n_tgt = h->tgt->n;
    if (m.state == GompMachine::kUpdate) {
      j.mode = 3;
      j.best_key = h->best_key;
      j.c1 = h->src->cov6;
      j.c2 = h->tgt->cov6;
      j.sqd = h->sqd;
      j.R = gomp_make_r(h, m.Tr);
    } else {
      j.mode = m.mode;
      float T[16];
      gomp_apply_state(m.x, T);
      for (int i = 0; i < 12; ++i) j.tf.m[i] = T[i];
    }
    const int nblk = (j.n + 255) / 256;
    return batch_rounds::JobShape{nblk, nblk, false};
  };
  auto launch = [&](const RoundView<GompJob>& v, int& launches) {
    const int n_upd = v.plan.n_leading;
    if (n_upd > 0) {
      long upd_waves = 0;
      int upd_max_n = 0, upd_max_m = 0, max_splits = 1;
      for (int k = 0; k < n_upd; ++k) {
        upd_waves += (hs[v.order[k]]->src->n + 63) / 64;
        upd_max_n = std::max(upd_max_n, hs[v.order[k]]->src->n);
        upd_max_m = std::max(upd_max_m, hs[v.order[k]]->tgt->n);
      }
      for (int k = 0; k < n_upd; ++k) {  // the searches read the `output` copy
        gorio_apd* h = hs[v.order[k]];
        fill_moved_search(h, descs[k], states[k], lead->d_states_batch + k, upd_waves, v.jobs[k].ox, v.jobs[k].oy, v.jobs[k].oz, h->gomp_s4, mc[v.order[k]].Tr);
        max_splits = std::max(max_splits, descs[k].nn_splits);
      }
      if (int rc2 = upload_staged(lead, lead->pin_desc, lead->d_desc, descs.data(), sizeof(PairDesc) * n_upd)) return rc2;
      if (int rc2 = upload_staged(lead, lead->pin_states, lead->d_states_batch, states.data(), sizeof(PairState) * n_upd)) return rc2;
      launch_nn(lead, lead->d_desc, dim3((upd_max_n + 255) / 256, max_splits, n_upd), roundup(upd_max_n, 512), n_upd, upd_max_m);
      gomp_update_batch_kernel<<<v.plan.lead_wg, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs, lead->round.cnt);
      launches += 2;
    }
    if (v.plan.wg > v.plan.lead_wg) {
      gomp_functor_batch_kernel<<<v.plan.wg - v.plan.lead_wg, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs + v.plan.lead_wg, lead->round.part);
      ++launches;
    }
    return (int)GORIO_OK;
  };
  auto consume = [&](int, int q, const double* sums, int pairs) {
    gorio_apd* h = hs[q];
    GompMachine& m = mc[q];
    if (m.state == GompMachine::kUpdate) {
      h->gomp_pairs = pairs;
      h->corr_valid = true;
      h->omega_valid = true;
      m.update_done(pairs);
    } else {
      double f = NAN, g[6] = {NAN, NAN, NAN, NAN, NAN, NAN};
      gomp_finish_evaluation(h, m.x, m.mode, sums, &f, g);
      m.evaluation_done(f, g);
    }
  };
  if ((rc = run_rounds<GompRounds>(lead, count, max_blocks, ctr, pending, fill, launch, consume))) return rc;
  for (int q = 0; q < count; ++q)
    mc[q].results(T_out + (size_t)16 * q, converged ? converged + q : nullptr, nr_iterations ? nr_iterations + q : nullptr, n_evaluations ? n_evaluations + q : nullptr);
  lead->gomp_b_rounds = ctr.rounds;
  lead->gomp_b_launches = ctr.launches;
  resolve_stage_events(lead);
  return GORIO_OK;
}

// the covariance rule of GO:50-122 over the lists run_covariances has just left in DevCloud::knn
int gomp_covariances(gorio_apd* lead, std::vector<std::pair<gorio_apd*, DevCloud*>>& todo) {
  for (auto& t : todo) {
    DevCloud& c = *t.second;
    gomp_cov_kernel<<<(c.n + 255) / 256, 256, 0, lead->stream>>>(c.view(), c.knn, c.knn_k, t.first->gomp_eps);
  }
  HIP_TRY(lead, hipGetLastError());
  return GORIO_OK;
}

}  // namespace

extern "C" {

int gorio_apd_set_gicp_omp_params(gorio_apd_t* h, double gicp_epsilon, int max_optimizer_iterations) {
  if (!h) return GORIO_ERR_INVALID;
  if (!(gicp_epsilon > 0.0) || !std::isfinite(gicp_epsilon)) return fail(h, GORIO_ERR_INVALID, "set_gicp_omp_params: gicp_epsilon must be positive");
  if (max_optimizer_iterations < 1) return fail(h, GORIO_ERR_INVALID, "set_gicp_omp_params: max_optimizer_iterations must be at least 1");
  if (gicp_epsilon != h->gomp_eps) {  // covariances estimated by the old epsilon are stale; a cloud other handles hold too is theirs (check_ready then refuses it)
    for (auto* c : {&h->src, &h->tgt})
      if ((*c)->cov_reg == kRegGicpOmp && (*c)->cov_count && c->use_count() == 1) (*c)->covs_dropped();
  }
  h->gomp_eps = gicp_epsilon;
  h->gomp_max_inner = max_optimizer_iterations;
  return GORIO_OK;
}

int gorio_apd_get_gicp_omp_params(const gorio_apd_t* h, double* gicp_epsilon, int* max_optimizer_iterations) {
  if (!h) return GORIO_ERR_INVALID;
  if (gicp_epsilon) *gicp_epsilon = h->gomp_eps;
  if (max_optimizer_iterations) *max_optimizer_iterations = h->gomp_max_inner;
  return GORIO_OK;
}

int gorio_apd_gicp_omp_update(gorio_apd_t* h, const float transformation[16], const float guess[16], int* m) {
  if (!h || !transformation || !guess || !m) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_GICP_OMP) return fail(h, GORIO_ERR_STATE, "gicp_omp_update: the handle's method is not GORIO_METHOD_GICP_OMP");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = gomp_prepare(h);
  if (rc) return rc;
  rc = gomp_set_guess(h, guess);
  if (rc) return rc;
  return gomp_update(h, transformation, m);
}

int gorio_apd_gicp_omp_evaluate(gorio_apd_t* h, const double x[6], int mode, double* f, double* g) {
  if (!h || !x || mode < 0 || mode > 2) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_GICP_OMP) return fail(h, GORIO_ERR_STATE, "gicp_omp_evaluate: the handle's method is not GORIO_METHOD_GICP_OMP");
  if (!gomp_ready(h) || h->gomp_cap < h->src->n) return fail(h, GORIO_ERR_STATE, "gicp_omp_evaluate: no pairs held (gorio_apd_gicp_omp_update or an align first)");
  if (h->gomp_pairs < 1) return fail(h, GORIO_ERR_STATE, "gicp_omp_evaluate: the last update found no pairs");
  if ((mode != 1 && !f) || (mode != 0 && !g)) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  return gomp_evaluate(h, x, mode, f, g);
}

int gorio_apd_gicp_omp_diag(const gorio_apd_t* h, int* outer, int* inner_total, int* evaluations, int* last_status) {
  if (!h) return GORIO_ERR_INVALID;
  if (outer) *outer = h->gomp_outer;
  if (inner_total) *inner_total = h->gomp_inner;
  if (evaluations) *evaluations = h->gomp_evals;
  if (last_status) *last_status = h->gomp_status;
  return GORIO_OK;
}

int gorio_apd_gicp_omp_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations, int* n_evaluations) {
  if (count == 0) return GORIO_OK;
  if (int rc = batch_front_door("gicp_omp_align_batch", handles, count, guesses, T_out, true, [](const gorio_apd* h) { return h->method == GORIO_METHOD_GICP_OMP; }, "the handle's method is not GORIO_METHOD_GICP_OMP", check_ready)) return rc;
  gorio_apd* lead = handles[0];
  for (int q = 0; q < count; ++q)
    if (handles[q]->comm || (handles[q]->shard_only && handles[q]->comm_world > 1))
      return fail(lead, GORIO_ERR_INVALID, "gicp_omp_align_batch: handle " + std::to_string(q) + ": a handle with a communicator (sharded source) cannot be part of a batch");
  HIP_TRY(lead, hipSetDevice(lead->device));
  return gomp_align_batch(handles, count, guesses, T_out, converged, nr_iterations, n_evaluations);
}

int gorio_apd_gicp_omp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches) {
  if (!lead) return GORIO_ERR_INVALID;
  if (rounds) *rounds = lead->gomp_b_rounds;
  if (launches) *launches = lead->gomp_b_launches;
  return GORIO_OK;
}

}  // extern "C"
