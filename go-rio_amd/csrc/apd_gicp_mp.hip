// apd_gicp_mp.hip -- fast_gicp::FastGICPMultiPoints (GORIO_METHOD_GICP_MP; the definition is the comment of include/gorio_apd.h): every
// source point is matched against a distribution merged from ALL target points within neighbor_search_radius of its transformed
// position, the merge redone at every Gauss-Newton pass.  Kernels first, the host side below them.  Included at the end of apd_api.hip,
// behind apd_search.hip: the neighbourhoods are that file's exact radius search (count, scan, fill, segment sort) run against the
// target's own DevCloud and index -- no second upload, no second index -- with its CSR left on the device.
//
//   mp_cov_kernel         one lane per point: the float covariance of its exact k-NN list (not divided by k) and the regularisation,
//                         written with the point as a record of three float4 (x y z c00 | c01 c02 c11 c12 | c22 0 0 0), so that the
//                         merge gathers a neighbour with three aligned 16-byte loads
//   mp_query_kernel       the float-transformed source (transform_f), as float4
//   mp_linearize_kernel   the hot path.  ONE LANE PER SOURCE POINT walks its CSR segment in the CSR's order (ascending (d, index)) and
//                         keeps the ten fp64 sums (weight, 3 mean, 6 covariance); the float term of the point follows, then its 21 + 6
//                         fp64 products and the used flag go through the wave tree of wave_sum28 and (w0 + w1) + (w2 + w3) into the
//                         block's 28 partials.  The summation order of a merge is therefore the CSR order and nothing else; a lane
//                         group per point would need a combination order of its own and buys nothing while the search dominates a pass
//                         (profiles/r20/gicp_mp.md).  No LDS but the 4 x 28 reduction cells, no scratch, no atomics.
//   mp_fold_kernel        the block partials added in block order
//
// The shell (6 x 6 LDLT, exp / log, update, convergence) runs on the host between passes: the radius search synchronises once per pass
// for its total anyway, and the pass ends with one copy back of 28 doubles.
#include <hip/hip_runtime.h>

#include <chrono>

namespace gorio {

struct MpPose {
  float m[12];  // rows of [R | t]
};

// grid ceil(n / 256), block 256.  knn: [n][k] lists in ascending (d, index) order, the point itself included.  reg: gorio_regularization
// (NONE is refused by the host).
__global__ __launch_bounds__(256) void mp_cov_kernel(const float4* __restrict__ pts, const int* __restrict__ knn, int n, int k, int reg, float4* __restrict__ rec) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* __restrict__ l = knn + (size_t)i * k;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int j = 0; j < k; ++j) {
    int t = l[j];
    if ((unsigned int)t >= (unsigned int)n) t = i;  // a list is full when n >= k (the host refuses smaller clouds)
    const float4 p = pts[t];
    sx = sx + p.x;
    sy = sy + p.y;
    sz = sz + p.z;
  }
  const float fk = (float)k;
  const float mx = sx / fk, my = sy / fk, mz = sz / fk;
  float c00 = 0.f, c01 = 0.f, c02 = 0.f, c11 = 0.f, c12 = 0.f, c22 = 0.f;
  for (int j = 0; j < k; ++j) {
    int t = l[j];
    if ((unsigned int)t >= (unsigned int)n) t = i;
    const float4 p = pts[t];
    const float dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
    c00 = c00 + dx * dx;
    c01 = c01 + dx * dy;
    c02 = c02 + dx * dz;
    c11 = c11 + dy * dy;
    c12 = c12 + dy * dz;
    c22 = c22 + dz * dz;
  }
  float o00, o01, o02, o11, o12, o22;
  if (reg == GORIO_REG_FROBENIUS) {
    double i00, i01, i02, i11, i12, i22;
    inv_sym3((double)c00 + 1e-3, (double)c01, (double)c02, (double)c11 + 1e-3, (double)c12, (double)c22 + 1e-3, i00, i01, i02, i11, i12, i22);
    const double nrm = sqrt((((i00 * i00 + i01 * i01) + i02 * i02) + ((i01 * i01 + i11 * i11) + i12 * i12)) + ((i02 * i02 + i12 * i12) + i22 * i22));
    double r00, r01, r02, r11, r12, r22;
    inv_sym3(i00 / nrm, i01 / nrm, i02 / nrm, i11 / nrm, i12 / nrm, i22 / nrm, r00, r01, r02, r11, r12, r22);
    o00 = (float)r00; o01 = (float)r01; o02 = (float)r02; o11 = (float)r11; o12 = (float)r12; o22 = (float)r22;
  } else {
    // the symmetric eigen-solver of this library stands in for JacobiSVD<Matrix3f>: the matrix is symmetric positive semi-definite, so its
    // singular values are its eigenvalues and U = V
    const Eig3 e = sym3_eigen((double)c00, (double)c01, (double)c02, (double)c11, (double)c12, (double)c22);
    const float s0 = fabsf((float)e.w0), s1 = fabsf((float)e.w1), s2 = fabsf((float)e.w2);
    float v0, v1, v2;
    if (reg == GORIO_REG_PLANE) {
      v0 = 1.f; v1 = 1.f; v2 = 1e-3f;
    } else if (reg == GORIO_REG_MIN_EIG) {
      v0 = fmaxf(s0, 1e-3f); v1 = fmaxf(s1, 1e-3f); v2 = fmaxf(s2, 1e-3f);
    } else {  // NORMALIZED_MIN_EIG
      const float smax = fmaxf(s0, fmaxf(s1, s2));
      v0 = fmaxf(s0 / smax, 1e-3f); v1 = fmaxf(s1 / smax, 1e-3f); v2 = fmaxf(s2 / smax, 1e-3f);
    }
    const double d0 = (double)v0, d1 = (double)v1, d2 = (double)v2;
    o00 = (float)((d0 * e.v00 * e.v00 + d1 * e.v01 * e.v01) + d2 * e.v02 * e.v02);
    o01 = (float)((d0 * e.v00 * e.v10 + d1 * e.v01 * e.v11) + d2 * e.v02 * e.v12);
    o02 = (float)((d0 * e.v00 * e.v20 + d1 * e.v01 * e.v21) + d2 * e.v02 * e.v22);
    o11 = (float)((d0 * e.v10 * e.v10 + d1 * e.v11 * e.v11) + d2 * e.v12 * e.v12);
    o12 = (float)((d0 * e.v10 * e.v20 + d1 * e.v11 * e.v21) + d2 * e.v12 * e.v22);
    o22 = (float)((d0 * e.v20 * e.v20 + d1 * e.v21 * e.v21) + d2 * e.v22 * e.v22);
  }
  const float4 p = pts[i];
  rec[3 * (size_t)i] = make_float4(p.x, p.y, p.z, o00);
  rec[3 * (size_t)i + 1] = make_float4(o01, o02, o11, o12);
  rec[3 * (size_t)i + 2] = make_float4(o22, 0.f, 0.f, 0.f);
}

// grid ceil(n / 256), block 256
__global__ __launch_bounds__(256) void mp_query_kernel(const float4* __restrict__ pts, int n, MpPose T, float4* __restrict__ q) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  float x, y, z;
  transform_f(T.m, p.x, p.y, p.z, x, y, z);
  q[i] = make_float4(x, y, z, 0.f);
}

// grid ceil(n / 256), block 256.  src_rec / tgt_rec: the records of mp_cov_kernel; q: the transformed source of THIS pose; offs / idx /
// sqd: the CSR of the radius search (idx and sqd may be null when it is empty).  merged (may be null): per source point mean_B, cov_B
// and the used flag as three float4 (m0 m1 m2 c00 | c01 c02 c11 c12 | c22 used 0 0).  partials: [blocks][28] = 21 H (upper triangle,
// row-major), 6 g, the points used.
__global__ __launch_bounds__(256) void mp_linearize_kernel(const float4* __restrict__ src_rec, const float4* __restrict__ q, int n, const long long* __restrict__ offs,
                                                           const int* __restrict__ idx, const float* __restrict__ sqd, const float4* __restrict__ tgt_rec, int n_tgt, MpPose T,
                                                           double radius, float4* __restrict__ merged, double* __restrict__ partials) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double acc[28];
#pragma unroll
  for (int t = 0; t < 28; ++t) acc[t] = 0.0;
  long long o0 = 0, o1 = 0;
  if (i < n) {
    o0 = offs[i];
    o1 = offs[i + 1];
  }
  float mb0 = 0.f, mb1 = 0.f, mb2 = 0.f, b00 = 0.f, b01 = 0.f, b02 = 0.f, b11 = 0.f, b12 = 0.f, b22 = 0.f;
  const bool used = o1 > o0;
  if (used) {
    double sw = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    for (long long j = o0; j < o1; ++j) {
      const int t = idx[j];
      if ((unsigned int)t >= (unsigned int)n_tgt) continue;  // the search emits indices of the target only
      double w = 1.0 - (double)sqrtf(sqd[j]) / radius;  // the correctly rounded float root
      w = fmax(1e-3, fmin(1.0, w));
      const float4 r0 = tgt_rec[3 * (size_t)t], r1 = tgt_rec[3 * (size_t)t + 1], r2 = tgt_rec[3 * (size_t)t + 2];
      sw += w;
      m0 += w * (double)r0.x;
      m1 += w * (double)r0.y;
      m2 += w * (double)r0.z;
      s00 += w * (double)r0.w;
      s01 += w * (double)r1.x;
      s02 += w * (double)r1.y;
      s11 += w * (double)r1.z;
      s12 += w * (double)r1.w;
      s22 += w * (double)r2.x;
    }
    mb0 = (float)(m0 / sw); mb1 = (float)(m1 / sw); mb2 = (float)(m2 / sw);
    b00 = (float)(s00 / sw); b01 = (float)(s01 / sw); b02 = (float)(s02 / sw);
    b11 = (float)(s11 / sw); b12 = (float)(s12 / sw); b22 = (float)(s22 / sw);
    const float4 a4 = q[i];
    const float a[3] = {a4.x, a4.y, a4.z};
    const float d[3] = {mb0 - a[0], mb1 - a[1], mb2 - a[2]};
    const float4 c0 = src_rec[3 * (size_t)i], c1 = src_rec[3 * (size_t)i + 1], c2 = src_rec[3 * (size_t)i + 2];
    const float A[3][3] = {{c0.w, c1.x, c1.y}, {c1.x, c1.z, c1.w}, {c1.y, c1.w, c2.x}};
    const float R[3][3] = {{T.m[0], T.m[1], T.m[2]}, {T.m[4], T.m[5], T.m[6]}, {T.m[8], T.m[9], T.m[10]}};
    const float B[3][3] = {{b00, b01, b02}, {b01, b11, b12}, {b02, b12, b22}};
    float M[3][3], Q[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[r][c] = (R[r][0] * A[0][c] + R[r][1] * A[1][c]) + R[r][2] * A[2][c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Q[r][c] = B[r][c] + ((M[r][0] * R[c][0] + M[r][1] * R[c][1]) + M[r][2] * R[c][2]);
    float C[3][3];  // adj(Q) / det(Q), the cofactor form of FastVGICPCuda's pair term
    C[0][0] = Q[1][1] * Q[2][2] - Q[1][2] * Q[2][1];
    C[0][1] = Q[0][2] * Q[2][1] - Q[0][1] * Q[2][2];
    C[0][2] = Q[0][1] * Q[1][2] - Q[0][2] * Q[1][1];
    C[1][0] = Q[1][2] * Q[2][0] - Q[1][0] * Q[2][2];
    C[1][1] = Q[0][0] * Q[2][2] - Q[0][2] * Q[2][0];
    C[1][2] = Q[0][2] * Q[1][0] - Q[0][0] * Q[1][2];
    C[2][0] = Q[1][0] * Q[2][1] - Q[1][1] * Q[2][0];
    C[2][1] = Q[0][1] * Q[2][0] - Q[0][0] * Q[2][1];
    C[2][2] = Q[0][0] * Q[1][1] - Q[0][1] * Q[1][0];
    const float det = (Q[0][0] * C[0][0] + Q[0][1] * C[1][0]) + Q[0][2] * C[2][0];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) C[r][c] = C[r][c] / det;
    const float S[3][3] = {{0.f, -a[2], a[1]}, {a[2], 0.f, -a[0]}, {-a[1], a[0], 0.f}};  // skew(trans a)
    float res[3], J[3][6];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      res[r] = (C[r][0] * d[0] + C[r][1] * d[1]) + C[r][2] * d[2];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[r][c] = (C[r][0] * S[0][c] + C[r][1] * S[1][c]) + C[r][2] * S[2][c];
        J[r][3 + c] = -C[r][c];
      }
    }
    int t = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = r; c < 6; ++c) acc[t++] = ((double)J[0][r] * (double)J[0][c] + (double)J[1][r] * (double)J[1][c]) + (double)J[2][r] * (double)J[2][c];
#pragma unroll
    for (int r = 0; r < 6; ++r) acc[21 + r] = ((double)J[0][r] * (double)res[0] + (double)J[1][r] * (double)res[1]) + (double)J[2][r] * (double)res[2];
    acc[27] = 1.0;
  }
  if (merged && i < n) {
    merged[3 * (size_t)i] = make_float4(mb0, mb1, mb2, b00);
    merged[3 * (size_t)i + 1] = make_float4(b01, b02, b11, b12);
    merged[3 * (size_t)i + 2] = make_float4(b22, used ? 1.f : 0.f, 0.f, 0.f);
  }
  __shared__ double red[4][28];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  {
    double ws[7];
    wave_sum28(acc, ws);
    if ((lane & 15) == 0) {
#pragma unroll
      for (int k = 0; k < 7; ++k) red[wv][7 * (lane >> 4) + k] = ws[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 28) partials[(size_t)blockIdx.x * 28 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// grid 1, block 64: out[t] = the partials of term t added in block order
__global__ __launch_bounds__(64) void mp_fold_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= 28) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partials[(size_t)b * 28 + t];
  out[t] = s;
}

}  // namespace gorio

// ================================================================================================= host

struct GicpMpState {
  gorio_search_handle s;         // the radius search's buffers; s.up is the registration handle, s.cloud its target
  DevBuf<float4> q;              // [n] transformed source
  DevBuf<float4> merged;         // [n][3] of the last gorio_apd_gicp_mp_pass
  DevBuf<double> part;           // [blocks][28]; q, merged and part: one group of capacity cap (source points)
  size_t cap = 0;
  DevBuf<double> out;            // [28]
  PinnedBuf h_out;
  int pass_n = 0;                // source points of the pass held
  bool merged_valid = false;
  long long total = 0;           // neighbours of the last pass
  int used = 0, passes = 0;      // of the last pass / of the last align
  double stage_s[4] = {0, 0, 0, 0};  // query transform, radius search, merge + linearise (with fold and copy back), shell: filled while profiling
};

namespace {

bool mp_cov_matches(const gorio_apd* h, const DevCloud& c) { return c.mp_valid && c.mp_k == h->params.k_correspondences && c.mp_reg == kRegMpBase + h->params.regularization; }
bool mp_shared_mismatch(const gorio_apd* h, const std::shared_ptr<DevCloud>& c) { return c.use_count() > 1 && c->mp_valid && !mp_cov_matches(h, *c); }

int mp_cloud_ready(gorio_apd* h, const DevCloud& c, const char* side) {
  const gorio_apd_params& p = h->params;
  if (p.regularization == GORIO_REG_NONE) return fail(h, GORIO_ERR_UNSUPPORTED, "FastGICPMultiPoints: regularization NONE is not supported (the reference aborts there)");
  if (p.regularization < 0 || p.regularization > 4) return fail(h, GORIO_ERR_UNSUPPORTED, "unknown regularization method");
  if (p.k_correspondences < 1 || p.k_correspondences > 32) return fail(h, GORIO_ERR_UNSUPPORTED, "k_correspondences must be in [1, 32]");
  if (c.n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, std::string(side) + " cloud has fewer points than k_correspondences (the k-NN list would hold padding)");
  return GORIO_OK;
}

int mp_ready(gorio_apd* h) {
  if (!h->src->present) return fail(h, GORIO_ERR_STATE, "no input source set (setInputSource)");
  if (!h->tgt->present) return fail(h, GORIO_ERR_STATE, "no input target set (setInputTarget)");
  if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "FastGICPMultiPoints has no sharded-source mode (gorio_apd_comm_init / gorio_apd_debug_set_shard): use an unsharded handle");
  if (mp_shared_mismatch(h, h->tgt)) return fail(h, GORIO_ERR_INVALID, "the shared target's FastGICPMultiPoints covariances were made with another k_correspondences or regularization: give this handle a target of its own (setInputTarget)");
  if (mp_shared_mismatch(h, h->src)) return fail(h, GORIO_ERR_INVALID, "the shared source's FastGICPMultiPoints covariances were made with another k_correspondences or regularization: give this handle a source of its own (setInputSource)");
  if (int rc = mp_cloud_ready(h, *h->src, "source")) return rc;
  return mp_cloud_ready(h, *h->tgt, "target");
}

// calculate_covariances (MPI:225-276) of cloud c: the handle's exact k-NN lists, then one lane per point
int mp_covariances(gorio_apd* h, DevCloud& c) {
  if (mp_cov_matches(h, c)) return GORIO_OK;
  c.mp_dropped();
  const int n = c.n, k = h->params.k_correspondences;
  HIP_TRY(h, c.mp_knn.reserve((size_t)n * k, (size_t)(n + n / 8 + 64) * k));
  HIP_TRY(h, c.mp_scratch.reserve((size_t)7 * n, (size_t)7 * (n + n / 8 + 64)));
  HIP_TRY(h, c.mp_rec.reserve((size_t)3 * n, (size_t)3 * (n + n / 8 + 64)));
  {
    std::vector<std::pair<gorio_apd*, DevCloud*>> one = {{h, &c}};
    const KnnListsOnly only = {c.mp_knn, c.mp_scratch, c.mp_scratch + (size_t)6 * n};
    if (int rc = run_covariances(h, one, &only)) return rc;
  }
  mp_cov_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(c.p4, c.mp_knn, n, k, h->params.regularization, c.mp_rec);
  HIP_TRY(h, hipGetLastError());
  c.mp_built(k, kRegMpBase + h->params.regularization);
  return GORIO_OK;
}

GicpMpState* mp_state(gorio_apd* h) {
  if (!h->mp) h->mp = std::make_shared<GicpMpState>();
  GicpMpState* m = h->mp.get();
  m->s.device = h->device;
  m->s.up = h;
  m->s.cloud = h->tgt.get();
  return m;
}

// everything a pass needs: both clouds' covariances, the target's search index, the per-source-point buffers
int mp_prepare(gorio_apd* h) {
  if (int rc = mp_covariances(h, *h->src)) return rc;
  if (int rc = mp_covariances(h, *h->tgt)) return rc;
  if (!h->tgt->idx_valid) {
    std::vector<std::pair<gorio_apd*, DevCloud*>> one = {{h, h->tgt.get()}};
    if (int rc = run_index_build(h, one)) return rc;
  }
  GicpMpState* m = mp_state(h);
  const size_t n = (size_t)h->src->n, cap = n + n / 8 + 256, nblk = (cap + 255) / 256;
  HIP_TRY(h, reserve_group(m->cap, n, cap, m->q, cap, m->merged, 3 * cap, m->part, 28 * nblk));
  HIP_TRY(h, m->out.reserve(28));
  HIP_TRY(h, m->h_out.reserve(sizeof(double) * 28));
  return GORIO_OK;
}

struct MpClock {  // a stage's wall time, taken only while profiling (each stage is then drained)
  gorio_apd* h;
  std::chrono::steady_clock::time_point t0;
  explicit MpClock(gorio_apd* handle) : h(handle) {
    if (h->profiling) t0 = std::chrono::steady_clock::now();
  }
  void lap(double& into) {
    if (!h->profiling) return;
    (void)hipStreamSynchronize(h->stream);
    const auto t1 = std::chrono::steady_clock::now();
    into += std::chrono::duration<double>(t1 - t0).count();
    t0 = t1;
  }
};

// update_correspondences + loss_ls (MPI:130-221) at the float pose T: sums[0..20] H (upper triangle), [21..26] g, [27] points used
int mp_pass(gorio_apd* h, const float* T12, bool keep_merged, double* sums) {
  GicpMpState* m = mp_state(h);
  const DevCloud& s = *h->src;
  const DevCloud& t = *h->tgt;
  const int n = s.n, nblk = (n + 255) / 256;
  MpPose P;
  for (int i = 0; i < 12; ++i) P.m[i] = T12[i];
  h->mp_pass_valid = false;
  h->corr_valid = false;  // every setInput*, clear, swap and method switch resets it: the pass held dies with the clouds it was made from
  m->merged_valid = false;
  MpClock clock(h);
  mp_query_kernel<<<nblk, 256, 0, h->stream>>>(s.p4, n, P, m->q);
  HIP_TRY(h, hipGetLastError());
  clock.lap(m->stage_s[0]);
  long long total = 0;
  if (int rc = search_radius_core(&m->s, reinterpret_cast<const float*>(m->q.get()), n, 16, h->mp_radius, 0, nullptr, &total)) return fail(h, rc, "FastGICPMultiPoints: " + g_search_err);
  clock.lap(m->stage_s[1]);
  mp_linearize_kernel<<<nblk, 256, 0, h->stream>>>(s.mp_rec, m->q, n, m->s.d_kept_offs, m->s.d_ridx, m->s.d_rsqd, t.mp_rec, t.n, P, h->mp_radius, keep_merged ? m->merged.get() : nullptr,
                                                   m->part);
  mp_fold_kernel<<<1, 64, 0, h->stream>>>(m->part, nblk, m->out);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(m->h_out.get(), m->out, sizeof(double) * 28, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  clock.lap(m->stage_s[2]);
  std::memcpy(sums, m->h_out.get(), sizeof(double) * 28);
  m->pass_n = n;
  m->total = total;
  m->used = (int)sums[27];
  m->merged_valid = keep_merged;
  h->mp_pass_valid = true;
  h->corr_valid = true;
  h->omega_valid = false;
  return GORIO_OK;
}

// Eigen::LDLT<6x6>(A).solve(rhs): ldlt6_solve of apd_kernels.hip on the host
void mp_ldlt6_solve(const double* A_in, const double* rhs, double* x) {
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
void mp_exp(const double* w, double* R) {
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
void mp_log(const double* R, double* w) {
  const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double s = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  const double th = std::atan2(s, c);
  const double f = s < 1e-6 ? 1.0 + th * th / 6.0 : th / s;
  for (int a = 0; a < 3; ++a) w[a] = f * v[a];
}

// trans of MPI:131-133, 158-160: [float(exp(x.head)) | x.tail], 12 floats
void mp_trans(const float* x, float* T12) {
  const double w[3] = {(double)x[0], (double)x[1], (double)x[2]};
  double R[9];
  mp_exp(w, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T12[r * 4 + c] = (float)R[r * 3 + c];
    T12[r * 4 + 3] = x[3 + r];
  }
}

// is_converged (MPI:118-127) in float: the scale 1 / epsilon is rounded to float before it multiplies
bool mp_converged(const float* delta, double rot_eps, double trans_eps) {
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

void mp_unpack_H(const double* sums, double* H) {
  int t = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) {
      H[r * 6 + c] = sums[t];
      H[c * 6 + r] = sums[t++];
    }
}

int mp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!guess || !T_out) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = mp_ready(h);
  if (!rc) rc = mp_prepare(h);
  if (rc) return rc;
  GicpMpState* m = mp_state(h);
  const gorio_apd_params& p = h->params;
  float x0[6];
  {
    double R[9], w[3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r * 3 + c] = (double)guess[r * 4 + c];
    mp_log(R, w);
    for (int a = 0; a < 3; ++a) {
      x0[a] = (float)w[a];
      x0[3 + a] = guess[a * 4 + 3];
    }
  }
  bool conv = false;
  int nr = 0, passes = 0;
  double H[36];
  std::memset(H, 0, sizeof(H));
  for (int i = 0; i < p.max_iterations; ++i) {
    nr = i;
    float T12[12];
    mp_trans(x0, T12);
    double sums[28];
    rc = mp_pass(h, T12, false, sums);
    if (rc) return rc;
    ++passes;
    MpClock clock(h);
    mp_unpack_H(sums, H);
    if (sums[27] < 1.0) break;  // no source point has a neighbour: nothing to solve (deviation, gorio_apd.h)
    double dd[6];
    mp_ldlt6_solve(H, sums + 21, dd);
    float delta[6];
    bool finite = true;
    for (int a = 0; a < 6; ++a) {
      delta[a] = (float)dd[a];
      finite = finite && std::isfinite(delta[a]);
    }
    if (!finite) break;  // deviation: the reference's solver substitutes a random step
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
    const bool done = mp_converged(delta, p.rotation_epsilon, p.transformation_epsilon);
    clock.lap(m->stage_s[3]);
    if (done) {
      conv = true;
      break;
    }
  }
  m->passes = passes;
  float T12[12];
  mp_trans(x0, T12);
  for (int i = 0; i < 12; ++i) T_out[i] = T12[i];
  T_out[12] = 0.f; T_out[13] = 0.f; T_out[14] = 0.f; T_out[15] = 1.f;
  if (H_out) std::memcpy(H_out, H, sizeof(H));
  if (converged) *converged = conv ? 1 : 0;
  if (nr_iterations) *nr_iterations = nr;
  if (n_linearize) *n_linearize = passes;
  return GORIO_OK;
}

}  // namespace

extern "C" {

int gorio_apd_set_gicp_mp_params(gorio_apd_t* h, double neighbor_search_radius) {
  if (!h) return GORIO_ERR_INVALID;
  if (!std::isfinite(neighbor_search_radius) || !(neighbor_search_radius > 0.0)) return fail(h, GORIO_ERR_INVALID, "set_gicp_mp_params: neighbor_search_radius must be finite and > 0");
  h->mp_radius = neighbor_search_radius;
  h->mp_pass_valid = false;
  return GORIO_OK;
}

int gorio_apd_get_gicp_mp_params(const gorio_apd_t* h, double* neighbor_search_radius) {
  if (!h) return GORIO_ERR_INVALID;
  if (neighbor_search_radius) *neighbor_search_radius = h->mp_radius;
  return GORIO_OK;
}

int gorio_apd_gicp_mp_get_covariances(gorio_apd_t* h, int which, int capacity, int* n, float* cov) {
  if (!h || !n || (which != 0 && which != 1)) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_covariances: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  const std::shared_ptr<DevCloud>& cp = which == 0 ? h->src : h->tgt;
  DevCloud& c = *cp;
  if (!c.present) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_covariances: that cloud is not set");
  if (mp_shared_mismatch(h, cp)) return fail(h, GORIO_ERR_INVALID, "gicp_mp_get_covariances: the shared cloud's covariances were made with another k_correspondences or regularization");
  if (int rc = mp_cloud_ready(h, c, which == 0 ? "source" : "target")) return rc;
  if (int rc = mp_covariances(h, c)) return rc;
  *n = c.n;
  if (capacity < c.n || !cov) return GORIO_OK;
  std::vector<float> rec((size_t)12 * c.n);
  HIP_TRY(h, hipMemcpyAsync(rec.data(), c.mp_rec, sizeof(float) * 12 * (size_t)c.n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < c.n; ++i)
    for (int t = 0; t < 6; ++t) cov[6 * (size_t)i + t] = rec[12 * (size_t)i + 3 + t];
  return GORIO_OK;
}

int gorio_apd_gicp_mp_pass(gorio_apd_t* h, const float T16[16], int* used, long long* total, double* H, double* g) {
  if (!h || !T16) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(h, GORIO_ERR_STATE, "gicp_mp_pass: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = mp_ready(h);
  if (!rc) rc = mp_prepare(h);
  if (rc) return rc;
  double sums[28];
  rc = mp_pass(h, T16, true, sums);
  if (rc) return rc;
  if (used) *used = (int)sums[27];
  if (total) *total = h->mp->total;
  if (H) mp_unpack_H(sums, H);
  if (g) std::memcpy(g, sums + 21, sizeof(double) * 6);
  return GORIO_OK;
}

int gorio_apd_gicp_mp_get_neighbors(gorio_apd_t* h, long long capacity, int* n_queries, long long* total, long long* offsets, int* idx, float* sqd) {
  if (!h || !n_queries || !total) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_neighbors: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  if (!h->corr_valid || !h->mp_pass_valid || !h->mp) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_neighbors: no pass is held (gorio_apd_gicp_mp_pass or an align first)");
  GicpMpState* m = h->mp.get();
  *n_queries = m->pass_n;
  *total = m->total;
  if (capacity < m->total) return GORIO_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  if (offsets) std::copy(m->s.r_offs.begin(), m->s.r_offs.end(), offsets);
  if (m->total > 0 && idx) HIP_TRY(h, hipMemcpyAsync(idx, m->s.d_ridx, sizeof(int) * (size_t)m->total, hipMemcpyDeviceToHost, h->stream));
  if (m->total > 0 && sqd) HIP_TRY(h, hipMemcpyAsync(sqd, m->s.d_rsqd, sizeof(float) * (size_t)m->total, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_apd_gicp_mp_get_merged(gorio_apd_t* h, int capacity, int* n, float* mean_B, float* cov_B, int* used) {
  if (!h || !n) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_merged: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  if (!h->corr_valid || !h->mp_pass_valid || !h->mp || !h->mp->merged_valid) return fail(h, GORIO_ERR_STATE, "gicp_mp_get_merged: no merged distributions are held (gorio_apd_gicp_mp_pass first; an align keeps none)");
  GicpMpState* m = h->mp.get();
  *n = m->pass_n;
  if (capacity < m->pass_n) return GORIO_OK;
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<float> rec((size_t)12 * m->pass_n);
  HIP_TRY(h, hipMemcpyAsync(rec.data(), m->merged, sizeof(float) * 12 * (size_t)m->pass_n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < m->pass_n; ++i) {
    const float* r = rec.data() + 12 * (size_t)i;
    if (mean_B)
      for (int t = 0; t < 3; ++t) mean_B[3 * (size_t)i + t] = r[t];
    if (cov_B)
      for (int t = 0; t < 6; ++t) cov_B[6 * (size_t)i + t] = r[3 + t];
    if (used) used[i] = r[9] != 0.f ? 1 : 0;
  }
  return GORIO_OK;
}

int gorio_apd_gicp_mp_diag(const gorio_apd_t* h, int* passes, int* used, long long* total, double* stage_seconds) {
  if (!h) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(const_cast<gorio_apd_t*>(h), GORIO_ERR_STATE, "gicp_mp_diag: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  const GicpMpState* m = h->mp.get();
  if (passes) *passes = m ? m->passes : 0;
  if (used) *used = m ? m->used : 0;
  if (total) *total = m ? m->total : 0;
  if (stage_seconds)
    for (int t = 0; t < 4; ++t) stage_seconds[t] = m ? m->stage_s[t] : 0.0;
  return GORIO_OK;
}

}  // extern "C"
