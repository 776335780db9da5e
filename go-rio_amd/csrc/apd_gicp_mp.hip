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
//   mp_*_batch_kernel     query, linearise and fold over the (job, block) entries of a batch round, calling the bodies of the three above
//
// The shell (6 x 6 LDLT, exp / log, update, convergence) runs on the host between passes: the radius search synchronises once per pass
// for its total anyway, and the pass ends with one copy back of 28 doubles.  It is the resumable MpMachine of gicp_mp_machine.h, which
// gorio_apd_align drives for one handle and gorio_apd_gicp_mp_align_batch for many in lock-step rounds (mp_run_batch).
#include <hip/hip_runtime.h>

#include <chrono>

#include "gicp_mp_machine.h"

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
__device__ __forceinline__ void mp_query_point(const float4* __restrict__ pts, int n, const MpPose& T, float4* __restrict__ q, int i) {
  if (i >= n) return;
  const float4 p = pts[i];
  float x, y, z;
  transform_f(T.m, p.x, p.y, p.z, x, y, z);
  q[i] = make_float4(x, y, z, 0.f);
}
__global__ __launch_bounds__(256) void mp_query_kernel(const float4* __restrict__ pts, int n, MpPose T, float4* __restrict__ q) {
  mp_query_point(pts, n, T, q, blockIdx.x * 256 + threadIdx.x);
}

// grid ceil(n / 256), block 256.  src_rec / tgt_rec: the records of mp_cov_kernel; q: the transformed source of THIS pose; offs / idx /
// sqd: the CSR of the radius search (idx and sqd may be null when it is empty).  merged (may be null): per source point mean_B, cov_B
// and the used flag as three float4 (m0 m1 m2 c00 | c01 c02 c11 c12 | c22 used 0 0).  partials: [blocks][28] = 21 H (upper triangle,
// row-major), 6 g, the points used.
// The work of ONE workgroup: source points [256 blk, 256 blk + 256), their 28 sums to block_out[0..27].  mp_linearize_kernel runs it for one
// handle, mp_linearize_batch_kernel for a (job, block) entry of a batch: one body, one summation order, the same bits.
__device__ __forceinline__ void mp_linearize_block(const float4* __restrict__ src_rec, const float4* __restrict__ q, int n, const long long* __restrict__ offs,
                                                   const int* __restrict__ idx, const float* __restrict__ sqd, const float4* __restrict__ tgt_rec, int n_tgt, const MpPose& T,
                                                   double radius, float4* __restrict__ merged, int blk, double* __restrict__ block_out) {
  const int i = blk * 256 + threadIdx.x;
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
  if (threadIdx.x < 28) block_out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void mp_linearize_kernel(const float4* __restrict__ src_rec, const float4* __restrict__ q, int n, const long long* __restrict__ offs,
                                                           const int* __restrict__ idx, const float* __restrict__ sqd, const float4* __restrict__ tgt_rec, int n_tgt, MpPose T,
                                                           double radius, float4* __restrict__ merged, double* __restrict__ partials) {
  mp_linearize_block(src_rec, q, n, offs, idx, sqd, tgt_rec, n_tgt, T, radius, merged, blockIdx.x, partials + (size_t)blockIdx.x * 28);
}

// grid 1, block 64: out[t] = the nblk partials of term t added in block order, lane t of one wave
__global__ __launch_bounds__(64) void mp_fold_kernel(const double* __restrict__ partials, int nblk, double* __restrict__ out) { fold_wave<28>(partials, nblk, out); }

// ---- the batched align (gorio_apd_gicp_mp_align_batch): the three launches above once more, each over the pending handles of a round.
// One handle's pass of a round.  Workgroups [first, first + nblk) of the query and the linearise launch belong to it, and so do the
// partial slots of the same numbers.
struct MpJob {
  const float4* src_p4;
  const float4* src_rec;
  float4* q;
  const long long* offs;  // the CSR of the handle's own search state (set after the search of the round)
  const int* idx;
  const float* sqd;
  const float4* tgt_rec;
  double radius;
  MpPose T;
  int n, n_tgt, first, nblk;
};
// grid: the jobs' blocks added up, block 256.  blocks: the round table (batch_rounds.h), job < number of jobs, blk < jobs[job].nblk
__global__ __launch_bounds__(256) void mp_query_batch_kernel(const MpJob* __restrict__ jobs, const BlockRef* __restrict__ blocks) {
  const BlockRef w = load_uniform(blocks + blockIdx.x);
  const MpJob j = load_uniform(jobs + w.job);
  mp_query_point(j.src_p4, j.n, j.T, j.q, w.blk * 256 + (int)threadIdx.x);
}
__global__ __launch_bounds__(256) void mp_linearize_batch_kernel(const MpJob* __restrict__ jobs, const BlockRef* __restrict__ blocks, double* __restrict__ partials) {
  const BlockRef w = load_uniform(blocks + blockIdx.x);
  const MpJob j = load_uniform(jobs + w.job);
  mp_linearize_block(j.src_rec, j.q, j.n, j.offs, j.idx, j.sqd, j.tgt_rec, j.n_tgt, j.T, j.radius, nullptr, w.blk, partials + (size_t)(j.first + w.blk) * 28);
}
// grid: the round's jobs, block 64
__global__ __launch_bounds__(64) void mp_fold_batch_kernel(const MpJob* __restrict__ jobs, const double* __restrict__ partials, double* __restrict__ out) {
  const MpJob j = load_uniform(jobs + blockIdx.x);
  fold_wave<28>(partials + (size_t)j.first * 28, j.nblk, out + (size_t)blockIdx.x * 28);
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
  double last_H[36] = {};        // H of the last pass of the last align, single or batched (gorio_apd_gicp_mp_last_hessian)
  double stage_s[4] = {0, 0, 0, 0};  // query transform, radius search, merge + linearise (with fold and copy back), shell: filled while profiling
  // the last batch this handle LED (gorio_apd_gicp_mp_align_batch)
  int b_rounds = 0, b_launches = 0, b_syncs = 0, b_max_round_launches = 0;  // gorio_apd_gicp_mp_batch_diag
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

// the shell -- 6 x 6 LDLT, exp / log, update, convergence, the two deviations -- is the resumable machine of gicp_mp_machine.h
using gorio_mp::MpMachine;
using gorio_mp::mp_unpack_H;

int mp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!guess || !T_out) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = mp_ready(h);
  if (!rc) rc = mp_prepare(h);
  if (rc) return rc;
  GicpMpState* m = mp_state(h);
  const gorio_apd_params& p = h->params;
  MpMachine mc;  // a batch of one: the machine the rounds of mp_run_batch drive, here over the single kernels
  mc.begin(guess, p.max_iterations, p.rotation_epsilon, p.transformation_epsilon);
  while (!mc.done()) {
    float T12[12];
    mc.next_pose(T12);
    double sums[28];
    rc = mp_pass(h, T12, false, sums);
    if (rc) return rc;
    MpClock clock(h);
    mc.consume(sums);
    clock.lap(m->stage_s[3]);
  }
  m->passes = mc.pass;
  mc.results(T_out, m->last_H, converged, nr_iterations, n_linearize);
  if (H_out) std::memcpy(H_out, m->last_H, sizeof(m->last_H));
  return GORIO_OK;
}

struct MpRounds {  // the round table of run_rounds
  using Job = MpJob;
  static constexpr int kSums = 28;
  static constexpr bool kCounts = false, kSecondList = false;
  static void fold(int njobs, hipStream_t stream, const MpJob* jobs, const double* part, const int*, double* out, int*) { mp_fold_batch_kernel<<<njobs, 64, 0, stream>>>(jobs, part, out); }
};

// The lock-step rounds of gorio_apd_gicp_mp_align_batch.  Every unfinished handle has one pass pending at its own pose; a round is one
// query-transform launch over (job, block) entries, the batched radius search (each handle's target through the search state inside the
// handle, its own radius), one merge-and-linearise launch, one fold launch, one copy back of 28 doubles per pending handle and one
// synchronisation -- on the stream and with the tables of hs[0].  Two synchronisations per round: the found offsets and the sums.
int mp_run_batch(gorio_apd** hs, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations) {
  gorio_apd* lead = hs[0];
  for (int q = 0; q < count; ++q) {  // preparation is per handle, not per pass
    gorio_apd* h = hs[q];
    if (int rc = hand_over(lead, h, mp_prepare(h))) return rc;
    if (h->stream != lead->stream) HIP_TRY(lead, hipStreamSynchronize(h->stream));
  }
  GicpMpState* lm = mp_state(lead);
  size_t max_blk = 0;
  for (int q = 0; q < count; ++q) max_blk += (size_t)(hs[q]->src->n + 255) / 256;
  if (batch_rounds::too_many_wg(max_blk, 32)) return fail(lead, GORIO_ERR_INVALID, "gicp_mp_align_batch: too many source points in one batch");
  std::vector<MpMachine> mc((size_t)count);
  for (int q = 0; q < count; ++q) {
    const gorio_apd_params& p = hs[q]->params;
    mc[q].begin(guesses + (size_t)16 * q, p.max_iterations, p.rotation_epsilon, p.transformation_epsilon);
  }
  std::vector<SearchBatchJob> sj((size_t)count);
  RoundCounters ctr;
  int syncs = 0, max_round = 0;
  auto pending = [&](int q) { return mc[q].done() ? -1 : 0; };
  auto fill = [&](int k, int q, MpJob& j) {
    gorio_apd* h = hs[q];
    GicpMpState* m = mp_state(h);
    const DevCloud& s = *h->src;
    j.src_p4 = s.p4;
    j.src_rec = s.mp_rec;
    j.q = m->q;
    j.tgt_rec = h->tgt->mp_rec;
    j.radius = h->mp_radius;
    mc[q].next_pose(j.T.m);
    j.n = s.n;
    j.n_tgt = h->tgt->n;
    h->mp_pass_valid = false;
    h->corr_valid = false;
    m->merged_valid = false;
    sj[k] = SearchBatchJob{&m->s, reinterpret_cast<const float*>(m->q.get()), s.n, 16, h->mp_radius, 0, nullptr, 0};
    const int nblk = (s.n + 255) / 256;
    return batch_rounds::JobShape{nblk, nblk, false};
  };
  // the search in the middle of the round: the job records go up a second time, with the CSR every handle's search state then holds
  auto launch = [&](const RoundView<MpJob>& v, int& launches) {
    const int njobs = v.plan.njobs;
    mp_query_batch_kernel<<<v.plan.wg, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs);
    HIP_TRY(lead, hipGetLastError());
    SearchBatchStats st;
    if (int rc = search_radius_batch_core(sj.data(), njobs, &st)) return fail(lead, rc, "FastGICPMultiPoints: " + g_search_err);
    for (int k = 0; k < njobs; ++k) {  // the search may have moved its buffers
      GicpMpState* m = hs[v.order[k]]->mp.get();
      v.jobs[k].offs = m->s.d_kept_offs;
      v.jobs[k].idx = m->s.d_ridx;
      v.jobs[k].sqd = m->s.d_rsqd;
    }
    if (int rc = upload_staged(lead, lead->round.pin, lead->round.tab, v.jobs, sizeof(MpJob) * (size_t)njobs)) return rc;
    mp_linearize_batch_kernel<<<v.plan.wg, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs, lead->round.part);
    launches += 2 + st.launches;
    max_round = std::max(max_round, launches);
    syncs += 1 + st.syncs;
    return (int)GORIO_OK;
  };
  auto consume = [&](int k, int q, const double* sk, int) {
    gorio_apd* h = hs[q];
    GicpMpState* m = h->mp.get();
    m->pass_n = h->src->n;
    m->total = sj[k].total;
    m->used = (int)sk[27];
    h->mp_pass_valid = true;
    h->corr_valid = true;
    h->omega_valid = false;
    mc[q].consume(sk);
  };
  if (int rc = run_rounds<MpRounds>(lead, count, max_blk, ctr, pending, fill, launch, consume)) return rc;
  for (int q = 0; q < count; ++q) {
    mp_state(hs[q])->passes = mc[q].pass;
    mc[q].results(T_out + (size_t)16 * q, mp_state(hs[q])->last_H, converged ? converged + q : nullptr, nr_iterations ? nr_iterations + q : nullptr, nullptr);
  }
  lm->b_rounds = ctr.rounds;
  lm->b_launches = ctr.launches;
  lm->b_syncs = syncs;
  lm->b_max_round_launches = max_round;
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

int gorio_apd_gicp_mp_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations) {
  if (count == 0) return GORIO_OK;
  if (int rc = batch_front_door("gicp_mp_align_batch", handles, count, guesses, T_out, false, is_mp, "the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)", mp_ready)) return rc;
  gorio_apd* lead = handles[0];
  // members that share a cloud must make its covariances by one rule: the single align refuses the second of them by the cloud's state, which
  // inside a batch the first member's preparation would only set after this check
  std::unordered_map<const DevCloud*, int> owner;
  for (int q = 0; q < count; ++q) {
    gorio_apd* h = handles[q];
    for (const DevCloud* c : {h->src.get(), h->tgt.get()}) {
      const auto it = owner.find(c);
      if (it == owner.end()) {
        owner.emplace(c, q);
        continue;
      }
      const gorio_apd_params &a = handles[it->second]->params, &b = h->params;
      if (a.k_correspondences != b.k_correspondences || a.regularization != b.regularization)
        return fail(lead, GORIO_ERR_INVALID, "gicp_mp_align_batch: handle " + std::to_string(q) + ": it shares a cloud with handle " + std::to_string(it->second) + " but has another k_correspondences or regularization");
    }
  }
  HIP_TRY(lead, hipSetDevice(lead->device));
  return mp_run_batch(handles, count, guesses, T_out, converged, nr_iterations);
}

int gorio_apd_gicp_mp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches, int* syncs, int* max_round_launches) {
  if (!lead) return GORIO_ERR_INVALID;
  if (!is_mp(lead)) return fail(const_cast<gorio_apd_t*>(lead), GORIO_ERR_STATE, "gicp_mp_batch_diag: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  const GicpMpState* m = lead->mp.get();
  if (rounds) *rounds = m ? m->b_rounds : 0;
  if (launches) *launches = m ? m->b_launches : 0;
  if (syncs) *syncs = m ? m->b_syncs : 0;
  if (max_round_launches) *max_round_launches = m ? m->b_max_round_launches : 0;
  return GORIO_OK;
}

int gorio_apd_gicp_mp_last_hessian(const gorio_apd_t* h, double* H36) {
  if (!h || !H36) return GORIO_ERR_INVALID;
  if (!is_mp(h)) return fail(const_cast<gorio_apd_t*>(h), GORIO_ERR_STATE, "gicp_mp_last_hessian: the handle is not in FastGICPMultiPoints mode (gorio_apd_set_method)");
  const GicpMpState* m = h->mp.get();
  if (m) std::memcpy(H36, m->last_H, sizeof(double) * 36);
  else std::memset(H36, 0, sizeof(double) * 36);
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
