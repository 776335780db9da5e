// apd_vgicp_cuda.hip -- fast_gicp::FastVGICPCuda on the device: float per-point covariances (from the k-NN lists, or by an RBF kernel over
// the whole cloud), their regularisation with the point-dropping PLANE filter, a voxel map that averages point covariances, and the GICP
// pair term with the sqrt(num_points) weight under the LsqRegistration shell.  Included by apd_api.hip after apd_ndt_cuda.hip: the float
// instances of the coordinate and key kernels (apd_voxel_group.hip), the key sort, the lookup, the slot table, the pair arithmetic
// (ndtc_pair_terms, third mode) and the fp64 sums are the ones of NDTCuda.
//
// Reference lines (paths relative to the reference's fast_apdgicp/):
//   VH / VI = include/fast_gicp/gicp/fast_vgicp_cuda.hpp and impl/fast_vgicp_cuda_impl.hpp   VC = src/fast_gicp/cuda/fast_vgicp_cuda.cu
//   CE = src/fast_gicp/cuda/covariance_estimation.cu        RB = src/fast_gicp/cuda/covariance_estimation_rbf.cu
//   CR = src/fast_gicp/cuda/covariance_regularization.cu    GV = src/fast_gicp/cuda/gaussian_voxelmap.cu
//   FV = src/fast_gicp/cuda/find_voxel_correspondences.cu   CD = src/fast_gicp/cuda/compute_derivatives.cu
// The definition this file implements is the one of include/gorio_apd.h ("GORIO_METHOD_VGICP_CUDA"); tests/vgicp_cuda_restatement.py
// restates it.
//
//   vgc_cov_knn_kernel      one lane per point: mean and raw moments of its k-NN list in list order, in float (CE:26-34)
//   vgc_cov_rbf_kernel      one lane per (point, block of 512 points): the block staged in LDS, its weighted moments from zero in index
//                           order (RB:116-151); grid (point tiles, blocks), so a 16 k cloud is 2048 workgroups, not 64
//   vgc_cov_rbf_fold_kernel one lane per point: the block partials added in block order, then the finalise of RB:98-108
//   vgc_regularize_kernel   fp64 Jacobi on the six floats, the keep flag of the PLANE filter (CR:29) and the rebuilt covariance (CR:91-117)
//   vgc_scatter_kernel      the scatter of the ordered compaction (compact_count_kernel of apd_scan.hip and block_scan_kernel before it)
//   vgc_accum_kernel        one lane per voxel: n, s += p, Csum += cov in kept order, in float (GV:229-252 without the atomics)
//   vgc_linearize_kernel    ndtc_linearize_body with the GICP term (CD:50-92): Q = cov_B + R_lin cov_A R_lin^T, w = sqrtf(num_points)
//   (compute_error, CD:106-135, over the slots of the last linearise is ndtc_error_part<true> of apd_ndt_cuda.hip, inside lm_solve_vgc_kernel)
//
// Every float expression here is un-fused (the library builds with -ffp-contract=off) and written in ONE order, the restatement's.
#include <hip/hip_runtime.h>

namespace gorio {

// the ordered compaction's count (apd_scan.hip, included at the end of apd_api.hip)
__global__ __launch_bounds__(256) void compact_count_kernel(const unsigned char* __restrict__ keep, int n, int* __restrict__ bcnt);

constexpr int kRbfBlock = 512;  // RB:116: the reference's tile of the pairwise pass; part of the summation order
constexpr int kRbfTerms = 10;   // sw, s[3], S[6] (upper triangle: the reference keeps nine sums)

// grid ceil(n / 256), block 256.  knn: [n][k] indices of this cloud in ascending (distance, index) order, the point itself included.
__global__ __launch_bounds__(256) void vgc_cov_knn_kernel(const float4* __restrict__ pts, const int* __restrict__ knn, int n, int k, float* __restrict__ raw6) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float m0 = 0.f, m1 = 0.f, m2 = 0.f;
  float S00 = 0.f, S01 = 0.f, S02 = 0.f, S11 = 0.f, S12 = 0.f, S22 = 0.f;
  for (int t = 0; t < k; ++t) {
    int j = knn[(size_t)i * k + t];
    j = j < 0 ? 0 : (j >= n ? n - 1 : j);  // the lists hold indices of this cloud
    const float4 p = pts[j];
    m0 = m0 + p.x; m1 = m1 + p.y; m2 = m2 + p.z;
    S00 = S00 + p.x * p.x; S01 = S01 + p.x * p.y; S02 = S02 + p.x * p.z;
    S11 = S11 + p.y * p.y; S12 = S12 + p.y * p.z; S22 = S22 + p.z * p.z;
  }
  const float fk = (float)k;
  m0 = m0 / fk; m1 = m1 / fk; m2 = m2 / fk;
  float* o = raw6 + (size_t)i * 6;
  o[0] = S00 / fk - m0 * m0; o[1] = S01 / fk - m0 * m1; o[2] = S02 / fk - m0 * m2;
  o[3] = S11 / fk - m1 * m1; o[4] = S12 / fk - m1 * m2; o[5] = S22 / fk - m2 * m2;
}

// grid (ceil(n / 256), blocks of this launch), block 256.  Workgroup (x, y): points 256 x .. + 255 against block b = b0 + y of the cloud
// extended with points at the origin to a multiple of 512 (RB:127-129: the padding takes part).  part: [gridDim.y][10][n], term-major so
// that lanes store side by side.  All lanes read the same LDS word per step (a broadcast, no bank conflict).
__global__ __launch_bounds__(256) void vgc_cov_rbf_kernel(const float4* __restrict__ pts, int n, int b0, float g, float m2, float* __restrict__ part) {
  __shared__ float sx[kRbfBlock], sy[kRbfBlock], sz[kRbfBlock];
  const int b = b0 + blockIdx.y;
  for (int t = threadIdx.x; t < kRbfBlock; t += 256) {
    const int j = b * kRbfBlock + t;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n) p = pts[j];
    sx[t] = p.x; sy[t] = p.y; sz[t] = p.z;
  }
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 x = pts[i];
  float sw = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
  float S00 = 0.f, S01 = 0.f, S02 = 0.f, S11 = 0.f, S12 = 0.f, S22 = 0.f;
#pragma unroll 4
  for (int t = 0; t < kRbfBlock; ++t) {
    const float px = sx[t], py = sy[t], pz = sz[t];
    const float dx = x.x - px, dy = x.y - py, dz = x.z - pz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    if (d2 > m2) continue;  // RB:76
    const float w = expf(-g * d2);
    const float w0 = w * px, w1 = w * py, w2 = w * pz;
    sw = sw + w;
    s0 = s0 + w0; s1 = s1 + w1; s2 = s2 + w2;
    S00 = S00 + w0 * px; S01 = S01 + w0 * py; S02 = S02 + w0 * pz;
    S11 = S11 + w1 * py; S12 = S12 + w1 * pz; S22 = S22 + w2 * pz;
  }
  float* o = part + (size_t)blockIdx.y * kRbfTerms * n + i;
  o[0] = sw;
  o[(size_t)n] = s0; o[(size_t)2 * n] = s1; o[(size_t)3 * n] = s2;
  o[(size_t)4 * n] = S00; o[(size_t)5 * n] = S01; o[(size_t)6 * n] = S02;
  o[(size_t)7 * n] = S11; o[(size_t)8 * n] = S12; o[(size_t)9 * n] = S22;
}

// grid ceil(n / 256), block 256.  A cloud whose partials do not fit one launch comes in runs of nb blocks: the running sums start from
// zero (first) or from acc [10][n], and go back there unless this run is the last.
__global__ __launch_bounds__(256) void vgc_cov_rbf_fold_kernel(const float* __restrict__ part, int n, int nb, float* __restrict__ acc, int first, int last,
                                                               float* __restrict__ raw6) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a[kRbfTerms];
#pragma unroll
  for (int q = 0; q < kRbfTerms; ++q) a[q] = first ? 0.f : acc[(size_t)q * n + i];
  for (int b = 0; b < nb; ++b) {
    const float* p = part + (size_t)b * kRbfTerms * n + i;
#pragma unroll
    for (int q = 0; q < kRbfTerms; ++q) a[q] = a[q] + p[(size_t)q * n];
  }
  if (!last) {
#pragma unroll
    for (int q = 0; q < kRbfTerms; ++q) acc[(size_t)q * n + i] = a[q];
    return;
  }
  const float sw = a[0];
  const float m0 = a[1] / sw, m1 = a[2] / sw, m2 = a[3] / sw;
  float* o = raw6 + (size_t)i * 6;
  o[0] = (a[4] - m0 * a[1]) / sw; o[1] = (a[5] - m0 * a[2]) / sw; o[2] = (a[6] - m0 * a[3]) / sw;
  o[3] = (a[7] - m1 * a[2]) / sw; o[4] = (a[8] - m1 * a[3]) / sw; o[5] = (a[9] - m2 * a[3]) / sw;
}

// grid ceil(n / 256), block 256.  reg: gorio_regularization.  sym3_eigen gives the eigenvalues in DESCENDING order: e.w0 is the w2 of
// CR:29 (Eigen sorts ascending), e.w2 its w0.  Every rebuilt matrix is summed in double and rounded to float once.
__global__ __launch_bounds__(256) void vgc_regularize_kernel(const float* __restrict__ raw6, int n, int reg, unsigned char* __restrict__ keep, float* __restrict__ cov6) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* r = raw6 + (size_t)i * 6;
  float* o = cov6 + (size_t)i * 6;
  unsigned char kept = 1;
  if (reg == GORIO_REG_PLANE || reg == GORIO_REG_MIN_EIG) {
    const Eig3 e = sym3_eigen((double)r[0], (double)r[1], (double)r[2], (double)r[3], (double)r[4], (double)r[5]);
    double l0, l1, l2;
    if (reg == GORIO_REG_PLANE) {
      kept = e.w1 > e.w0 * 0.1 ? 1 : 0;  // CR:29
      l0 = 1.0; l1 = 1.0; l2 = 1e-3;
    } else {
      l0 = fmax(1e-3, e.w0); l1 = fmax(1e-3, e.w1); l2 = fmax(1e-3, e.w2);
    }
    o[0] = (float)(l2 * e.v02 * e.v02 + l1 * e.v01 * e.v01 + l0 * e.v00 * e.v00);
    o[1] = (float)(l2 * e.v02 * e.v12 + l1 * e.v01 * e.v11 + l0 * e.v00 * e.v10);
    o[2] = (float)(l2 * e.v02 * e.v22 + l1 * e.v01 * e.v21 + l0 * e.v00 * e.v20);
    o[3] = (float)(l2 * e.v12 * e.v12 + l1 * e.v11 * e.v11 + l0 * e.v10 * e.v10);
    o[4] = (float)(l2 * e.v12 * e.v22 + l1 * e.v11 * e.v21 + l0 * e.v10 * e.v20);
    o[5] = (float)(l2 * e.v22 * e.v22 + l1 * e.v21 * e.v21 + l0 * e.v20 * e.v20);
  } else if (reg == GORIO_REG_FROBENIUS) {  // CR:63-71: (C^-1 / ||C^-1||_F)^-1 = ||C^-1||_F C with C = cov + 1e-3 I
    const double c00 = (double)r[0] + 1e-3, c01 = (double)r[1], c02 = (double)r[2], c11 = (double)r[3] + 1e-3, c12 = (double)r[4], c22 = (double)r[5] + 1e-3;
    double i00, i01, i02, i11, i12, i22;
    inv_sym3(c00, c01, c02, c11, c12, c22, i00, i01, i02, i11, i12, i22);
    const double fro = sqrt(i00 * i00 + i11 * i11 + i22 * i22 + 2.0 * (i01 * i01 + i02 * i02 + i12 * i12));
    o[0] = (float)(fro * c00); o[1] = (float)(fro * c01); o[2] = (float)(fro * c02);
    o[3] = (float)(fro * c11); o[4] = (float)(fro * c12); o[5] = (float)(fro * c22);
  } else {  // NONE, NORMALIZED_MIN_EIG: the reference prints "unimplemented" and leaves the matrices (CR:114-116)
#pragma unroll
    for (int q = 0; q < 6; ++q) o[q] = r[q];
  }
  keep[i] = kept;
}

// grid ceil(n / 256), block 256: position = workgroup offset + kept points of the lower waves + kept lanes below this one
__global__ __launch_bounds__(256) void vgc_scatter_kernel(const float4* __restrict__ pts, const float* __restrict__ cov6, const unsigned char* __restrict__ keep, int n,
                                                          const int* __restrict__ boffs, float4* __restrict__ kept_pts, float* __restrict__ kept_cov6, int* __restrict__ kept_index) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool k = i < n && keep[i];
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if (lane == 0) w[wave] = __popcll(b);
  __syncthreads();
  if (!k) return;
  int pos = boffs[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int q = 0; q < wave; ++q) pos += w[q];
  kept_pts[pos] = pts[i];
  kept_index[pos] = i;
#pragma unroll
  for (int q = 0; q < 6; ++q) kept_cov6[(size_t)pos * 6 + q] = cov6[(size_t)i * 6 + q];
}

// one lane per voxel start of the sorted keys (rank as in ndtc_accum_kernel); pts / cov6: the kept points and their regularised covariances
__global__ __launch_bounds__(256) void vgc_accum_kernel(const unsigned long long* __restrict__ keys, const float4* __restrict__ pts, const float* __restrict__ cov6, int n,
                                                        const int* __restrict__ offsets, unsigned long long* __restrict__ vkey, float* __restrict__ vmean,
                                                        float* __restrict__ vcov6, int* __restrict__ vnum) {
  const RunStart rs = cell_run_start<31>(keys, n);
  if (!rs.start) return;
  const int p = blockIdx.x * 256 + threadIdx.x, rank = offsets[blockIdx.x] + rs.local;
  const unsigned long long vox = keys[p] >> 31;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  float c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int cnt = 0;
  for (int j = p; j < n && (keys[j] >> 31) == vox; ++j) {  // kept order inside the voxel
    const int idx = (int)(keys[j] & 0x7fffffffull);
    const float4 v = pts[idx];
    const float* q = cov6 + (size_t)idx * 6;
    s0 = s0 + v.x; s1 = s1 + v.y; s2 = s2 + v.z;
#pragma unroll
    for (int a = 0; a < 6; ++a) c[a] = c[a] + q[a];
    ++cnt;
  }
  const float fn = (float)cnt;
  float* om = vmean + (size_t)rank * 3;
  om[0] = s0 / fn; om[1] = s1 / fn; om[2] = s2 / fn;
  float* oc = vcov6 + (size_t)rank * 6;
#pragma unroll
  for (int a = 0; a < 6; ++a) oc[a] = c[a] / fn;
  vkey[rank] = vox;
  vnum[rank] = cnt;
}

// grid: (ceil(max n_items * n_off / 256), 1, pairs), block 256
__global__ __launch_bounds__(256) void vgc_linearize_kernel(const PairDesc* __restrict__ descs, const NdtcPair* __restrict__ pairs) {
  const GridPos gp = xcd_grid_pos();
  ndtc_linearize_body<true, true>(descs[gp.z], pairs[gp.z], gp.x);
}

}  // namespace gorio
