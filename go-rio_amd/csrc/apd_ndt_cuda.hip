// apd_ndt_cuda.hip -- fast_gicp::NDTCuda on the device: point-to-distribution (P2D) and distribution-to-distribution (D2D) NDT with a Cauchy
// kernel under the LsqRegistration shell.  Included by apd_api.hip after apd_voxel.hip: it reuses the cell grouping of apd_voxel_group.hip
// (voxel_axis, the bounding-box and key kernels in float), the binary-search lookup of the FastVGICP map, the 21 + 6 + 1 partial layout and lm_solve_body.
//
// Reference lines (paths relative to the reference's fast_apdgicp/):
//   NC = src/fast_gicp/cuda/ndt_cuda.cu                 ND = src/fast_gicp/cuda/ndt_compute_derivatives.cu
//   GV = src/fast_gicp/cuda/gaussian_voxelmap.cu        FV = src/fast_gicp/cuda/find_voxel_correspondences.cu
//   CR = src/fast_gicp/cuda/covariance_regularization.cu
// The definition this file implements is the one of include/gorio_apd.h ("GORIO_METHOD_NDT_CUDA"); tests/ndt_cuda_restatement.py restates it.
//
//   cell_coord_bbox_kernel<float>, cell_key_kernel<float> (apd_voxel_group.hip)   calc_voxel_coord (GV:118-121) of every point IN FLOAT
//   ndtc_accum_kernel       one lane per voxel: n, s += p, S += p p^T in float in input order (GV:133-141 without the atomics), the finalise
//                           of GV:185-188, and the MIN_EIG rebuild (CR:73-87) by the fp64 Jacobi of this library
//   ndtc_linearize_kernel   one lane per (offset, item) slot, offset-major: q = Tf * item in float, lookup (FV:32-60), the pair terms of
//                           ND:50-91 (P2D) / ND:120-163 (D2D) in float, widened and summed in fp64: wave -> block -> blocks in block order
//   ndtc_error_part         compute_error (NC:162-177) over the slots of the last linearise at another pose (inside lm_solve_ndtc_kernel)
//
// Every float expression here is un-fused (the library builds with -ffp-contract=off) and written in ONE order, the restatement's.
#include <hip/hip_runtime.h>

namespace gorio {

// one lane per voxel start of the sorted keys (rank as in vg_accum_kernel).  cov_raw: the 9 floats of GV:188, row-major (mean s^T is not
// symmetric in float); cov6: upper triangle of sum_i max(1e-3, lambda_i) v_i v_i^T, (lambda, v) of the UPPER triangle of cov_raw widened to
// double, summed in double and rounded once (the reference: Eigen's float closed form and V diag V^-1, CR:73-87)
__global__ __launch_bounds__(256) void ndtc_accum_kernel(const unsigned long long* __restrict__ keys, const float4* __restrict__ pts, int n, const int* __restrict__ offsets,
                                                         unsigned long long* __restrict__ vkey, float* __restrict__ vmean, float* __restrict__ vraw, float* __restrict__ vcov6,
                                                         int* __restrict__ vnum) {
  const RunStart rs = cell_run_start<31>(keys, n);
  if (!rs.start) return;
  const int p = blockIdx.x * 256 + threadIdx.x, rank = offsets[blockIdx.x] + rs.local;
  const unsigned long long vox = keys[p] >> 31;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  float S00 = 0.f, S01 = 0.f, S02 = 0.f, S11 = 0.f, S12 = 0.f, S22 = 0.f;
  int cnt = 0;
  for (int j = p; j < n && (keys[j] >> 31) == vox; ++j) {  // input order inside the voxel
    const float4 v = pts[(int)(keys[j] & 0x7fffffffull)];
    s0 = s0 + v.x; s1 = s1 + v.y; s2 = s2 + v.z;
    S00 = S00 + v.x * v.x; S01 = S01 + v.x * v.y; S02 = S02 + v.x * v.z;
    S11 = S11 + v.y * v.y; S12 = S12 + v.y * v.z; S22 = S22 + v.z * v.z;
    ++cnt;
  }
  const float fn = (float)cnt;
  const float m0 = s0 / fn, m1 = s1 / fn, m2 = s2 / fn;
  float* om = vmean + (size_t)rank * 3;
  om[0] = m0; om[1] = m1; om[2] = m2;
  float* r = vraw + (size_t)rank * 9;
  r[0] = (S00 - m0 * s0) / fn; r[1] = (S01 - m0 * s1) / fn; r[2] = (S02 - m0 * s2) / fn;
  r[3] = (S01 - m1 * s0) / fn; r[4] = (S11 - m1 * s1) / fn; r[5] = (S12 - m1 * s2) / fn;
  r[6] = (S02 - m2 * s0) / fn; r[7] = (S12 - m2 * s1) / fn; r[8] = (S22 - m2 * s2) / fn;
  const Eig3 e = sym3_eigen((double)r[0], (double)r[1], (double)r[2], (double)r[4], (double)r[5], (double)r[8]);
  const double w0 = fmax(1e-3, e.w0), w1 = fmax(1e-3, e.w1), w2 = fmax(1e-3, e.w2);
  float* oc = vcov6 + (size_t)rank * 6;
  oc[0] = (float)(w0 * e.v00 * e.v00 + w1 * e.v01 * e.v01 + w2 * e.v02 * e.v02);
  oc[1] = (float)(w0 * e.v00 * e.v10 + w1 * e.v01 * e.v11 + w2 * e.v02 * e.v12);
  oc[2] = (float)(w0 * e.v00 * e.v20 + w1 * e.v01 * e.v21 + w2 * e.v02 * e.v22);
  oc[3] = (float)(w0 * e.v10 * e.v10 + w1 * e.v11 * e.v11 + w2 * e.v12 * e.v12);
  oc[4] = (float)(w0 * e.v10 * e.v20 + w1 * e.v11 * e.v21 + w2 * e.v12 * e.v22);
  oc[5] = (float)(w0 * e.v20 * e.v20 + w1 * e.v21 * e.v21 + w2 * e.v22 * e.v22);
  vkey[rank] = vox;
  vnum[rank] = cnt;
}

// q = R p + t per row, left to right, un-fused, in float (Eigen: R * mean_A + t, ND:72)
__device__ __forceinline__ void ndtc_transform(const float* __restrict__ T, float x, float y, float z, float& qx, float& qy, float& qz) {
  float a = T[0] * x;
  a = a + T[1] * y;
  a = a + T[2] * z;
  qx = a + T[3];
  a = T[4] * x;
  a = a + T[5] * y;
  a = a + T[6] * z;
  qy = a + T[7];
  a = T[8] * x;
  a = a + T[9] * y;
  a = a + T[10] * z;
  qz = a + T[11];
}

// The terms of one (item, voxel) pair, all in float (ND:50-91, ND:120-163).  Te: evaluation pose, Tl: pose of the linearisation (its
// rotation enters the D2D covariance).  out[0..20] upper triangle of H, [21..26] b, [27] err; with ERR_ONLY only out[27] is written.
// Order (the restatement's pair_terms): a' = R a + t; e = mean_B - a'; Q = cov_B (+ (R_l cov_A) R_l^T); C = adj(Q) / det(Q) with
// adj as written below and det = (q00 c00 + q01 c10) + q02 c20; w = k^2 / (k^2 + n n), n = sqrtf((e0 e0 + e1 e1) + e2 e2);
// J = [skew(a') | -I]; A = w J^T; B = A C; H = B J; b = B e; err = ((w e)^T C) e; every 3-term sum left to right, zeros included.
// VGICP (fast_gicp::FastVGICPCuda, apd_vgicp_cuda.hip; CD:50-92): the same terms with w = sqrtf((float)num_points) instead of the Cauchy kernel.
template <bool D2D, bool ERR_ONLY, bool VGICP = false>
__device__ __forceinline__ void ndtc_pair_terms(const NdtcPair& np, int item, int v, const float* __restrict__ Te, const float* __restrict__ Tl, float ax, float ay, float az,
                                                float (&out)[28]) {
  float a[3];
  ndtc_transform(Te, ax, ay, az, a[0], a[1], a[2]);
  const float* mb = np.map.mean + (size_t)v * 3;
  const float* cb = np.map.cov6 + (size_t)v * 6;
  float e[3];
  e[0] = mb[0] - a[0]; e[1] = mb[1] - a[1]; e[2] = mb[2] - a[2];
  float q[3][3];
  q[0][0] = cb[0]; q[0][1] = cb[1]; q[0][2] = cb[2];
  q[1][0] = cb[1]; q[1][1] = cb[3]; q[1][2] = cb[4];
  q[2][0] = cb[2]; q[2][1] = cb[4]; q[2][2] = cb[5];
  if constexpr (D2D) {
    const float* ca = np.item_cov6 + (size_t)item * 6;
    const float A[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
    const float R[3][3] = {{Tl[0], Tl[1], Tl[2]}, {Tl[4], Tl[5], Tl[6]}, {Tl[8], Tl[9], Tl[10]}};
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) M[i][j] = (R[i][0] * A[0][j] + R[i][1] * A[1][j]) + R[i][2] * A[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) q[i][j] = q[i][j] + ((M[i][0] * R[j][0] + M[i][1] * R[j][1]) + M[i][2] * R[j][2]);
  }
  float c[3][3];
  c[0][0] = q[1][1] * q[2][2] - q[1][2] * q[2][1];
  c[0][1] = q[0][2] * q[2][1] - q[0][1] * q[2][2];
  c[0][2] = q[0][1] * q[1][2] - q[0][2] * q[1][1];
  c[1][0] = q[1][2] * q[2][0] - q[1][0] * q[2][2];
  c[1][1] = q[0][0] * q[2][2] - q[0][2] * q[2][0];
  c[1][2] = q[0][2] * q[1][0] - q[0][0] * q[1][2];
  c[2][0] = q[1][0] * q[2][1] - q[1][1] * q[2][0];
  c[2][1] = q[0][1] * q[2][0] - q[0][0] * q[2][1];
  c[2][2] = q[0][0] * q[1][1] - q[0][1] * q[1][0];
  const float det = (q[0][0] * c[0][0] + q[0][1] * c[1][0]) + q[0][2] * c[2][0];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i][j] = c[i][j] / det;
  float w;
  if constexpr (VGICP) {
    w = sqrtf((float)np.map.num[v]);
  } else {
    const float k2 = np.map.res * np.map.res;
    const float nrm = sqrtf((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    w = k2 / (k2 + nrm * nrm);
  }
  {
    const float we0 = w * e[0], we1 = w * e[1], we2 = w * e[2];
    const float u0 = (we0 * c[0][0] + we1 * c[1][0]) + we2 * c[2][0];
    const float u1 = (we0 * c[0][1] + we1 * c[1][1]) + we2 * c[2][1];
    const float u2 = (we0 * c[0][2] + we1 * c[1][2]) + we2 * c[2][2];
    out[27] = (u0 * e[0] + u1 * e[1]) + u2 * e[2];
  }
  if constexpr (!ERR_ONLY) {
    const float J[3][6] = {{0.f, -a[2], a[1], -1.f, 0.f, 0.f}, {a[2], 0.f, -a[0], 0.f, -1.f, 0.f}, {-a[1], a[0], 0.f, 0.f, 0.f, -1.f}};
    float B[6][3];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const float A0 = w * J[0][i], A1 = w * J[1][i], A2 = w * J[2][i];
#pragma unroll
      for (int j = 0; j < 3; ++j) B[i][j] = (A0 * c[0][j] + A1 * c[1][j]) + A2 * c[2][j];
    }
    int t = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) out[t++] = (B[i][0] * J[0][j] + B[i][1] * J[1][j]) + B[i][2] * J[2][j];
#pragma unroll
    for (int i = 0; i < 6; ++i) out[21 + i] = (B[i][0] * e[0] + B[i][1] * e[1]) + B[i][2] * e[2];
  }
}

__device__ __forceinline__ void ndtc_item(const NdtcPair& np, int i, float& x, float& y, float& z) {
  const float* p = np.item + (size_t)i * np.item_stride;
  x = p[0]; y = p[1]; z = p[2];
}

// The linearisation of one pair's slots by one workgroup: called by the single and the batched launch alike (grid z = pair), so a batch
// returns the single align's bits.  Slot t = o * n_items + i (offset-major, FV:83-111).  VGICP: no num_points gate (CD:50-92).
template <bool D2D, bool VGICP = false>
__device__ __forceinline__ void ndtc_linearize_body(const PairDesc& pd, const NdtcPair& np, unsigned int bx) {
  const PairState* __restrict__ st = pd.state;
  if (st->done) return;
  const long long total = (long long)np.n_items * np.n_off;
  if ((long long)bx * 256 >= total) return;
  const long long t = (long long)bx * 256 + threadIdx.x;
  float Tf[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) Tf[q] = (float)st->x0[q];  // trans.cast<float>(), NC:144
  if (bx == 0 && threadIdx.x < 12) np.tlin[threadIdx.x] = (float)st->x0[threadIdx.x];  // linearized_x, NC:149

  double acc[28];
#pragma unroll
  for (int q = 0; q < 28; ++q) acc[q] = 0.0;
  if (t < total) {
    const int o = (int)(t / np.n_items), i = (int)(t - (long long)o * np.n_items);
    float ax, ay, az, qx, qy, qz;
    ndtc_item(np, i, ax, ay, az);
    ndtc_transform(Tf, ax, ay, az, qx, qy, qz);
    int c0, c1, c2;
    bool ok = voxel_axis(qx, np.map.res, c0);
    ok = voxel_axis(qy, np.map.res, c1) && ok;
    ok = voxel_axis(qz, np.map.res, c2) && ok;
    const int* off = np.offsets + 3 * o;
    const int v = ok ? voxel_lookup(np.map, c0 + off[0], c1 + off[1], c2 + off[2]) : -1;
    np.slots[t] = v;
    if (v >= 0 && (VGICP || np.map.num[v] > 6)) {  // ND:61, ND:132
      float out[28];
      ndtc_pair_terms<D2D, false, VGICP>(np, i, v, Tf, Tf, ax, ay, az, out);
#pragma unroll
      for (int q = 0; q < 28; ++q) acc[q] = (double)out[q];
    }
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
  if (threadIdx.x < 28) pd.partials[(size_t)bx * 28 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// grid: (ceil(max n_items * n_off / 256), 1, pairs), block 256
template <bool D2D>
__global__ __launch_bounds__(256) void ndtc_linearize_kernel(const PairDesc* __restrict__ descs, const NdtcPair* __restrict__ pairs) {
  const GridPos gp = xcd_grid_pos();
  ndtc_linearize_body<D2D>(descs[gp.z], pairs[gp.z], gp.x);
}

// compute_error (NC:162-177; VGICP: CD:106-135, no num_points gate): the slots of the last linearise at pose T, R_lin from tlin; this
// thread's strided share
template <bool VGICP>
__device__ double ndtc_error_part(const PairDesc& pd, const NdtcPair& np, const double* __restrict__ T) {
  const long long total = (long long)np.n_items * np.n_off;
  float Te[12], Tl[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) {
    Te[q] = (float)T[q];
    Tl[q] = np.tlin[q];
  }
  double sum = 0.0;
  for (long long t = threadIdx.x; t < total; t += blockDim.x) {
    const int v = np.slots[t];
    if (v < 0 || (!VGICP && np.map.num[v] <= 6)) continue;
    const int i = (int)(t % np.n_items);
    float ax, ay, az;
    ndtc_item(np, i, ax, ay, az);
    float out[28];
    if constexpr (VGICP) ndtc_pair_terms<true, true, true>(np, i, v, Te, Tl, ax, ay, az, out);
    else if (np.d2d) ndtc_pair_terms<true, true>(np, i, v, Te, Tl, ax, ay, az, out);
    else ndtc_pair_terms<false, true>(np, i, v, Te, Tl, ax, ay, az, out);
    sum += (double)out[27];
  }
  return sum;
}

}  // namespace gorio
