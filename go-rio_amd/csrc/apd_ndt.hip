// apd_ndt.hip -- NDT_OMP registration (include/gorio_ndt.h): pclomp::NormalDistributionsTransform with the DIRECT1 / 7 / 26 searches, and
// the radius neighbourhood of pcl::NormalDistributionsTransform / pclomp's KDTREE (gorio_ndt_set_radius_search).
// Included by apd_api.hip after apd_sc.hip (it reuses the tiled bitonic sort, the voxel-start count / scan kernels, the fp64 Jacobi of
// the covariance code and the 28-value wave reduction of linearize_kernel).
//
// NDT = ndt_omp_impl.hpp, NDTH = ndt_omp.h, VGC = voxel_grid_covariance_omp_impl.hpp under ndt_omp/include/pclomp of the Go-RIO sources.
//   voxel map      ndt_bbox_kernel        bounding box of the finite target points (integer atomics on an order-preserving code)
//                  ndt_key_kernel         leaf index in the float arithmetic of VGC:218-223, key = leaf index << 31 | point index
//                  (enqueue_tiled_sort; cell_count_kernel, block_scan_kernel of apd_voxel_group.hip)
//                  ndt_leaf_kernel        one lane per leaf: sums in input order in fp64 (VGC:233-237), mean, covariance, Jacobi
//                                         eigen-decomposition, inflation, inverse, the two disabling rules (VGC:293-364)
//   derivatives    ndt_derivative_kernel  one lane per source point: float transform, <= 26 leaf lookups (binary search over the ascending
//                                         leaf indices), computePointDerivatives / updateDerivatives in float (NDT:398-537) or
//                                         updateHessian in double (NDT:613-645); 28 fp64 accumulators, wave_sum28, one partial per block
//                  ndt_fold_kernel        the block partials in block order -> 28 doubles
//   batch          ndt_derivative_batch_kernel, ndt_fold_batch_kernel: the same two bodies (ndt_derivative_block, ndt_fold_sum) for the
//                                         pending evaluations of many handles: a job table and a per-workgroup (job, local block) table
//   score          ndt_score_kernel       calculateScore (NDT:935-983), one double per block, ndt_fold_kernel; ndt_score_batch_kernel runs
//                                         the same body (ndt_score_block) over the job table of the batch for many handles
//   radius mode    ndt_centroid_count_kernel, ndt_centroid_compact_kernel: once per map, the ordered compaction of the eligible leaves' float
//                                         centroids (VGC:282-326) into SoA columns + a centroid -> leaf table; their search index is the library's
//                  ndt_query_kernel       the float-transformed source, the queries of the radius search of apd_search.hip (a CSR)
//                  ndt_derivative_csr_kernel, ndt_score_csr_kernel: one lane per source point walks its CSR segment through ndt_pair; the
//                                         same wave_sum28 and block fold.  Batched: ndt_query_batch_kernel, ndt_derivative_csr_batch_kernel,
//                                         ndt_score_csr_batch_kernel run the same bodies over the job table.  The host half that needs the
//                                         search handle's type is apd_ndt_radius.hip
//   device clouds  ndt_adopt_kernel       device arrays, the cloud of a scan pipeline or of a gorio_apd handle into the handle's own
//                                         buffers: the copy and the finiteness check in one pass
//   align          host                   computeTransformation, computeStepLengthMT and its helpers (NDT:81-171, 648-932) as ONE resumable
//                                         machine (NdtMachine): gorio_ndt_align drives one, gorio_ndt_align_batch many in lock-step
// The only device loops are bounded: points of a leaf (<= n), neighbours (<= 26, or a CSR segment of the radius search: <= 27 centroids),
// binary-search steps (<= 32).  Every index that comes from data is range-checked before it addresses memory: a source point outside the
// grid reads nothing, a centroid index or leaf position outside its table is skipped.
#include <hip/hip_runtime.h>

#include "../../include/gorio_search.h"  // the centroid index of the radius mode is a search handle

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace gorio {

constexpr int kNdtCoordLimit = 1 << 30;  // |cell coordinate| below this: offsets and differences stay inside int32

struct NdtGrid {  // VGC:87-103
  int min_b[3], max_b[3], div_b[3];
  int mul1, mul2;  // divb_mul_ = (1, mul1, mul2)
  float inv;       // inverse_leaf_size_
  float leaf;      // leaf_size_
};

struct NdtMapView {
  const int* lidx;     // [nl] ascending linear leaf index
  const int* cnt;      // [nl] nr_points, -1 when disabled
  const double* mean;  // [nl][3]
  const double* icov;  // [nl][9]
  int nl, min_points;
  NdtGrid g;
};

struct NdtEval {  // one evaluation's constants, passed by value
  float T[12];    // rows 0..2 of the float transform
  double ja[24];  // j_ang, NDT:329-346, row-major [8][3]
  double ha[45];  // h_ang with the double d1 row, NDT:351-371, [15][3]
  double d1, d2, d3;
  int n_off;      // 1, 7 or 26
};

// bb (cell_bbox_init_kernel): bb[0..2] min, bb[3..5] max (sc_code of the floats), bb[6] finite points, bb[7] flags
__device__ __forceinline__ bool ndt_finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

__global__ __launch_bounds__(256) void ndt_bbox_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, int* __restrict__ bb) {
  int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN, cnt = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float px = x[i], py = y[i], pz = z[i];
    if (!ndt_finite3(px, py, pz)) continue;  // VGC:213-215
    const int c0 = sc_code(px), c1 = sc_code(py), c2 = sc_code(pz);
    lo0 = min(lo0, c0); lo1 = min(lo1, c1); lo2 = min(lo2, c2);
    hi0 = max(hi0, c0); hi1 = max(hi1, c1); hi2 = max(hi2, c2);
    ++cnt;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo0 = min(lo0, __shfl_down(lo0, off, 64)); lo1 = min(lo1, __shfl_down(lo1, off, 64)); lo2 = min(lo2, __shfl_down(lo2, off, 64));
    hi0 = max(hi0, __shfl_down(hi0, off, 64)); hi1 = max(hi1, __shfl_down(hi1, off, 64)); hi2 = max(hi2, __shfl_down(hi2, off, 64));
    cnt += __shfl_down(cnt, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(bb + 0, lo0); atomicMin(bb + 1, lo1); atomicMin(bb + 2, lo2);
    atomicMax(bb + 3, hi0); atomicMax(bb + 4, hi1); atomicMax(bb + 5, hi2);
    atomicAdd(bb + 6, cnt);
  }
}

// Clouds that are already on the device (gorio_ndt_set_*_device, _set_*_from_scan, _set_target_from_apd): ONE pass copies x, y, z of
// the first n points into (dx, dy, dz) -- each of at least n floats, reserved by the host -- and raises flag[0] for a non-finite
// point (the source check: it must be known before the source held is replaced).  grid ceil(n / 256), block 256.
__global__ __launch_bounds__(256) void ndt_adopt_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, float* __restrict__ dx,
                                                        float* __restrict__ dy, float* __restrict__ dz, int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const float px = x[i], py = y[i], pz = z[i];
    dx[i] = px; dy[i] = py; dz[i] = pz;
    bad = !ndt_finite3(px, py, pz);
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// keys[i] = leaf index << 31 | i, VGC:218-223 in float; ~0 for the sort's padding and for non-finite points (they sort behind the rest).
// A finite point outside the grid (impossible while floor is monotone; kept as the bounds check of what follows) raises bb[7].
__global__ __launch_bounds__(256) void ndt_key_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, int npow2, NdtGrid g,
                                                      unsigned long long* __restrict__ keys, int* __restrict__ bb) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npow2) return;
  unsigned long long key = ~0ull;
  if (i < n) {
    const float px = x[i], py = y[i], pz = z[i];
    if (ndt_finite3(px, py, pz)) {
      const float f0 = floorf(px * g.inv) - (float)g.min_b[0];
      const float f1 = floorf(py * g.inv) - (float)g.min_b[1];
      const float f2 = floorf(pz * g.inv) - (float)g.min_b[2];
      const bool ok = f0 >= 0.0f && f0 < (float)g.div_b[0] && f1 >= 0.0f && f1 < (float)g.div_b[1] && f2 >= 0.0f && f2 < (float)g.div_b[2];
      if (ok) {
        const long long idx = (long long)(int)f0 + (long long)(int)f1 * g.mul1 + (long long)(int)f2 * g.mul2;  // < 2^31, checked on the host
        key = ((unsigned long long)idx << 31) | (unsigned long long)i;
      } else {
        atomicOr(bb + 7, 1);
      }
    }
  }
  keys[i] = key;
}

// general 3 x 3 inverse by cofactors (Eigen's fixed-size inverse), row-major
__device__ __forceinline__ void ndt_inv3(const double* __restrict__ a, double* __restrict__ r) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = a[0] * c00 + a[1] * c01 + a[2] * c02;
  const double s = 1.0 / det;
  r[0] = c00 * s; r[1] = (a[2] * a[7] - a[1] * a[8]) * s; r[2] = (a[1] * a[5] - a[2] * a[4]) * s;
  r[3] = c01 * s; r[4] = (a[0] * a[8] - a[2] * a[6]) * s; r[5] = (a[2] * a[3] - a[0] * a[5]) * s;
  r[6] = c02 * s; r[7] = (a[1] * a[6] - a[0] * a[7]) * s; r[8] = (a[0] * a[4] - a[1] * a[3]) * s;
}

// One lane per leaf start of the sorted keys (rank as in vg_accum_kernel): the second pass of applyFilter, VGC:282-367, on the sums of
// VGC:233-237 taken in input order (the key's low bits ascend inside a leaf).  n = number of finite points = real keys.
__global__ __launch_bounds__(256) void ndt_leaf_kernel(const unsigned long long* __restrict__ keys, const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ z, int n, int n_points, const int* __restrict__ offsets, int min_points, double eig_mult,
                                                       int nl, int* __restrict__ lidx, int* __restrict__ lcnt, double* __restrict__ lmean, double* __restrict__ lraw,
                                                       double* __restrict__ lcov, double* __restrict__ licov, float* __restrict__ lcent) {
  const RunStart rs = cell_run_start<31>(keys, n);
  if (!rs.start) return;
  const int p = blockIdx.x * 256 + threadIdx.x, rank = offsets[blockIdx.x] + rs.local;
  if (rank < 0 || rank >= nl) return;
  const unsigned long long leaf = keys[p] >> 31;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  double c[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;  // the centroid cloud's sums: float, in input order (VGC:242-243)
  int cnt = 0;
  for (int j = p; j < n && (keys[j] >> 31) == leaf; ++j) {
    const int i = (int)(keys[j] & 0x7fffffffull);
    if (i >= n_points) break;
    const double px = (double)x[i], py = (double)y[i], pz = (double)z[i];
    s0 += px; s1 += py; s2 += pz;  // VGC:235
    f0 += x[i]; f1 += y[i]; f2 += z[i];
    c[0] += px * px; c[1] += px * py; c[2] += px * pz;  // VGC:237
    c[3] += py * px; c[4] += py * py; c[5] += py * pz;
    c[6] += pz * px; c[7] += pz * py; c[8] += pz * pz;
    ++cnt;
  }
  const double nd = (double)cnt;
  const double m0 = s0 / nd, m1 = s1 / nd, m2 = s2 / nd;  // VGC:293
  lidx[rank] = (int)leaf;
  double* om = lmean + (size_t)rank * 3;
  om[0] = m0; om[1] = m1; om[2] = m2;
  {
    const float nf = (float)cnt;  // VGC:289: a true division per element
    float* oc = lcent + (size_t)rank * 3;
    oc[0] = f0 / nf; oc[1] = f1 / nf; oc[2] = f2 / nf;
  }
  double raw[9], cov[9], ic[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) raw[q] = cov[q] = ic[q] = 0.0;
  int out_cnt = cnt;
  if (cnt >= min_points) {  // VGC:297
    const double ps[3] = {s0, s1, s2}, mn[3] = {m0, m1, m2};
    const double f = (nd - 1.0) / nd;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        double v = (c[3 * r + q] - 2.0 * (ps[r] * mn[q])) / nd;  // VGC:329
        v = v + mn[r] * mn[q];
        raw[3 * r + q] = v * f;                                  // VGC:330
        cov[3 * r + q] = raw[3 * r + q];
      }
    // SelfAdjointEigenSolver reads the lower triangle (VGC:333); w0 >= w1 >= w2 here, the reference's order is ascending
    const Eig3 e = sym3_eigen(raw[0], raw[3], raw[6], raw[4], raw[7], raw[8]);
    double ev0 = e.w2, ev1 = e.w1;
    const double ev2 = e.w0;
    if (ev0 < 0 || ev1 < 0 || ev2 <= 0) {  // VGC:337-341
      out_cnt = -1;
    } else {
      const double lo = eig_mult * ev2;  // VGC:345
      if (ev0 < lo) {
        ev0 = lo;
        if (ev1 < lo) ev1 = lo;
        // cov_ = evecs_ * eigen_val * evecs_.inverse(), VGC:355; columns in ascending order
        const double V[9] = {e.v02, e.v01, e.v00, e.v12, e.v11, e.v10, e.v22, e.v21, e.v20};
        double Vi[9];
        ndt_inv3(V, Vi);
        const double w[3] = {ev0, ev1, ev2};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int q = 0; q < 3; ++q) cov[3 * r + q] = (V[3 * r] * w[0] * Vi[q] + V[3 * r + 1] * w[1] * Vi[3 + q]) + V[3 * r + 2] * w[2] * Vi[6 + q];
      }
      ndt_inv3(cov, ic);  // VGC:359
      double mx = ic[0], mi = ic[0];
#pragma unroll
      for (int q = 1; q < 9; ++q) {
        mx = ic[q] > mx ? ic[q] : mx;
        mi = ic[q] < mi ? ic[q] : mi;
      }
      if (mx == INFINITY || mi == -INFINITY) out_cnt = -1;  // VGC:360-364
    }
  }
  lcnt[rank] = out_cnt;
#pragma unroll
  for (int q = 0; q < 9; ++q) {
    lraw[(size_t)rank * 9 + q] = raw[q];
    lcov[(size_t)rank * 9 + q] = cov[q];
    licov[(size_t)rank * 9 + q] = out_cnt >= min_points ? ic[q] : 0.0;
  }
}

// ---- the centroid cloud of the radius mode (VGC:282-326): one point per leaf with nr_points >= min_points_per_voxel, in ascending leaf
// index.  A leaf the eigenvalue or the infinity rule disabled afterwards (lcnt == -1: it had the points) stays in the cloud.
__device__ __forceinline__ bool ndt_in_centroid_cloud(int cnt, int min_points) { return cnt == -1 || cnt >= min_points; }

// counts[b] = leaves of block b that are in the cloud.  grid ceil(nl / 256), block 256; block_scan_kernel turns counts into offsets.
__global__ __launch_bounds__(256) void ndt_centroid_count_kernel(const int* __restrict__ lcnt, int nl, int min_points, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < nl && ndt_in_centroid_cloud(lcnt[i], min_points);
  __shared__ int wcnt[4];
  const unsigned long long b = __ballot(in);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

// The ordered compaction: leaf i of the cloud goes to position offsets[block] + (leaves of the cloud before it in the block).  The
// position is checked against nc (the scanned total the buffers were sized for) before it addresses memory.
__global__ __launch_bounds__(256) void ndt_centroid_compact_kernel(const int* __restrict__ lcnt, const float* __restrict__ lcent, int nl, int min_points,
                                                                   const int* __restrict__ offsets, int nc, float* __restrict__ cx, float* __restrict__ cy, float* __restrict__ cz,
                                                                   int* __restrict__ c2l) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool in = i < nl && ndt_in_centroid_cloud(lcnt[i], min_points);
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long b = __ballot(in);
  if (lane == 0) wcnt[wv] = __popcll(b);
  __syncthreads();
  int pos = offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wv; ++w) pos += wcnt[w];
  if (!in || pos < 0 || pos >= nc) return;
  cx[pos] = lcent[(size_t)i * 3];
  cy[pos] = lcent[(size_t)i * 3 + 1];
  cz[pos] = lcent[(size_t)i * 3 + 2];
  c2l[pos] = i;
}

// floor(x / leaf_size) of VGC:379-381 as an int; false when it does not fit (or is not finite)
__device__ __forceinline__ bool ndt_cell(float v, float leaf, int& c) {
  const float f = floorf(v / leaf);
  const bool ok = f > -(float)kNdtCoordLimit && f < (float)kNdtCoordLimit;  // false for NaN
  c = ok ? (int)f : 0;
  return ok;
}

// displacement o of getNeighborhoodAtPoint1 / 7 / getAllNeighborCellIndices (VGC:406-442), without a table
__device__ __forceinline__ void ndt_offset(int n_off, int o, int& d0, int& d1, int& d2) {
  d0 = 0; d1 = 0; d2 = 0;
  if (n_off == 7) {
    if (o > 0) {  // centre, +x, -x, +y, -y, +z, -z (VGC:423-430)
      const int axis = (o - 1) >> 1, sgn = (o & 1) ? 1 : -1;
      d0 = axis == 0 ? sgn : 0;
      d1 = axis == 1 ? sgn : 0;
      d2 = axis == 2 ? sgn : 0;
    }
  } else if (n_off == 26) {  // 13 half cells, then their negatives
    const int h = o < 13 ? o : o - 13, sgn = o < 13 ? 1 : -1;
    if (h < 9) { d0 = h / 3 - 1; d1 = h % 3 - 1; d2 = -1; }
    else if (h < 12) { d0 = h - 10; d1 = -1; d2 = 0; }
    else { d0 = -1; d1 = 0; d2 = 0; }
    d0 *= sgn; d1 *= sgn; d2 *= sgn;
  }
}

// VGC:382-399: the leaf at cell (c + d), or -1.  The diff2min / diff2max test keeps the cell inside the grid BEFORE it becomes an index.
__device__ __forceinline__ int ndt_lookup(const NdtMapView& vm, int c0, int c1, int c2, int d0, int d1, int d2) {
  const NdtGrid& g = vm.g;
  if (g.min_b[0] - c0 > d0 || g.min_b[1] - c1 > d1 || g.min_b[2] - c2 > d2) return -1;
  if (g.max_b[0] - c0 < d0 || g.max_b[1] - c1 < d1 || g.max_b[2] - c2 < d2) return -1;
  const long long lin = (long long)(c0 + d0 - g.min_b[0]) + (long long)(c1 + d1 - g.min_b[1]) * g.mul1 + (long long)(c2 + d2 - g.min_b[2]) * g.mul2;
  int lo = 0, hi = vm.nl;  // first position whose index is >= lin
  for (int step = 0; step < 32 && lo < hi; ++step) {
    const int mid = (lo + hi) >> 1;
    if ((long long)vm.lidx[mid] < lin) lo = mid + 1;
    else hi = mid;
  }
  if (lo >= vm.nl || (long long)vm.lidx[lo] != lin) return -1;
  return vm.cnt[lo] >= vm.min_points ? lo : -1;  // VGC:395
}

template <typename S>
__device__ __forceinline__ S ndt_dot3(S a0, S a1, S a2, S b0, S b1, S b2) {
  S r = a0 * b0;
  r = r + a1 * b1;
  r = r + a2 * b2;
  return r;
}

// One (point, leaf) pair.  S = float: updateDerivatives (NDT:484-537) after computePointDerivatives (NDT:398-440), every float operation
// in one written order, left to right; S = double: updateHessian (NDT:613-645), Hessian only.
// acc: [0] score, [1..6] gradient, [7..27] upper triangle of the Hessian, row-major.
template <typename S, bool HESS>
__device__ __forceinline__ void ndt_pair(const NdtEval& ev, const S (&jx)[8], const S (&hx)[15], float qx, float qy, float qz, const double* __restrict__ mean,
                                         const double* __restrict__ icov, double (&acc)[28]) {
  constexpr bool kFloat = sizeof(S) == 4;
  const S xt0 = (S)((double)qx - mean[0]), xt1 = (S)((double)qy - mean[1]), xt2 = (S)((double)qz - mean[2]);  // NDT:259-262, 492
  S C[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) C[q] = (S)icov[q];  // NDT:494
  const S xC0 = ndt_dot3<S>(xt0, xt1, xt2, C[0], C[3], C[6]);  // x_trans4 * c_inv4
  const S xC1 = ndt_dot3<S>(xt0, xt1, xt2, C[1], C[4], C[7]);
  const S xC2 = ndt_dot3<S>(xt0, xt1, xt2, C[2], C[5], C[8]);
  const S d2 = (S)ev.d2;
  S e;
  if constexpr (kFloat) {
    const S arg = (-d2 * ndt_dot3<S>(xt0, xt1, xt2, xC0, xC1, xC2)) * 0.5f;
    e = (S)exp((double)arg);                 // NDT:499, the correctly rounded float
    const float inc = (float)(-ev.d1 * (double)e);  // NDT:501
    e = d2 * e;
    if (e > 1 || e < 0 || e != e) return;    // NDT:506
    acc[0] += (double)inc;
    e = (S)((double)e * ev.d1);              // NDT:510
  } else {
    e = d2 * exp(-d2 * ndt_dot3<S>(xt0, xt1, xt2, xC0, xC1, xC2) / 2);  // NDT:622
    if (e > 1 || e < 0 || e != e) return;
    e = e * ev.d1;
  }
  // point_gradient4 (NDT:223-224, 407-414), columns
  const S G[6][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, jx[0], jx[1]}, {jx[2], jx[3], jx[4]}, {jx[5], jx[6], jx[7]}};
  S CG[6][3], xCG[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
#pragma unroll
    for (int r = 0; r < 3; ++r) CG[k][r] = ndt_dot3<S>(C[3 * r], C[3 * r + 1], C[3 * r + 2], G[k][0], G[k][1], G[k][2]);  // NDT:512
    xCG[k] = ndt_dot3<S>(xt0, xt1, xt2, CG[k][0], CG[k][1], CG[k][2]);                                                   // NDT:513
    if constexpr (kFloat) acc[1 + k] += (double)(e * xCG[k]);                                                            // NDT:515
  }
  if constexpr (HESS) {
    // blocks (i, j), 3 <= i <= j, of the point Hessian (NDT:421-438): a, b, c have no x component
    const S Hv[6][3] = {{0, hx[0], hx[1]}, {0, hx[2], hx[3]}, {0, hx[4], hx[5]}, {hx[6], hx[7], hx[8]}, {hx[9], hx[10], hx[11]}, {hx[12], hx[13], hx[14]}};
    int t = 7;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) {
        S v = (-d2 * xCG[i]) * xCG[j];
        if (i >= 3) {
          const int b = i == 3 ? j - 3 : (i == 4 ? j - 1 : 5);
          v = v + ndt_dot3<S>(xC0, xC1, xC2, Hv[b][0], Hv[b][1], Hv[b][2]);  // NDT:525
        }
        v = v + ndt_dot3<S>(G[j][0], G[j][1], G[j][2], CG[i][0], CG[i][1], CG[i][2]);  // NDT:519, element (j, i)
        acc[t] += (double)(e * v);                                                     // NDT:529
        ++t;
      }
    }
  }
}

// x_j_ang (NDT:405) and x_h_ang (NDT:418) of one source point, shared by the DIRECT and the radius body
template <typename S, bool HESS>
__device__ __forceinline__ void ndt_point_tables(const NdtEval& ev, float x, float y, float z, S (&jx)[8], S (&hx)[15]) {
  constexpr bool kFloat = sizeof(S) == 4;
#pragma unroll
  for (int r = 0; r < 8; ++r) jx[r] = ndt_dot3<S>((S)ev.ja[3 * r], (S)ev.ja[3 * r + 1], (S)ev.ja[3 * r + 2], (S)x, (S)y, (S)z);  // NDT:405
#pragma unroll
  for (int r = 0; r < 15; ++r) {
    S h2 = (S)ev.ha[3 * r + 2];
    if (kFloat && r == 6) h2 = -h2;  // NDT:383: the float table holds +sy, the double one -sy (NDT:361)
    hx[r] = HESS ? ndt_dot3<S>((S)ev.ha[3 * r], (S)ev.ha[3 * r + 1], h2, (S)x, (S)y, (S)z) : (S)0;  // NDT:418
  }
}

// the 28 sums of a 256-lane workgroup: wave_sum28, then the four waves in a fixed order -> out[0..27]
__device__ __forceinline__ void ndt_block_sum28(const double (&acc)[28], double* __restrict__ out) {
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
  if (threadIdx.x < 28) out[threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// The work of ONE workgroup of 256 lanes, shared by the single and the batched kernel so that the two cannot drift apart: source points
// [256 block, 256 block + 256) of the cloud -> out[0..27], the block's sums (wave_sum28, then the four waves in a fixed order).
template <typename S, bool HESS>
__device__ __forceinline__ void ndt_derivative_block(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, const NdtMapView& vm,
                                                     const NdtEval& ev, int block, double* __restrict__ out) {
  double acc[28];
#pragma unroll
  for (int q = 0; q < 28; ++q) acc[q] = 0.0;
  const int i = block * 256 + threadIdx.x;
  if (i < n) {
    const float x = sx[i], y = sy[i], z = sz[i];
    float qx, qy, qz;
    transform_f(ev.T, x, y, z, qx, qy, qz);
    int c0, c1, c2;
    bool ok = ndt_cell(qx, vm.g.leaf, c0);
    ok = ndt_cell(qy, vm.g.leaf, c1) && ok;
    ok = ndt_cell(qz, vm.g.leaf, c2) && ok;
    if (ok) {
      S jx[8], hx[15];
      ndt_point_tables<S, HESS>(ev, x, y, z, jx, hx);
#pragma unroll 1
      for (int o = 0; o < ev.n_off; ++o) {
        int d0, d1, d2;
        ndt_offset(ev.n_off, o, d0, d1, d2);
        const int leaf = ndt_lookup(vm, c0, c1, c2, d0, d1, d2);
        if (leaf < 0) continue;
        ndt_pair<S, HESS>(ev, jx, hx, qx, qy, qz, vm.mean + (size_t)leaf * 3, vm.icov + (size_t)leaf * 9, acc);
      }
    }
  }
  ndt_block_sum28(acc, out);
}

// ---- the radius mode (gorio_ndt_set_radius_search): the neighbourhood of a point is target_cells_.radiusSearch(x_trans_pt, resolution_)
// (NDT:234-235, 573-574, 948-949) over the centroid cloud.  One query launch writes the float-transformed source, the exact radius
// search of apd_search.hip turns it into a CSR in ascending (distance, centroid index), one launch walks each point's segment.
struct NdtNeighbours {   // the CSR of one evaluation; offs == nullptr: no point has a neighbour (a map without an eligible leaf)
  float4* q;             // [n] the transformed source, written by ndt_query_block
  const long long* offs; // [n + 1]
  const int* idx;        // [offs[n]] centroid indices
  const int* c2l;        // [nc] centroid -> leaf position
  int nc;
};

// q[i] = T * source[i] in the float arithmetic of pcl::transformPointCloud: the bits the search sees are the bits the pair arithmetic reads
__device__ __forceinline__ void ndt_query_block(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, const float* __restrict__ T,
                                                int block, float4* __restrict__ q) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  float qx, qy, qz;
  transform_f(T, sx[i], sy[i], sz[i], qx, qy, qz);
  q[i] = make_float4(qx, qy, qz, 0.0f);
}

// grid: ceil(n / 256), block 256
__global__ __launch_bounds__(256) void ndt_query_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, NdtEval ev,
                                                        float4* __restrict__ q) {
  ndt_query_block(sx, sy, sz, n, ev.T, (int)blockIdx.x, q);
}

// ndt_derivative_block with the neighbours taken from the CSR: the pair terms of a point are added in the order of its segment.  Every
// centroid index and leaf position read from memory is range-checked before it addresses the map.  There is no ndt_cell test here.
template <typename S, bool HESS>
__device__ __forceinline__ void ndt_derivative_csr_block(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, const NdtMapView& vm,
                                                         const NdtEval& ev, const NdtNeighbours& nb, int block, double* __restrict__ out) {
  double acc[28];
#pragma unroll
  for (int q = 0; q < 28; ++q) acc[q] = 0.0;
  const int i = block * 256 + threadIdx.x;
  if (i < n && nb.offs) {
    const long long b = nb.offs[i], e = nb.offs[i + 1];
    if (e > b) {
      const float4 qt = nb.q[i];
      S jx[8], hx[15];
      ndt_point_tables<S, HESS>(ev, sx[i], sy[i], sz[i], jx, hx);
#pragma unroll 1
      for (long long k = b; k < e; ++k) {
        const int c = nb.idx[k];
        if (c < 0 || c >= nb.nc) continue;
        const int leaf = nb.c2l[c];
        if (leaf < 0 || leaf >= vm.nl) continue;
        ndt_pair<S, HESS>(ev, jx, hx, qt.x, qt.y, qt.z, vm.mean + (size_t)leaf * 3, vm.icov + (size_t)leaf * 9, acc);
      }
    }
  }
  ndt_block_sum28(acc, out);
}

// grid: ceil(n / 256), block 256.  One 28-double partial per block.
template <typename S, bool HESS>
__global__ __launch_bounds__(256) void ndt_derivative_csr_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, NdtMapView vm,
                                                                 NdtEval ev, NdtNeighbours nb, double* __restrict__ partials) {
  ndt_derivative_csr_block<S, HESS>(sx, sy, sz, n, vm, ev, nb, (int)blockIdx.x, partials + (size_t)blockIdx.x * 28);
}

// grid: ceil(n / 256), block 256.  One 28-double partial per block.
template <typename S, bool HESS>
__global__ __launch_bounds__(256) void ndt_derivative_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, NdtMapView vm,
                                                             NdtEval ev, double* __restrict__ partials) {
  ndt_derivative_block<S, HESS>(sx, sy, sz, n, vm, ev, (int)blockIdx.x, partials + (size_t)blockIdx.x * 28);
}

// One pending evaluation of gorio_ndt_align_batch.  Its workgroups write the partial slots [first, first + nblk).
struct NdtJob {
  const float *sx, *sy, *sz;
  int n;
  int mode;   // 0 <float, false>, 1 <float, true>, 2 <double, true>, 3 the score
  int first;  // first partial-block slot
  int nblk;   // ceil(n / 256)
  NdtMapView vm;
  NdtEval ev;
  NdtNeighbours nb;  // radius jobs only: q from the start, the CSR once the round's search has run
};

// grid: the sum over the launch's jobs of ceil(n_j / 256), block 256.  wg[blockIdx.x] = (job, job-local block), written by the host with
// the job table; the index is uniform over the workgroup, so the job record comes in through scalar loads.  The host keeps
// wg[].x < number of jobs and wg[].y < jobs[wg[].x].nblk; the partial buffer holds first + nblk slots for every job.
template <typename S, bool HESS>
__global__ __launch_bounds__(256) void ndt_derivative_batch_kernel(const NdtJob* __restrict__ jobs, const int2* __restrict__ wg, double* __restrict__ partials) {
  const int2 w = wg[blockIdx.x];
  const NdtJob& j = jobs[w.x];
  ndt_derivative_block<S, HESS>(j.sx, j.sy, j.sz, j.n, j.vm, j.ev, w.y, partials + (size_t)(j.first + w.y) * 28);
}

// The radius jobs of a round, under the same grid, table and host guarantees: the query launch, then (after the batched search has
// filled every job's CSR) the walk.
__global__ __launch_bounds__(256) void ndt_query_batch_kernel(const NdtJob* __restrict__ jobs, const int2* __restrict__ wg) {
  const int2 w = wg[blockIdx.x];
  const NdtJob& j = jobs[w.x];
  ndt_query_block(j.sx, j.sy, j.sz, j.n, j.ev.T, w.y, j.nb.q);
}

template <typename S, bool HESS>
__global__ __launch_bounds__(256) void ndt_derivative_csr_batch_kernel(const NdtJob* __restrict__ jobs, const int2* __restrict__ wg, double* __restrict__ partials) {
  const int2 w = wg[blockIdx.x];
  const NdtJob& j = jobs[w.x];
  ndt_derivative_csr_block<S, HESS>(j.sx, j.sy, j.sz, j.n, j.vm, j.ev, j.nb, w.y, partials + (size_t)(j.first + w.y) * 28);
}

// score_inc of one (point, leaf) pair, NDT:975-977, in double
__device__ __forceinline__ double ndt_score_pair(const NdtMapView& vm, const NdtEval& ev, int leaf, float qx, float qy, float qz) {
  const double* mean = vm.mean + (size_t)leaf * 3;
  const double* C = vm.icov + (size_t)leaf * 9;
  const double x0 = (double)qx - mean[0], x1 = (double)qy - mean[1], x2 = (double)qz - mean[2];
  const double q = ndt_dot3<double>(x0, x1, x2, ndt_dot3<double>(C[0], C[1], C[2], x0, x1, x2), ndt_dot3<double>(C[3], C[4], C[5], x0, x1, x2),
                                    ndt_dot3<double>(C[6], C[7], C[8], x0, x1, x2));
  return -ev.d1 * exp(-ev.d2 * q / 2) - ev.d3;
}

// one sum of a 256-lane workgroup: wave_sum, then the four waves in a fixed order -> out[0]
__device__ __forceinline__ void ndt_block_sum1(double sum, double* __restrict__ out) {
  sum = wave_sum(sum);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// calculateScore, NDT:935-983: per point sum of score_inc / neighborhood.size().  The work of ONE workgroup of 256 lanes, shared by the
// single and the batched kernel as ndt_derivative_block is: source points [256 block, 256 block + 256) -> out[0], the block's sum
// (wave_sum, then the four waves in a fixed order).
__device__ __forceinline__ void ndt_score_block(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, const NdtMapView& vm,
                                                const NdtEval& ev, int block, double* __restrict__ out) {
  double sum = 0.0;
  const int i = block * 256 + threadIdx.x;
  if (i < n) {
    float qx, qy, qz;
    transform_f(ev.T, sx[i], sy[i], sz[i], qx, qy, qz);
    int c0, c1, c2;
    bool ok = ndt_cell(qx, vm.g.leaf, c0);
    ok = ndt_cell(qy, vm.g.leaf, c1) && ok;
    ok = ndt_cell(qz, vm.g.leaf, c2) && ok;
    if (ok) {
      int nn = 0;
      double s = 0.0;
#pragma unroll 1
      for (int o = 0; o < ev.n_off; ++o) {
        int d0, d1, d2;
        ndt_offset(ev.n_off, o, d0, d1, d2);
        const int leaf = ndt_lookup(vm, c0, c1, c2, d0, d1, d2);
        if (leaf < 0) continue;
        s += ndt_score_pair(vm, ev, leaf, qx, qy, qz);
        ++nn;
      }
      if (nn) sum = s / (double)nn;  // NDT:979
    }
  }
  ndt_block_sum1(sum, out);
}

// ndt_score_block with the neighbours taken from the CSR (NDT:948-949); the divisor is neighborhood.size(), the whole segment
__device__ __forceinline__ void ndt_score_csr_block(int n, const NdtMapView& vm, const NdtEval& ev, const NdtNeighbours& nb, int block, double* __restrict__ out) {
  double sum = 0.0;
  const int i = block * 256 + threadIdx.x;
  if (i < n && nb.offs) {
    const long long b = nb.offs[i], e = nb.offs[i + 1];
    if (e > b) {
      const float4 qt = nb.q[i];
      double s = 0.0;
#pragma unroll 1
      for (long long k = b; k < e; ++k) {
        const int c = nb.idx[k];
        if (c < 0 || c >= nb.nc) continue;
        const int leaf = nb.c2l[c];
        if (leaf < 0 || leaf >= vm.nl) continue;
        s += ndt_score_pair(vm, ev, leaf, qt.x, qt.y, qt.z);
      }
      sum = s / (double)(e - b);  // NDT:979
    }
  }
  ndt_block_sum1(sum, out);
}

// grid: ceil(n / 256), block 256.  One double per block.
__global__ __launch_bounds__(256) void ndt_score_csr_kernel(int n, NdtMapView vm, NdtEval ev, NdtNeighbours nb, double* __restrict__ partials) {
  ndt_score_csr_block(n, vm, ev, nb, (int)blockIdx.x, partials + blockIdx.x);
}

__global__ __launch_bounds__(256) void ndt_score_csr_batch_kernel(const NdtJob* __restrict__ jobs, const int2* __restrict__ wg, double* __restrict__ partials) {
  const int2 w = wg[blockIdx.x];
  const NdtJob& j = jobs[w.x];
  ndt_score_csr_block(j.n, j.vm, j.ev, j.nb, w.y, partials + (size_t)(j.first + w.y));
}

// grid: ceil(n / 256), block 256.  One double per block.
__global__ __launch_bounds__(256) void ndt_score_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, int n, NdtMapView vm, NdtEval ev,
                                                        double* __restrict__ partials) {
  ndt_score_block(sx, sy, sz, n, vm, ev, (int)blockIdx.x, partials + blockIdx.x);
}

// gorio_ndt_calculate_score_batch: the grid and the (job, job-local block) table of ndt_derivative_batch_kernel, under the same host
// guarantees; the partial buffer holds first + nblk doubles for every job.
__global__ __launch_bounds__(256) void ndt_score_batch_kernel(const NdtJob* __restrict__ jobs, const int2* __restrict__ wg, double* __restrict__ partials) {
  const int2 w = wg[blockIdx.x];
  const NdtJob& j = jobs[w.x];
  ndt_score_block(j.sx, j.sy, j.sz, j.n, j.vm, j.ev, w.y, partials + (size_t)(j.first + w.y));
}

// sum over the blocks, in block order, of partials[b * width + k]
__device__ __forceinline__ double ndt_fold_sum(const double* __restrict__ partials, int nblk, int width, int k) {
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partials[(size_t)b * width + k];
  return s;
}

// out[k] = ndt_fold_sum(k); width <= 64.  grid 1, block 64
__global__ __launch_bounds__(64) void ndt_fold_kernel(const double* __restrict__ partials, int nblk, int width, double* __restrict__ out) {
  if ((int)threadIdx.x >= width) return;
  out[threadIdx.x] = ndt_fold_sum(partials, nblk, width, (int)threadIdx.x);
}

// grid: one 64-lane workgroup per job; width <= 64 (28 for the derivative sums, 1 for the score).  out[width job + k] = the job's sums,
// its partials added in block order
__global__ __launch_bounds__(64) void ndt_fold_batch_kernel(const NdtJob* __restrict__ jobs, const double* __restrict__ partials, int width, double* __restrict__ out) {
  if ((int)threadIdx.x >= width) return;
  const NdtJob& j = jobs[blockIdx.x];
  out[(size_t)blockIdx.x * width + threadIdx.x] = ndt_fold_sum(partials + (size_t)j.first * width, j.nblk, width, (int)threadIdx.x);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_ndt.h)
namespace gorio {
// What setInputTarget leaves on the device: the cloud and the voxel map built from it (target_cells_).  Handles hold it through a
// shared_ptr: gorio_ndt_set_target_shared makes two handles look at ONE state, which lives until the last of them lets go.
struct NdtTarget {
  int device = 0;
  DevBuf<float> tx, ty, tz;
  size_t t_cap = 0;
  int n_t = 0;
  bool has_target = false;
  // voxel map: stale after a new target, or (with one holder) a changed resolution / leaf rule; rebuilt by the next call that needs it
  DevBuf<unsigned long long> keys;
  DevBuf<int> counts, bb;
  DevBuf<int> lidx, lcnt;
  DevBuf<double> lmean, lraw, lcov, licov;
  DevBuf<float> lcent;  // [nl][3] the float centroid of every leaf (VGC:242-243, 289)
  size_t l_cap = 0;
  int nl = 0;
  NdtGrid grid{};
  bool map_valid = false;
  // the three parameters the valid map was built with
  double resolution = 0.0, min_covar_eigvalue_mult = 0.0;
  int min_points_per_voxel = 0;
  // radius mode: the centroid cloud (SoA, ascending leaf index), centroid -> leaf position, and the search handle that holds the indexed
  // copy of the cloud.  Part of the map, so sharers see ONE index; built by the first evaluation that needs it, stale with the map.
  DevBuf<float> cx, cy, cz;
  DevBuf<int> c2l;
  size_t c_cap = 0;
  int nc = 0;
  bool cent_valid = false;
  gorio_search_handle* cent = nullptr;
  NdtTarget() = default;
  NdtTarget(const NdtTarget&) = delete;
  NdtTarget& operator=(const NdtTarget&) = delete;
  ~NdtTarget() {
    hipSetDevice(device);
    if (cent) gorio_search_destroy(cent);
  }  // the buffers free themselves as members, after this body: the device has to be current by then
};
}  // namespace gorio

struct gorio_ndt {
  int device = 0;
  hipStream_t stream = nullptr;
  gorio_ndt_params p;
  std::shared_ptr<gorio::NdtTarget> tgt;  // never null; may be shared with other handles of the device
  bool tgt_owned = true;                  // false after gorio_ndt_set_target_shared: the buffers were allocated through another handle
  // source cloud, SoA
  gorio::DevBuf<float> sx, sy, sz;
  size_t s_cap = 0;
  int n_s = 0;
  bool has_source = false;
  gorio::DevBuf<int> flag;
  // staging of a source that comes from the device (ndt_adopt): filled first, swapped with sx, sy, sz only when every point is finite
  gorio::DevBuf<float> ax, ay, az;
  size_t a_cap = 0;
  hipEvent_t adopt_ev = nullptr;  // orders a hand-off's copy behind the producer's stream; made by the first hand-off
  // evaluation scratch
  gorio::DevBuf<double> partials, d_out;
  gorio::PinnedBuf h_out;  // 28 doubles
  // batch scratch (of the handle that leads a gorio_ndt_align_batch): job table + workgroup table, partials, sums
  gorio::DevBuf<void> b_jobs;
  gorio::DevBuf<double> b_partials, b_out;
  gorio::PinnedBuf b_h_jobs, b_h_out;
  // radius mode (gorio_ndt_set_radius_search): the switch, the transformed source of the last evaluation, this handle's search state
  // (scratch and the CSR of its last search; the cloud searched is the target state's) and whether that CSR is still the last evaluation's
  bool radius = false;
  gorio::DevBuf<float4> rq;
  gorio_search_handle* rs = nullptr;
  bool nb_valid = false, nb_empty = false;
  int nb_n = 0;
  gorio::NdtMapView map() const { return gorio::NdtMapView{tgt->lidx, tgt->lcnt, tgt->lmean, tgt->licov, tgt->nl, p.min_points_per_voxel, tgt->grid}; }
};

namespace {
thread_local std::string g_ndt_err;
int ndt_fail(int code, const std::string& m) {
  g_ndt_err = m;
  return code;
}

float ndt_decode(int k) {  // sc_decode on the host
  const int i = k >= 0 ? k : k ^ 0x7fffffff;
  float f;
  std::memcpy(&f, &i, 4);
  return f;
}

// ---- the search half of the radius mode.  The exact radius search lives in apd_search.hip, which is included after this file (its handle
// type is complete only there): these five are defined in apd_ndt_radius.hip, behind it.  `cloud` is the search handle that holds the
// indexed centroid cloud (NdtTarget::cent); `s` a per-handle search state (scratch and the CSR of its last search).
struct NdtCsr {  // device pointers into a search state, valid until its next search
  const long long* offs = nullptr;
  const int* idx = nullptr;
  const float* sqd = nullptr;
  long long total = 0;
};
struct NdtRadiusJob {
  gorio_search_handle* s;
  gorio_search_handle* cloud;
  const float4* q;
  int n;
  double radius;
  NdtCsr csr;  // out
};
gorio_search_handle* ndt_rs_new(int device);
void ndt_rs_free(gorio_search_handle* s);
hipStream_t ndt_rs_stream(gorio_search_handle* cloud);  // the device's launch stream: every radius evaluation runs on it
int ndt_rs_radius(NdtRadiusJob* job);                   // one search_radius_core; errors through ndt_fail
int ndt_rs_radius_batch(NdtRadiusJob* jobs, int count, int* launches, int* syncs);  // one search_radius_batch_core
const std::vector<long long>& ndt_rs_host_offsets(const gorio_search_handle* s);    // host copy of the last CSR's offsets, nq + 1
void ndt_rs_csr(NdtRadiusJob* job);                     // job->csr = the CSR job->s holds

int ndt_n_off(int search) { return search == GORIO_NDT_DIRECT1 ? 1 : search == GORIO_NDT_DIRECT7 ? 7 : 26; }

int ndt_check_params(const gorio_ndt_params& p) {
  if (p.search == GORIO_NDT_KDTREE) return ndt_fail(GORIO_ERR_UNSUPPORTED, "set_params: KDTREE is not a value of params.search; gorio_ndt_set_radius_search(h, 1) selects the radius search over leaf centroids");
  if (p.search != GORIO_NDT_DIRECT26 && p.search != GORIO_NDT_DIRECT7 && p.search != GORIO_NDT_DIRECT1) return ndt_fail(GORIO_ERR_UNSUPPORTED, "set_params: unknown search method");
  if (!(p.resolution > 0) || !std::isfinite(p.resolution)) return ndt_fail(GORIO_ERR_UNSUPPORTED, "set_params: resolution must be finite and > 0");
  if (p.min_points_per_voxel < 1) return ndt_fail(GORIO_ERR_INVALID, "set_params: min_points_per_voxel < 1");
  if (std::isnan(p.step_size) || std::isnan(p.outlier_ratio) || std::isnan(p.transformation_epsilon) || std::isnan(p.min_covar_eigvalue_mult))
    return ndt_fail(GORIO_ERR_INVALID, "set_params: NaN parameter");
  return GORIO_OK;
}

// SoA upload of a strided host cloud into (x, y, z) of one capacity
int ndt_upload(gorio_ndt* h, const float* xyz, int n, int stride_bytes, gorio::DevBuf<float>& x, gorio::DevBuf<float>& y, gorio::DevBuf<float>& z, size_t& cap) {
  std::vector<float> soa;
  try {
    soa.resize((size_t)3 * std::max(n, 1));
  } catch (const std::bad_alloc&) {
    return ndt_fail(GORIO_ERR_ALLOC, "out of host memory for the staging copy of the cloud");
  }
  const size_t st = stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    soa[i] = xyz[st * i];
    soa[(size_t)n + i] = xyz[st * i + 1];
    soa[(size_t)2 * n + i] = xyz[st * i + 2];
  }
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  const size_t need = std::max(n, 1);
  GORIO_HIP_CHECK(ndt_fail, gorio::reserve_group(cap, need, need + need / 8 + 64, x, need + need / 8 + 64, y, need + need / 8 + 64, z, need + need / 8 + 64));
  if (n) {
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(x, soa.data(), sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(y, soa.data() + n, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(z, soa.data() + (size_t)2 * n, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
  }
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));  // soa dies here
  return GORIO_OK;
}

// a target about to be overwritten must not be one other handles still look at (gorio_ndt_set_target_shared): detach first
void ndt_make_private(gorio_ndt* h) {
  if (h->tgt.use_count() > 1 || !h->tgt_owned) {
    h->tgt = std::make_shared<gorio::NdtTarget>();
    h->tgt->device = h->device;
  }
  h->tgt_owned = true;
}

// Every cloud that is already on the device comes in here: x, y, z [n] of the handle's device become the source or the target.  It is
// the whole of gorio_ndt_set_source_device / _set_target_device (producer == nullptr: the caller orders its own writes, as before) and
// the device half of gorio_ndt_set_source_from_scan / _set_target_from_scan / _set_target_from_apd, whose argument and state checks
// come first, in csrc/apd_scan.hip, where the other handle types are complete; there `producer` is the stream the cloud was last
// written on.  Ordering: that producer may still have work in flight (gorio_apd_set_target_device returns without a synchronisation),
// so ONE event is recorded on its stream and this handle's stream waits for it on the device; nothing polls.  The copy is complete
// when the call returns (the synchronisation that brings the flag down), so the producer may overwrite its cloud at once.
// A source goes to the staging buffers and changes places with the held one only when no point is non-finite: a refusal leaves the
// held source as it was.  A target is written in place: non-finite target points are accepted (the map skips them), nothing can refuse.
int ndt_adopt(gorio_ndt* h, const float* x, const float* y, const float* z, int n, hipStream_t producer, bool source, const std::string& what) {
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  const size_t need = std::max(n, 1), grown = need + need / 8 + 64;
  gorio::NdtTarget* t = nullptr;
  h->nb_valid = false;
  if (source) {
    GORIO_HIP_CHECK(ndt_fail, gorio::reserve_group(h->a_cap, need, grown, h->ax, grown, h->ay, grown, h->az, grown));
  } else {
    ndt_make_private(h);
    t = h->tgt.get();
    t->map_valid = false;
    t->has_target = false;
    GORIO_HIP_CHECK(ndt_fail, gorio::reserve_group(t->t_cap, need, grown, t->tx, grown, t->ty, grown, t->tz, grown));
  }
  if (n) {
    GORIO_HIP_CHECK(ndt_fail, h->flag.reserve(1));
    if (producer) {
      if (!h->adopt_ev) GORIO_HIP_CHECK(ndt_fail, hipEventCreateWithFlags(&h->adopt_ev, hipEventDisableTiming));
      GORIO_HIP_CHECK(ndt_fail, hipEventRecord(h->adopt_ev, producer));
      GORIO_HIP_CHECK(ndt_fail, hipStreamWaitEvent(h->stream, h->adopt_ev, 0));
    }
    int flag = 0;
    GORIO_HIP_CHECK(ndt_fail, hipMemsetAsync(h->flag, 0, sizeof(int), h->stream));
    if (source) gorio::ndt_adopt_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(x, y, z, n, h->ax, h->ay, h->az, h->flag);
    else gorio::ndt_adopt_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(x, y, z, n, t->tx, t->ty, t->tz, h->flag);
    GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(&flag, h->flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
    if (source && flag) return ndt_fail(GORIO_ERR_INVALID, what + ": a point is not finite (the reference's cell index of it is undefined)");
  }
  if (source) {
    std::swap(h->sx, h->ax);
    std::swap(h->sy, h->ay);
    std::swap(h->sz, h->az);
    std::swap(h->s_cap, h->a_cap);
    h->n_s = n;
    h->has_source = true;
  } else {
    t->n_t = n;
    t->has_target = true;
  }
  return GORIO_OK;
}

// "" when the handle's three map parameters are those the valid map was built with, else a text that names the first one that differs
std::string ndt_map_mismatch(const gorio_ndt* h) {
  const gorio::NdtTarget& t = *h->tgt;
  if ((float)h->p.resolution != (float)t.resolution) return "resolution " + std::to_string(h->p.resolution) + " differs from the shared map's " + std::to_string(t.resolution);
  if (h->p.min_points_per_voxel != t.min_points_per_voxel)
    return "min_points_per_voxel " + std::to_string(h->p.min_points_per_voxel) + " differs from the shared map's " + std::to_string(t.min_points_per_voxel);
  if (h->p.min_covar_eigvalue_mult != t.min_covar_eigvalue_mult)
    return "min_covar_eigvalue_mult " + std::to_string(h->p.min_covar_eigvalue_mult) + " differs from the shared map's " + std::to_string(t.min_covar_eigvalue_mult);
  return std::string();
}

// init() (NDTH:276-283) -> VoxelGridCovariance::applyFilter (VGC:60-370) when the map is stale.  A valid map built with other parameters
// is rebuilt when this handle is the state's only holder, and refused (GORIO_ERR_INVALID) when other handles look at it too.
int ndt_ensure_map(gorio_ndt* h) {
  using namespace gorio;
  NdtTarget* t = h->tgt.get();
  if (t->map_valid) {
    const std::string bad = ndt_map_mismatch(h);
    if (bad.empty()) return GORIO_OK;
    if (h->tgt.use_count() > 1) return ndt_fail(GORIO_ERR_INVALID, "shared target: " + bad + " (set the owner's value, or give this handle a target of its own)");
    t->map_valid = false;
  }
  if (!t->has_target) return ndt_fail(GORIO_ERR_STATE, "no target set");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  const int n = t->n_t;
  t->nl = 0;
  t->nc = 0;
  t->cent_valid = false;
  h->nb_valid = false;
  t->grid = NdtGrid{};
  t->grid.leaf = (float)h->p.resolution;
  t->grid.inv = 1.0f / t->grid.leaf;
  t->resolution = h->p.resolution;
  t->min_points_per_voxel = h->p.min_points_per_voxel;
  t->min_covar_eigvalue_mult = h->p.min_covar_eigvalue_mult;
  if (n == 0) {
    t->map_valid = true;
    return GORIO_OK;
  }
  GORIO_HIP_CHECK(ndt_fail, t->bb.reserve(8));
  cell_bbox_init_kernel<<<1, 64, 0, h->stream>>>(t->bb);
  ndt_bbox_kernel<<<std::min(256, (n + 255) / 256), 256, 0, h->stream>>>(t->tx, t->ty, t->tz, n, t->bb);
  int bb[8];
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(bb, t->bb, sizeof(int) * 8, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  const int n_fin = bb[6];
  if (n_fin < 0 || n_fin > n) return ndt_fail(GORIO_ERR_STATE, "voxel map: internal error, the finite-point count does not fit the cloud");
  if (n_fin == 0) {
    t->map_valid = true;
    return GORIO_OK;
  }
  NdtGrid g = t->grid;
  double cells_f = 1.0, cells_b = 1.0;
  for (int a = 0; a < 3; ++a) {
    const float lo = ndt_decode(bb[a]), hi = ndt_decode(bb[3 + a]);
    const float d = (hi - lo) * g.inv;  // VGC:75-77
    cells_f *= std::floor((double)d) + 1.0;
    const float fl = std::floor(lo * g.inv), fh = std::floor(hi * g.inv);  // VGC:87-92
    if (!(std::fabs(fl) < (float)kNdtCoordLimit) || !(std::fabs(fh) < (float)kNdtCoordLimit))
      return ndt_fail(GORIO_ERR_UNSUPPORTED, "voxel map: a leaf coordinate of the target does not fit 31 bits");
    g.min_b[a] = (int)fl;
    g.max_b[a] = (int)fh;
    g.div_b[a] = g.max_b[a] - g.min_b[a] + 1;  // VGC:95
    cells_b *= (double)g.div_b[a];
  }
  if (cells_f > 2147483647.0 || cells_b > 2147483647.0)  // VGC:79-84
    return ndt_fail(GORIO_ERR_UNSUPPORTED, "voxel map: leaf size is too small for the target, integer leaf indices would overflow");
  g.mul1 = g.div_b[0];  // VGC:103
  g.mul2 = g.div_b[0] * g.div_b[1];
  const int npow2 = sort_padded_size(n);
  const int nblocks = (n_fin + 255) / 256;
  GORIO_HIP_CHECK(ndt_fail, t->keys.reserve(npow2));
  GORIO_HIP_CHECK(ndt_fail, t->counts.reserve((size_t)(n + 255) / 256 + 1));
  ndt_key_kernel<<<(npow2 + 255) / 256, 256, 0, h->stream>>>(t->tx, t->ty, t->tz, n, npow2, g, t->keys, t->bb);
  enqueue_tiled_sort(h->stream, SortKeys{t->keys, npow2}, 1, npow2);
  cell_count_kernel<31><<<nblocks, 256, 0, h->stream>>>(t->keys, n_fin, t->counts);
  block_scan_kernel<<<1, 1024, 0, h->stream>>>(t->counts, nblocks);
  int nv = 0, flags = 0;
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(&nv, t->counts + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(&flags, t->bb + 7, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  if (flags) return ndt_fail(GORIO_ERR_UNSUPPORTED, "voxel map: a target point falls outside the leaf grid (float leaf arithmetic out of range)");
  if (nv <= 0 || nv > n_fin) return ndt_fail(GORIO_ERR_STATE, "voxel map: internal error, the leaf count does not fit the cloud");
  {
    const size_t cap = (size_t)nv + nv / 8 + 64;
    GORIO_HIP_CHECK(ndt_fail, reserve_group(t->l_cap, nv, cap, t->lidx, cap, t->lcnt, cap, t->lmean, 3 * cap, t->lraw, 9 * cap, t->lcov, 9 * cap, t->licov, 9 * cap, t->lcent, 3 * cap));
  }
  ndt_leaf_kernel<<<nblocks, 256, 0, h->stream>>>(t->keys, t->tx, t->ty, t->tz, n_fin, n, t->counts, h->p.min_points_per_voxel, h->p.min_covar_eigvalue_mult, nv, t->lidx, t->lcnt,
                                                  t->lmean, t->lraw, t->lcov, t->licov, t->lcent);
  GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  t->nl = nv;
  t->grid = g;
  t->map_valid = true;
  return GORIO_OK;
}

// The centroid cloud of the valid map and its search index (VGC:282-326: cloud of leaf centroids + kdtree_.setInputCloud), built once per
// map by the first call that needs them: count, scan, ordered compaction, then the index through the library's one index build.
int ndt_ensure_centroids(gorio_ndt* h) {
  using namespace gorio;
  NdtTarget* t = h->tgt.get();
  if (t->cent_valid) return GORIO_OK;
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  const int nl = t->nl, nblk = (nl + 255) / 256;
  int nc = 0;
  if (nl > 0) {
    GORIO_HIP_CHECK(ndt_fail, t->counts.reserve((size_t)nblk + 1));
    ndt_centroid_count_kernel<<<nblk, 256, 0, h->stream>>>(t->lcnt, nl, t->min_points_per_voxel, t->counts);
    block_scan_kernel<<<1, 1024, 0, h->stream>>>(t->counts, nblk);
    GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(&nc, t->counts + nblk, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
    if (nc < 0 || nc > nl) return ndt_fail(GORIO_ERR_STATE, "centroid cloud: internal error, the count does not fit the leaves");
  }
  if (nc > 0) {
    const size_t cap = (size_t)nc + nc / 8 + 64;
    GORIO_HIP_CHECK(ndt_fail, reserve_group(t->c_cap, nc, cap, t->cx, cap, t->cy, cap, t->cz, cap, t->c2l, cap));
    ndt_centroid_compact_kernel<<<nblk, 256, 0, h->stream>>>(t->lcnt, t->lcent, nl, t->min_points_per_voxel, t->counts, nc, t->cx, t->cy, t->cz, t->c2l);
    GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
    GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));  // the index build below runs on the device's launch stream
  }
  if (!t->cent && gorio_search_create(&t->cent, t->device)) return ndt_fail(GORIO_ERR_NO_DEVICE, std::string("centroid index: ") + gorio_search_last_error());
  if (const int rc = gorio_search_set_cloud_device(t->cent, t->cx, t->cy, t->cz, nc))  // a float sum that overflowed is refused here
    return ndt_fail(rc, std::string("centroid index: ") + gorio_search_last_error());
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(ndt_rs_stream(t->cent)));  // the columns are free again (a rebuild writes them on h->stream)
  t->nc = nc;
  t->cent_valid = true;
  return GORIO_OK;
}

// ---- host arithmetic of the shell (plain C++, this file is built un-fused)

float ndt_sinf(float a) { return (float)std::sin((double)a); }  // the correctly rounded float results, include/gorio_ndt.h
float ndt_cosf(float a) { return (float)std::cos((double)a); }
float ndt_atan2f(float a, float b) { return (float)std::atan2((double)a, (double)b); }

// AngleAxis<float>(angle, unit axis).toRotationMatrix(), Eigen 3.3.7
void ndt_angle_axis(float angle, int axis, float R[9]) {
  float a[3] = {0, 0, 0};
  a[axis] = 1.0f;
  const float s = ndt_sinf(angle), c = ndt_cosf(angle);
  const float sa[3] = {s * a[0], s * a[1], s * a[2]};
  const float c1[3] = {(1.0f - c) * a[0], (1.0f - c) * a[1], (1.0f - c) * a[2]};
  float t = c1[0] * a[1];
  R[1] = t - sa[2]; R[3] = t + sa[2];
  t = c1[0] * a[2];
  R[2] = t + sa[1]; R[6] = t - sa[1];
  t = c1[1] * a[2];
  R[5] = t - sa[0]; R[7] = t + sa[0];
  for (int k = 0; k < 3; ++k) R[4 * k] = c1[k] * a[k] + c;
}
void ndt_mul3f(const float* A, const float* B, float* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float v = A[3 * i] * B[j];
      v = v + A[3 * i + 1] * B[3 + j];
      v = v + A[3 * i + 2] * B[6 + j];
      C[3 * i + j] = v;
    }
}
// Translation * AngleAxis(X) * AngleAxis(Y) * AngleAxis(Z) in float, NDT:827-830; T row-major 4 x 4
void ndt_pose_matrix(const double* p, float* T) {
  float Rx[9], Ry[9], Rz[9], A[9], R[9];
  ndt_angle_axis((float)p[3], 0, Rx);
  ndt_angle_axis((float)p[4], 1, Ry);
  ndt_angle_axis((float)p[5], 2, Rz);
  ndt_mul3f(Rx, Ry, A);
  ndt_mul3f(A, Rz, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[4 * r + c] = R[3 * r + c];
    T[4 * r + 3] = (float)p[r];
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}
// eulerAngles(0, 1, 2) of the float rotation, Eigen 3.3.7 EulerAngles.h (NDT:109)
void ndt_euler012(const float* T, float* out) {
  auto R = [&](int r, int c) { return T[4 * r + c]; };
  float r0 = ndt_atan2f(R(1, 2), R(2, 2)), r1;
  const float c2 = std::sqrt(R(0, 0) * R(0, 0) + R(0, 1) * R(0, 1));
  if (r0 > 0.0f) {
    r0 = r0 - (float)M_PI;
    r1 = ndt_atan2f(-R(0, 2), -c2);
  } else {
    r1 = ndt_atan2f(-R(0, 2), c2);
  }
  const float s1 = ndt_sinf(r0), c1 = ndt_cosf(r0);
  const float r2 = ndt_atan2f(s1 * R(2, 0) - c1 * R(1, 0), c1 * R(1, 1) - s1 * R(2, 1));
  out[0] = -r0; out[1] = -r1; out[2] = -r2;
}

// computeAngleDerivatives, NDT:288-395, in double (the kernel rounds to float where the reference does)
void ndt_angle_tables(const double* p, double* ja, double* ha) {
  double cx, cy, cz, sx, sy, sz;
  if (std::fabs(p[3]) < 10e-5) { cx = 1.0; sx = 0.0; } else { cx = std::cos(p[3]); sx = std::sin(p[3]); }
  if (std::fabs(p[4]) < 10e-5) { cy = 1.0; sy = 0.0; } else { cy = std::cos(p[4]); sy = std::sin(p[4]); }
  if (std::fabs(p[5]) < 10e-5) { cz = 1.0; sz = 0.0; } else { cz = std::cos(p[5]); sz = std::sin(p[5]); }
  const double j[24] = {(-sx * sz + cx * sy * cz), (-sx * cz - cx * sy * sz), (-cx * cy),
                        (cx * sz + sx * sy * cz), (cx * cz - sx * sy * sz), (-sx * cy),
                        (-sy * cz), sy * sz, cy,
                        sx * cy * cz, (-sx * cy * sz), sx * sy,
                        (-cx * cy * cz), cx * cy * sz, (-cx * sy),
                        (-cy * sz), (-cy * cz), 0,
                        (cx * cz - sx * sy * sz), (-cx * sz - sx * sy * cz), 0,
                        (sx * cz + cx * sy * sz), (cx * sy * cz - sx * sz), 0};
  const double hh[45] = {(-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), sx * cy,
                         (-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), (-cx * cy),
                         (cx * cy * cz), (-cx * cy * sz), (cx * sy),
                         (sx * cy * cz), (-sx * cy * sz), (sx * sy),
                         (-sx * cz - cx * sy * sz), (sx * sz - cx * sy * cz), 0,
                         (cx * cz - sx * sy * sz), (-sx * sy * cz - cx * sz), 0,
                         (-cy * cz), (cy * sz), (-sy),
                         (-sx * sy * cz), (sx * sy * sz), (sx * cy),
                         (cx * sy * cz), (-cx * sy * sz), (-cx * cy),
                         (sy * sz), (sy * cz), 0,
                         (-sx * cy * sz), (-sx * cy * cz), 0,
                         (cx * cy * sz), (cx * cy * cz), 0,
                         (-cy * cz), (cy * sz), 0,
                         (-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), 0,
                         (-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), 0};
  std::copy(j, j + 24, ja);
  std::copy(hh, hh + 45, ha);
}

gorio::NdtEval ndt_make_eval(const gorio_ndt* h, const double* p, const float* T) {
  gorio::NdtEval ev{};
  for (int q = 0; q < 12; ++q) ev.T[q] = T[q];
  if (p) ndt_angle_tables(p, ev.ja, ev.ha);
  // NDT:89-93; resolution_ is a float member
  const double res = (double)(float)h->p.resolution;
  const double c1 = 10 * (1 - h->p.outlier_ratio), c2 = h->p.outlier_ratio / std::pow(res, 3);
  ev.d3 = -std::log(c2);
  ev.d1 = -std::log(c1 + c2) - ev.d3;
  ev.d2 = -2 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - ev.d3) / ev.d1);
  ev.n_off = ndt_n_off(h->p.search);
  return ev;
}

double ndt_radius_of(const gorio_ndt* h) { return (double)(float)h->p.resolution; }  // resolution_, the float member (NDT:234)

// what a radius evaluation needs beside the map: the centroid index, this handle's search state and its query buffer
int ndt_radius_prepare(gorio_ndt* h) {
  if (const int rc = ndt_ensure_centroids(h)) return rc;
  if (!h->rs && !(h->rs = ndt_rs_new(h->device))) return ndt_fail(GORIO_ERR_ALLOC, "radius search: out of memory");
  const size_t n = (size_t)h->n_s;
  GORIO_HIP_CHECK(ndt_fail, h->rq.reserve(n, n + n / 8 + 64));
  return GORIO_OK;
}

// ndt_evaluate for a handle with the radius switch on: query launch, radius search, walk, fold -- all on the device's launch stream, where
// the search runs.  (Uploads and map builds end with a synchronisation of the handle's own stream, so nothing is in flight there.)
int ndt_evaluate_radius(gorio_ndt* h, const gorio::NdtEval& ev, int mode, double* out) {
  using namespace gorio;
  const int n = h->n_s, nblk = (n + 255) / 256;
  const int width = mode == 3 ? 1 : 28;
  if (const int rc = ndt_radius_prepare(h)) return rc;
  NdtTarget* t = h->tgt.get();
  hipStream_t stream = ndt_rs_stream(t->cent);
  GORIO_HIP_CHECK(ndt_fail, h->partials.reserve((size_t)28 * nblk, (size_t)28 * (nblk + nblk / 8 + 4)));
  GORIO_HIP_CHECK(ndt_fail, h->d_out.reserve(28));
  if (!h->h_out.get()) GORIO_HIP_CHECK(ndt_fail, h->h_out.realloc(sizeof(double) * 28));
  h->nb_valid = false;
  NdtNeighbours nb{h->rq, nullptr, nullptr, t->c2l, t->nc};
  if (t->nc > 0) {
    ndt_query_kernel<<<nblk, 256, 0, stream>>>(h->sx, h->sy, h->sz, n, ev, h->rq);
    GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
    NdtRadiusJob job{h->rs, t->cent, h->rq, n, ndt_radius_of(h), NdtCsr{}};
    if (const int rc = ndt_rs_radius(&job)) return rc;
    nb.offs = job.csr.offs;
    nb.idx = job.csr.idx;
  }
  const NdtMapView vm = h->map();
  if (mode == 0) ndt_derivative_csr_kernel<float, false><<<nblk, 256, 0, stream>>>(h->sx, h->sy, h->sz, n, vm, ev, nb, h->partials);
  else if (mode == 1) ndt_derivative_csr_kernel<float, true><<<nblk, 256, 0, stream>>>(h->sx, h->sy, h->sz, n, vm, ev, nb, h->partials);
  else if (mode == 2) ndt_derivative_csr_kernel<double, true><<<nblk, 256, 0, stream>>>(h->sx, h->sy, h->sz, n, vm, ev, nb, h->partials);
  else ndt_score_csr_kernel<<<nblk, 256, 0, stream>>>(n, vm, ev, nb, h->partials);
  ndt_fold_kernel<<<1, 64, 0, stream>>>(h->partials, nblk, width, h->d_out);
  GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(h->h_out.get(), h->d_out, sizeof(double) * width, hipMemcpyDeviceToHost, stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(stream));
  std::memcpy(out, h->h_out.get(), sizeof(double) * width);
  h->nb_valid = true;
  h->nb_empty = t->nc == 0;
  h->nb_n = n;
  return GORIO_OK;
}

// one evaluation: mode 0 computeDerivatives without the Hessian, 1 with it, 2 computeHessian, 3 calculateScore.  out: 28 doubles
int ndt_evaluate(gorio_ndt* h, const gorio::NdtEval& ev, int mode, double* out) {
  using namespace gorio;
  if (h->radius) return ndt_evaluate_radius(h, ev, mode, out);
  const int n = h->n_s, nblk = (n + 255) / 256;
  const int width = mode == 3 ? 1 : 28;
  GORIO_HIP_CHECK(ndt_fail, h->partials.reserve((size_t)28 * nblk, (size_t)28 * (nblk + nblk / 8 + 4)));
  GORIO_HIP_CHECK(ndt_fail, h->d_out.reserve(28));
  if (!h->h_out.get()) GORIO_HIP_CHECK(ndt_fail, h->h_out.realloc(sizeof(double) * 28));
  const NdtMapView vm = h->map();
  if (mode == 0) ndt_derivative_kernel<float, false><<<nblk, 256, 0, h->stream>>>(h->sx, h->sy, h->sz, n, vm, ev, h->partials);
  else if (mode == 1) ndt_derivative_kernel<float, true><<<nblk, 256, 0, h->stream>>>(h->sx, h->sy, h->sz, n, vm, ev, h->partials);
  else if (mode == 2) ndt_derivative_kernel<double, true><<<nblk, 256, 0, h->stream>>>(h->sx, h->sy, h->sz, n, vm, ev, h->partials);
  else ndt_score_kernel<<<nblk, 256, 0, h->stream>>>(h->sx, h->sy, h->sz, n, vm, ev, h->partials);
  ndt_fold_kernel<<<1, 64, 0, h->stream>>>(h->partials, nblk, width, h->d_out);
  GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(h->h_out.get(), h->d_out, sizeof(double) * width, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  std::memcpy(out, h->h_out.get(), sizeof(double) * width);
  return GORIO_OK;
}

void ndt_unpack_hessian(const double* acc, double* H) {  // upper triangle, mirrored
  int t = 7;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++t) H[6 * i + j] = H[6 * j + i] = acc[t];
}

// what a call that evaluates needs, without building anything: GORIO_OK or the refusal
int ndt_check_ready(const gorio_ndt* h, const std::string& what) {
  if (!h->tgt->has_target) return ndt_fail(GORIO_ERR_STATE, what + ": no target set");
  if (!h->has_source || h->n_s == 0) return ndt_fail(GORIO_ERR_STATE, what + ": no source set (or an empty one)");
  return GORIO_OK;
}

int ndt_ready(gorio_ndt* h, const std::string& what) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, what + ": null handle");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));  // the evaluation scratch below is allocated on the handle's device, whatever the caller left current
  if (const int rc = ndt_check_ready(h, what)) return rc;
  if (const int rc = ndt_ensure_map(h)) return ndt_fail(rc, what + ": " + g_ndt_err);
  if (h->tgt->nl == 0) return ndt_fail(GORIO_ERR_STATE, what + ": the target has no finite point");
  return GORIO_OK;
}

// JacobiSVD<6x6 double>(H).solve(b) for the symmetric H: cyclic Jacobi H = V L V^T, x = V L^+ V^T b, |L| <= 6 eps max|L| -> 0
void ndt_svd_solve(const double* Hin, const double* b, double* x) {
  double A[36], V[36];
  for (int i = 0; i < 36; ++i) {
    A[i] = Hin[i];
    V[i] = (i % 7 == 0) ? 1.0 : 0.0;
  }
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0;
    for (int i = 0; i < 6; ++i)
      for (int j = i + 1; j < 6; ++j) off += A[6 * i + j] * A[6 * i + j];
    if (off == 0.0) break;
    for (int pp = 0; pp < 6; ++pp)
      for (int q = pp + 1; q < 6; ++q) {
        const double apq = A[6 * pp + q];
        if (apq == 0.0) continue;
        const double g = 100.0 * std::fabs(apq);
        if (sweep > 3 && std::fabs(A[7 * pp]) + g == std::fabs(A[7 * pp]) && std::fabs(A[7 * q]) + g == std::fabs(A[7 * q])) {
          A[6 * pp + q] = A[6 * q + pp] = 0.0;
          continue;
        }
        const double theta = (A[7 * q] - A[7 * pp]) / (2.0 * apq);
        double t = 1.0 / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {  // A <- A J
          const double akp = A[6 * k + pp], akq = A[6 * k + q];
          A[6 * k + pp] = c * akp - s * akq;
          A[6 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {  // A <- J^T A
          const double apk = A[6 * pp + k], aqk = A[6 * q + k];
          A[6 * pp + k] = c * apk - s * aqk;
          A[6 * q + k] = s * apk + c * aqk;
        }
        A[6 * pp + q] = A[6 * q + pp] = 0.0;
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[6 * k + pp], vkq = V[6 * k + q];
          V[6 * k + pp] = c * vkp - s * vkq;
          V[6 * k + q] = s * vkp + c * vkq;
        }
      }
  }
  double smax = 0.0;
  for (int i = 0; i < 6; ++i) smax = std::max(smax, std::fabs(A[7 * i]));
  const double thr = 6 * 2.220446049250313e-16 * smax;
  for (int i = 0; i < 6; ++i) x[i] = 0.0;
  for (int k = 0; k < 6; ++k) {
    if (!(std::fabs(A[7 * k]) > thr)) continue;
    double y = 0.0;
    for (int i = 0; i < 6; ++i) y += V[6 * i + k] * b[i];
    y /= A[7 * k];
    for (int i = 0; i < 6; ++i) x[i] += V[6 * i + k] * y;
  }
}

// trialValueSelectionMT, NDT:689-769
double ndt_trial_value(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    if (std::fabs(a_c - a_l) < std::fabs(a_q - a_l)) return a_c;
    return 0.5 * (a_q + a_c);
  } else if (g_t * g_l < 0) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    if (std::fabs(a_c - a_t) >= std::fabs(a_s - a_t)) return a_c;
    return a_s;
  } else if (std::fabs(g_t) <= std::fabs(g_l)) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = std::sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double a_t_next = std::fabs(a_c - a_t) < std::fabs(a_s - a_t) ? a_c : a_s;
    if (a_t > a_l) return std::min(a_t + 0.66 * (a_u - a_t), a_t_next);
    return std::max(a_t + 0.66 * (a_u - a_t), a_t_next);
  }
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = std::sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

// updateIntervalMT, NDT:648-686
bool ndt_update_interval(double& a_l, double& f_l, double& g_l, double& a_u, double& f_u, double& g_u, double a_t, double f_t, double g_t) {
  if (f_t > f_l) {
    a_u = a_t; f_u = f_t; g_u = g_t;
    return false;
  } else if (g_t * (a_l - a_t) > 0) {
    a_l = a_t; f_l = f_t; g_l = g_t;
    return false;
  } else if (g_t * (a_l - a_t) < 0) {
    a_u = a_l; f_u = f_l; g_u = g_l;
    a_l = a_t; f_l = f_t; g_l = g_t;
    return false;
  }
  return true;
}

struct NdtState {  // what computeTransformation carries between the calls
  double score = 0.0, g[6], H[36];
  float T[16];
  gorio_ndt_diag diag{};
};

// the 28 sums of a computeDerivatives evaluation -> score, gradient and (asked for) Hessian
void ndt_take_derivs(NdtState& st, const double* acc, bool hessian) {
  st.score = acc[0];
  for (int k = 0; k < 6; ++k) st.g[k] = acc[1 + k];
  if (hessian) ndt_unpack_hessian(acc, st.H);
  st.diag.n_derivatives++;
}

int ndt_derivs_at(gorio_ndt* h, NdtState& st, const double* p, const float* T, bool hessian) {
  double acc[28];
  const gorio::NdtEval ev = ndt_make_eval(h, p, T);
  if (const int rc = ndt_evaluate(h, ev, hessian ? 1 : 0, acc)) return rc;
  ndt_take_derivs(st, acc, hessian);
  return GORIO_OK;
}

// computeTransformation (NDT:81-171) with computeStepLengthMT (NDT:772-932) inside, as a resumable machine: it stops wherever the
// reference evaluates the derivative sums ("I need evaluation `mode` at pose `x_eval` / matrix st.T") and goes on when it is handed
// the 28 sums.  gorio_ndt_align feeds one machine through ndt_evaluate; gorio_ndt_align_batch feeds many, one evaluation per round.
struct NdtMachine {
  enum Phase { kFirst, kStepFirst, kStepInner, kStepHessian, kDone };
  const gorio_ndt* h = nullptr;
  NdtState st;
  Phase phase = kDone;
  int mode = 1;        // of the pending evaluation: 0 computeDerivatives without the Hessian, 1 with it, 2 computeHessian
  double x_eval[6];    // pose vector of the pending evaluation (its float matrix is st.T)
  // computeTransformation's locals
  double p[6], delta[6], delta_p_norm = 0.0, prob = 0.0;
  int nr = 0;
  bool conv = false;
  // computeStepLengthMT's locals
  double phi_0, d_phi_0, a_l, a_u, f_l, g_l, f_u, g_u, a_t, step_max, step_min, phi_t, d_phi_t, psi_t, d_psi_t;
  bool interval_converged, open_interval;
  int step_iterations;

  static constexpr double mu = 1.e-4, nu = 0.9;
  static constexpr int max_step_iterations = 10;

  bool done() const { return phase == kDone; }

  void begin(const gorio_ndt* handle, const float* guess) {
    h = handle;
    for (int i = 0; i < 16; ++i) st.T[i] = guess ? guess[i] : ((i % 5 == 0) ? 1.0f : 0.0f);  // NDT:95-104: final_transformation_ = guess
    float ang[3];
    ndt_euler012(st.T, ang);
    const double p0[6] = {(double)st.T[3], (double)st.T[7], (double)st.T[11], (double)ang[0], (double)ang[1], (double)ang[2]};  // NDT:107-111
    std::copy(p0, p0 + 6, p);
    std::copy(p0, p0 + 6, x_eval);
    mode = 1;  // NDT:119: the cloud moved by the guess itself
    phase = kFirst;
  }

  // the 28 sums of the pending evaluation arrive; afterwards another evaluation is pending, or the machine is done
  void resume(const double* acc) {
    switch (phase) {
      case kFirst:
        ndt_take_derivs(st, acc, true);
        newton();
        break;
      case kStepFirst:  // NDT:837
        ndt_take_derivs(st, acc, true);
        phi_t = -st.score;
        d_phi_t = -dir_dot();
        psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t;
        d_psi_t = d_phi_t - mu * d_phi_0;
        step_loop();
        break;
      case kStepInner:  // NDT:881
        ndt_take_derivs(st, acc, false);
        phi_t = -st.score;
        d_phi_t = -dir_dot();
        psi_t = phi_t - phi_0 - mu * d_phi_0 * a_t;
        d_psi_t = d_phi_t - mu * d_phi_0;
        if (open_interval && (psi_t <= 0 && d_psi_t >= 0)) {
          open_interval = false;
          f_l = f_l + phi_0 - mu * d_phi_0 * a_l;
          g_l = g_l + mu * d_phi_0;
          f_u = f_u + phi_0 - mu * d_phi_0 * a_u;
          g_u = g_u + mu * d_phi_0;
        }
        if (open_interval) interval_converged = ndt_update_interval(a_l, f_l, g_l, a_u, f_u, g_u, a_t, psi_t, d_psi_t);
        else interval_converged = ndt_update_interval(a_l, f_l, g_l, a_u, f_u, g_u, a_t, phi_t, d_phi_t);
        step_iterations++;
        step_loop();
        break;
      case kStepHessian:  // NDT:928-929
        ndt_unpack_hessian(acc, st.H);
        st.diag.n_hessians++;
        step_end();
        break;
      case kDone:
        break;
    }
  }

  void results(float* T_out, int* converged, int* nr_iterations, double* trans_probability, gorio_ndt_diag* diag) const {
    std::copy(st.T, st.T + 16, T_out);
    if (converged) *converged = conv ? 1 : 0;
    if (nr_iterations) *nr_iterations = nr;
    if (trans_probability) *trans_probability = prob;
    if (diag) {
      *diag = st.diag;
      diag->score = st.score;
    }
  }

 private:
  double dir_dot() const {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += st.g[k] * delta[k];
    return s;
  }
  void ask(int m, Phase ph) {
    mode = m;
    phase = ph;
  }
  void trial_pose() {  // NDT:825-830
    for (int k = 0; k < 6; ++k) x_eval[k] = p[k] + delta[k] * a_t;
    ndt_pose_matrix(x_eval, st.T);
  }

  // the body of NDT:122-168 up to the line search's first evaluation; loops while a step needs no evaluation at all
  void newton() {
    const double n_src = (double)h->n_s;
    while (!conv) {
      double mg[6];
      for (int k = 0; k < 6; ++k) mg[k] = -st.g[k];
      ndt_svd_solve(st.H, mg, delta);  // NDT:127-129
      double nn = 0.0;
      for (int k = 0; k < 6; ++k) nn += delta[k] * delta[k];
      delta_p_norm = std::sqrt(nn);
      if (delta_p_norm == 0 || delta_p_norm != delta_p_norm) {  // NDT:134-139
        prob = st.score / n_src;
        conv = delta_p_norm == delta_p_norm;
        phase = kDone;
        return;
      }
      for (int k = 0; k < 6; ++k) delta[k] /= delta_p_norm;
      if (step_begin(delta_p_norm, h->p.step_size, h->p.transformation_epsilon / 2)) return;  // an evaluation is pending
      step_taken(0.0);  // NDT:787-789: no descent along the direction, a step of length 0
    }
    prob = st.score / n_src;  // NDT:170
    phase = kDone;
  }

  // computeStepLengthMT up to NDT:837; false when it returns 0 without an evaluation (d_phi_0 == 0)
  bool step_begin(double step_init, double smax, double smin) {
    step_max = smax;
    step_min = smin;
    phi_0 = -st.score;
    d_phi_0 = 0.0;
    for (int k = 0; k < 6; ++k) d_phi_0 += st.g[k] * delta[k];
    d_phi_0 = -d_phi_0;
    if (d_phi_0 >= 0) {
      if (d_phi_0 == 0) return false;
      d_phi_0 *= -1;
      for (int k = 0; k < 6; ++k) delta[k] *= -1;
    }
    step_iterations = 0;
    a_l = 0;
    a_u = 0;
    f_l = phi_0 - phi_0 - mu * d_phi_0 * a_l;  // auxiliaryFunction_PsiMT / _dPsiMT, NDTH:433, 446
    g_l = d_phi_0 - mu * d_phi_0;
    f_u = phi_0 - phi_0 - mu * d_phi_0 * a_u;
    g_u = d_phi_0 - mu * d_phi_0;
    interval_converged = (step_max - step_min) < 0;
    open_interval = true;
    a_t = step_init;
    a_t = std::min(a_t, step_max);
    a_t = std::max(a_t, step_min);
    trial_pose();
    ask(1, kStepFirst);
    return true;
  }

  // the head of the loop NDT:850: another trial step, or the end of the search
  void step_loop() {
    if (!interval_converged && step_iterations < max_step_iterations && !(psi_t <= 0 && d_phi_t <= -nu * d_phi_0)) {
      if (open_interval) a_t = ndt_trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, psi_t, d_psi_t);
      else a_t = ndt_trial_value(a_l, f_l, g_l, a_u, f_u, g_u, a_t, phi_t, d_phi_t);
      a_t = std::min(a_t, step_max);
      a_t = std::max(a_t, step_min);
      trial_pose();
      ask(0, kStepInner);
      return;
    }
    if (step_iterations) {  // NDT:928-929: x_eval and st.T are those of the last trial
      ask(2, kStepHessian);
      return;
    }
    step_end();
  }

  void step_end() {
    st.diag.n_mt_iterations += step_iterations;
    step_taken(a_t);
    newton();
  }

  // NDT:150-166
  void step_taken(double a) {
    delta_p_norm = a;
    for (int k = 0; k < 6; ++k) {
      delta[k] *= delta_p_norm;
      p[k] = p[k] + delta[k];
    }
    if (nr > h->p.max_iterations || (nr && (std::fabs(delta_p_norm) < h->p.transformation_epsilon))) conv = true;  // NDT:158-162
    nr++;
  }
};

// What gorio_ndt_align_batch and gorio_ndt_calculate_score_batch ask of their handles before anything is built, allocated or launched;
// `name` is the entry's name in the text.
int ndt_batch_check(gorio_ndt* const* handles, int count, const std::string& name) {
  auto who = [&](int i) { return name + ": handle " + std::to_string(i); };
  for (int i = 0; i < count; ++i) {
    if (!handles[i]) return ndt_fail(GORIO_ERR_INVALID, who(i) + ": null handle");
    if (handles[i]->device != handles[0]->device) return ndt_fail(GORIO_ERR_INVALID, who(i) + ": on another device than handle 0");
  }
  {
    std::vector<const gorio_ndt*> sorted(handles, handles + count);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
      for (int i = 0; i < count; ++i)
        for (int k = 0; k < i; ++k)
          if (handles[i] == handles[k]) return ndt_fail(GORIO_ERR_INVALID, who(i) + ": the same handle as handle " + std::to_string(k));
    }
  }
  for (int i = 0; i < count; ++i) {
    const gorio_ndt* h = handles[i];
    if (const int rc = ndt_check_ready(h, who(i))) return rc;
    if (h->tgt->map_valid && h->tgt.use_count() > 1) {
      const std::string bad = ndt_map_mismatch(h);
      if (!bad.empty()) return ndt_fail(GORIO_ERR_INVALID, who(i) + ": shared target: " + bad);
    }
  }
  return GORIO_OK;
}

// stale maps, once per target state (each build ends with a synchronisation of the building handle's stream)
int ndt_batch_maps(gorio_ndt* const* handles, int count, const std::string& name) {
  for (int i = 0; i < count; ++i) {
    const std::string who = name + ": handle " + std::to_string(i);
    if (const int rc = ndt_ensure_map(handles[i])) return ndt_fail(rc, who + ": " + g_ndt_err);
    if (handles[i]->tgt->nl == 0) return ndt_fail(GORIO_ERR_STATE, who + ": the target has no finite point");
  }
  return GORIO_OK;
}

// the derivative launch of one evaluation mode, over DIRECT jobs or over radius jobs (whose CSR the round's search has filled)
template <typename... A>
void ndt_launch_batch(int mode, bool radius, int blocks, hipStream_t stream, A... a) {
  using namespace gorio;
  if (radius) {
    if (mode == 0) ndt_derivative_csr_batch_kernel<float, false><<<blocks, 256, 0, stream>>>(a...);
    else if (mode == 1) ndt_derivative_csr_batch_kernel<float, true><<<blocks, 256, 0, stream>>>(a...);
    else ndt_derivative_csr_batch_kernel<double, true><<<blocks, 256, 0, stream>>>(a...);
  } else {
    if (mode == 0) ndt_derivative_batch_kernel<float, false><<<blocks, 256, 0, stream>>>(a...);
    else if (mode == 1) ndt_derivative_batch_kernel<float, true><<<blocks, 256, 0, stream>>>(a...);
    else ndt_derivative_batch_kernel<double, true><<<blocks, 256, 0, stream>>>(a...);
  }
}

// what a batch prepares per radius handle before its rounds: centroid index, search state, query buffer
int ndt_batch_radius_prepare(gorio_ndt* const* handles, int count, const std::string& name) {
  for (int i = 0; i < count; ++i)
    if (handles[i]->radius)
      if (const int rc = ndt_radius_prepare(handles[i])) return ndt_fail(rc, name + ": handle " + std::to_string(i) + ": " + g_ndt_err);
  return GORIO_OK;
}

// The stream the launches of a batch run on: handles[0]'s own while every handle is DIRECT; the device's launch stream, where the search
// runs, as soon as one handle has the radius switch on.
hipStream_t ndt_batch_stream(gorio_ndt* const* handles, int count) {
  for (int i = 0; i < count; ++i)
    if (handles[i]->radius) return ndt_rs_stream(handles[i]->tgt->cent);
  return handles[0]->stream;
}

// job record of one pending evaluation; the partial slots [first, first + nblk) are its own
void ndt_fill_job(gorio::NdtJob& j, gorio_ndt* h, int mode, int first, const gorio::NdtEval& ev) {
  j.sx = h->sx; j.sy = h->sy; j.sz = h->sz;
  j.n = h->n_s;
  j.mode = mode;
  j.first = first;
  j.nblk = (h->n_s + 255) / 256;
  j.vm = h->map();
  j.ev = ev;
  j.nb = gorio::NdtNeighbours{nullptr, nullptr, nullptr, nullptr, 0};
  if (h->radius) {
    j.nb = gorio::NdtNeighbours{h->rq, nullptr, nullptr, h->tgt->c2l, h->tgt->nc};
    h->nb_valid = false;
  }
}

// The neighbours of a round's radius jobs rk (indices into the job table; job k belongs to handles[order[k]]): ONE query launch over their
// (job, block) entries d_wg[0 .. blocks), ONE search_radius_batch_core over those whose map has a centroid, then the job records go up
// once more with the CSR every search state now holds.  The table is already on its way to the device when this is called.
int ndt_batch_neighbours(gorio_ndt* const* handles, const std::vector<int>& order, const std::vector<int>& rk, gorio::NdtJob* h_jobs, gorio::NdtJob* d_jobs, const int2* d_wg, int blocks,
                         hipStream_t stream, std::vector<NdtRadiusJob>& rjobs, int* launches) {
  using namespace gorio;
  rjobs.clear();
  std::vector<int> searched;
  for (const int k : rk) {
    gorio_ndt* h = handles[order[k]];
    if (h->tgt->nc == 0) continue;  // no centroid: the job keeps offs == nullptr, no point has a neighbour
    rjobs.push_back(NdtRadiusJob{h->rs, h->tgt->cent, h->rq, h->n_s, ndt_radius_of(h), NdtCsr{}});
    searched.push_back(k);
  }
  if (rjobs.empty()) return GORIO_OK;
  ndt_query_batch_kernel<<<blocks, 256, 0, stream>>>(d_jobs, d_wg);
  GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
  int search_launches = 0, syncs = 0;
  if (const int rc = ndt_rs_radius_batch(rjobs.data(), (int)rjobs.size(), &search_launches, &syncs)) return rc;
  if (syncs == 0) GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(stream));  // the pinned table is read by the first copy until then
  int lo = INT_MAX, hi = -1;
  for (size_t r = 0; r < searched.size(); ++r) {
    NdtJob& j = h_jobs[searched[r]];
    j.nb.offs = rjobs[r].csr.offs;
    j.nb.idx = rjobs[r].csr.idx;
    lo = std::min(lo, searched[r]);
    hi = std::max(hi, searched[r]);
  }
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(d_jobs + lo, h_jobs + lo, sizeof(NdtJob) * (size_t)(hi - lo + 1), hipMemcpyHostToDevice, stream));
  *launches += 1 + search_launches;
  return GORIO_OK;
}

// after the round's synchronisation: every radius job's CSR is the last evaluation of its handle
void ndt_batch_neighbours_done(gorio_ndt* const* handles, const std::vector<int>& order, const std::vector<int>& rk) {
  for (const int k : rk) {
    gorio_ndt* h = handles[order[k]];
    h->nb_valid = true;
    h->nb_empty = h->tgt->nc == 0;
    h->nb_n = h->n_s;
  }
}
}  // namespace

extern "C" {

const char* gorio_ndt_last_error(void) { return g_ndt_err.c_str(); }

void gorio_ndt_default_params(gorio_ndt_params* p) {  // NDT:47-76, VoxelGridCovariance's constructor
  if (!p) return;
  p->resolution = 1.0;
  p->step_size = 0.1;
  p->outlier_ratio = 0.55;
  p->transformation_epsilon = 0.1;
  p->max_iterations = 35;
  p->search = GORIO_NDT_DIRECT7;
  p->min_points_per_voxel = 6;
  p->min_covar_eigvalue_mult = 0.01;
}

int gorio_ndt_create(gorio_ndt_t** out, int device) {  // NDT:47-76
  if (!out) return ndt_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ndt_fail(GORIO_ERR_NO_DEVICE, "create: no usable HIP device (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return ndt_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(device));
  gorio_ndt* h = new (std::nothrow) gorio_ndt();
  if (!h) return ndt_fail(GORIO_ERR_ALLOC, "create: out of memory");
  h->device = device;
  h->tgt = std::make_shared<gorio::NdtTarget>();
  h->tgt->device = device;
  gorio_ndt_default_params(&h->p);
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return ndt_fail(GORIO_ERR_NO_DEVICE, "create: no stream");
  }
  *out = h;
  return GORIO_OK;
}

void gorio_ndt_destroy(gorio_ndt_t* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) {
    hipStreamSynchronize(h->stream);
    hipStreamDestroy(h->stream);
  }
  if (h->adopt_ev) hipEventDestroy(h->adopt_ev);
  if (h->rs) ndt_rs_free(h->rs);
  delete h;
}

// setResolution / setStepSize / setOutlierRatio / setNeighborhoodSearchMethod / setTransformationEpsilon / setMaximumIterations, NDTH:115-191
int gorio_ndt_set_params(gorio_ndt_t* h, const gorio_ndt_params* p) {
  if (!p) return ndt_fail(GORIO_ERR_INVALID, "set_params: null argument");
  if (const int rc = ndt_check_params(*p)) return rc;  // before the handle: a refused value needs no device
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_params: null handle");
  // NDTH:136-141.  A map other handles look at too is never dropped under them: ndt_ensure_map compares and refuses instead.
  if (((float)p->resolution != (float)h->p.resolution || p->min_points_per_voxel != h->p.min_points_per_voxel || p->min_covar_eigvalue_mult != h->p.min_covar_eigvalue_mult) &&
      h->tgt.use_count() == 1)
    h->tgt->map_valid = false;
  h->p = *p;
  return GORIO_OK;
}

int gorio_ndt_get_params(const gorio_ndt_t* h, gorio_ndt_params* p) {
  if (!h || !p) return ndt_fail(GORIO_ERR_INVALID, "get_params: null argument");
  *p = h->p;
  return GORIO_OK;
}

// setInputTarget, NDTH:122-127 (init() runs at the next call that needs the map)
int gorio_ndt_set_target(gorio_ndt_t* h, const float* xyz, int n, int stride_bytes) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_target: null handle");
  if (n < 0 || (n > 0 && (!xyz || stride_bytes < 12 || stride_bytes % 4))) return ndt_fail(GORIO_ERR_INVALID, "set_target: bad cloud arguments");
  if (n > INT_MAX / 2) return ndt_fail(GORIO_ERR_INVALID, "set_target: too many points");
  ndt_make_private(h);
  gorio::NdtTarget& t = *h->tgt;
  t.map_valid = false;
  t.has_target = false;
  h->nb_valid = false;
  if (const int rc = ndt_upload(h, xyz, n, stride_bytes, t.tx, t.ty, t.tz, t.t_cap)) return rc;
  t.n_t = n;
  t.has_target = true;
  return GORIO_OK;
}

// setInputSource (pcl::Registration)
int gorio_ndt_set_source(gorio_ndt_t* h, const float* xyz, int n, int stride_bytes) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_source: null handle");
  if (n < 0 || (n > 0 && (!xyz || stride_bytes < 12 || stride_bytes % 4))) return ndt_fail(GORIO_ERR_INVALID, "set_source: bad cloud arguments");
  if (n > INT_MAX / 2) return ndt_fail(GORIO_ERR_INVALID, "set_source: too many points");
  const size_t st = n ? stride_bytes / 4 : 0;
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(xyz[st * i]) || !std::isfinite(xyz[st * i + 1]) || !std::isfinite(xyz[st * i + 2]))
      return ndt_fail(GORIO_ERR_INVALID, "set_source: point " + std::to_string(i) + " is not finite (the reference's cell index of it is undefined)");
  h->has_source = false;
  h->nb_valid = false;
  if (const int rc = ndt_upload(h, xyz, n, stride_bytes, h->sx, h->sy, h->sz, h->s_cap)) return rc;
  h->n_s = n;
  h->has_source = true;
  return GORIO_OK;
}

// setInputTarget from device arrays
int gorio_ndt_set_target_device(gorio_ndt_t* h, const float* x, const float* y, const float* z, int n) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_target_device: null handle");
  if (n < 0 || (n > 0 && (!x || !y || !z)) || n > INT_MAX / 2) return ndt_fail(GORIO_ERR_INVALID, "set_target_device: bad cloud arguments");
  return ndt_adopt(h, x, y, z, n, nullptr, false, "set_target_device");
}

// setInputSource from device arrays; the finiteness check runs on the device, in the pass that copies, BEFORE the source held is replaced
int gorio_ndt_set_source_device(gorio_ndt_t* h, const float* x, const float* y, const float* z, int n) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_source_device: null handle");
  if (n < 0 || (n > 0 && (!x || !y || !z)) || n > INT_MAX / 2) return ndt_fail(GORIO_ERR_INVALID, "set_source_device: bad cloud arguments");
  return ndt_adopt(h, x, y, z, n, nullptr, true, "set_source_device");
}

// no reference member: how many elements the handle's device buffers hold (they grow, they are never shrunk or freed by a smaller cloud)
int gorio_ndt_get_capacities(const gorio_ndt_t* h, long long* capacities) {
  if (!h || !capacities) return ndt_fail(GORIO_ERR_INVALID, "get_capacities: null argument");
  const bool own = h->tgt_owned;  // a sharer owns no target buffers
  capacities[0] = own ? (long long)h->tgt->t_cap : 0;
  capacities[1] = (long long)h->s_cap;
  capacities[2] = own ? (long long)h->tgt->l_cap : 0;
  capacities[3] = own ? (long long)h->tgt->keys.cap() : 0;
  return GORIO_OK;
}

// the leaves_ map of VoxelGridCovariance after applyFilter (VGC:60-370)
int gorio_ndt_get_voxels(gorio_ndt_t* h, int capacity, int* n_leaves, int* leaf_index, int* nr_points, double* mean, double* cov_raw, double* cov, double* icov, int* min_b,
                         int* div_b) {
  if (!h || !n_leaves) return ndt_fail(GORIO_ERR_INVALID, "get_voxels: null argument");
  if (!h->tgt->has_target) return ndt_fail(GORIO_ERR_STATE, "get_voxels: no target set");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  if (const int rc = ndt_ensure_map(h)) return ndt_fail(rc, "get_voxels: " + g_ndt_err);
  const gorio::NdtTarget& t = *h->tgt;
  *n_leaves = t.nl;
  for (int a = 0; a < 3; ++a) {
    if (min_b) min_b[a] = t.grid.min_b[a];
    if (div_b) div_b[a] = t.grid.div_b[a];
  }
  const bool any = leaf_index || nr_points || mean || cov_raw || cov || icov;
  if (!any || t.nl == 0) return GORIO_OK;
  if (capacity < t.nl) return ndt_fail(GORIO_ERR_INVALID, "get_voxels: capacity below the number of leaves");
  const size_t nl = t.nl;
  if (leaf_index) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(leaf_index, t.lidx, sizeof(int) * nl, hipMemcpyDeviceToHost, h->stream));
  if (nr_points) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(nr_points, t.lcnt, sizeof(int) * nl, hipMemcpyDeviceToHost, h->stream));
  if (mean) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(mean, t.lmean, sizeof(double) * 3 * nl, hipMemcpyDeviceToHost, h->stream));
  if (cov_raw) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(cov_raw, t.lraw, sizeof(double) * 9 * nl, hipMemcpyDeviceToHost, h->stream));
  if (cov) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(cov, t.lcov, sizeof(double) * 9 * nl, hipMemcpyDeviceToHost, h->stream));
  if (icov) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(icov, t.licov, sizeof(double) * 9 * nl, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

// pcl::NormalDistributionsTransform / pclomp's KDTREE: every neighbourhood is target_cells_.radiusSearch(x_trans_pt, resolution_)
int gorio_ndt_set_radius_search(gorio_ndt_t* h, int enable) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "set_radius_search: null handle");
  const bool on = enable != 0;
  if (on != h->radius) h->nb_valid = false;  // the map stays; the neighbour lists held belong to the other mode's past
  h->radius = on;
  return GORIO_OK;
}

int gorio_ndt_get_radius_search(const gorio_ndt_t* h, int* enabled) {
  if (!h || !enabled) return ndt_fail(GORIO_ERR_INVALID, "get_radius_search: null argument");
  *enabled = h->radius ? 1 : 0;
  return GORIO_OK;
}

// the centroid cloud of VGC:282-326 and the leaf position of every centroid
int gorio_ndt_get_centroids(gorio_ndt_t* h, int capacity, int* n_centroids, float* xyz, int* leaf_pos) {
  if (!h || !n_centroids) return ndt_fail(GORIO_ERR_INVALID, "get_centroids: null argument");
  if (!h->tgt->has_target) return ndt_fail(GORIO_ERR_STATE, "get_centroids: no target set");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  if (const int rc = ndt_ensure_map(h)) return ndt_fail(rc, "get_centroids: " + g_ndt_err);
  if (const int rc = ndt_ensure_centroids(h)) return ndt_fail(rc, "get_centroids: " + g_ndt_err);
  const gorio::NdtTarget& t = *h->tgt;
  *n_centroids = t.nc;
  if ((!xyz && !leaf_pos) || t.nc == 0) return GORIO_OK;
  if (capacity < t.nc) return ndt_fail(GORIO_ERR_INVALID, "get_centroids: capacity below the number of centroids");
  const size_t nc = (size_t)t.nc;
  std::vector<float> soa;
  try {
    soa.resize(3 * nc);
  } catch (const std::bad_alloc&) {
    return ndt_fail(GORIO_ERR_ALLOC, "get_centroids: out of host memory");
  }
  if (xyz) {
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(soa.data(), t.cx, sizeof(float) * nc, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(soa.data() + nc, t.cy, sizeof(float) * nc, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(soa.data() + 2 * nc, t.cz, sizeof(float) * nc, hipMemcpyDeviceToHost, h->stream));
  }
  if (leaf_pos) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(leaf_pos, t.c2l, sizeof(int) * nc, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(h->stream));
  if (xyz)
    for (size_t i = 0; i < nc; ++i) {
      xyz[3 * i] = soa[i];
      xyz[3 * i + 1] = soa[nc + i];
      xyz[3 * i + 2] = soa[2 * nc + i];
    }
  return GORIO_OK;
}

// the CSR of the handle's last radius evaluation: offsets [source size + 1], then per neighbour the leaf position and the squared distance
int gorio_ndt_get_neighbours(gorio_ndt_t* h, long long* offsets, int* leaf_pos, float* sqd, long long capacity) {
  if (!h) return ndt_fail(GORIO_ERR_INVALID, "get_neighbours: null handle");
  if (!h->nb_valid || !h->rs) return ndt_fail(GORIO_ERR_STATE, "get_neighbours: no radius evaluation to report (none yet, or the source, the target or the switch changed since)");
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));
  const size_t n = (size_t)h->nb_n;
  if (h->nb_empty) {
    if (offsets) std::fill(offsets, offsets + n + 1, 0LL);
    return GORIO_OK;
  }
  const std::vector<long long>& offs = ndt_rs_host_offsets(h->rs);
  if (offs.size() != n + 1) return ndt_fail(GORIO_ERR_STATE, "get_neighbours: internal error, the result held does not fit the source");
  const long long total = offs[n];
  if ((leaf_pos || sqd) && capacity < total) return ndt_fail(GORIO_ERR_INVALID, "get_neighbours: capacity below the number of neighbours");
  if (offsets) std::copy(offs.begin(), offs.end(), offsets);
  if (total == 0 || (!leaf_pos && !sqd)) return GORIO_OK;
  const gorio::NdtTarget& t = *h->tgt;
  NdtRadiusJob job{h->rs, t.cent, nullptr, 0, 0.0, NdtCsr{}};
  ndt_rs_csr(&job);
  hipStream_t stream = ndt_rs_stream(t.cent);
  std::vector<int> c2l;
  try {
    c2l.resize((size_t)t.nc);
  } catch (const std::bad_alloc&) {
    return ndt_fail(GORIO_ERR_ALLOC, "get_neighbours: out of host memory");
  }
  if (leaf_pos) {
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(leaf_pos, job.csr.idx, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, stream));
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(c2l.data(), t.c2l, sizeof(int) * (size_t)t.nc, hipMemcpyDeviceToHost, stream));
  }
  if (sqd) GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(sqd, job.csr.sqd, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(stream));
  if (leaf_pos)
    for (long long k = 0; k < total; ++k) leaf_pos[k] = (leaf_pos[k] >= 0 && leaf_pos[k] < t.nc) ? c2l[(size_t)leaf_pos[k]] : -1;
  return GORIO_OK;
}

// computeDerivatives, NDT:180-285
int gorio_ndt_derivatives(gorio_ndt_t* h, const double* p, int compute_hessian, double* score, double* gradient, double* hessian) {
  if (const int rc = ndt_ready(h, "derivatives")) return rc;
  if (!p || !score || !gradient || (compute_hessian && !hessian)) return ndt_fail(GORIO_ERR_INVALID, "derivatives: null argument");
  NdtState st;
  ndt_pose_matrix(p, st.T);
  if (const int rc = ndt_derivs_at(h, st, p, st.T, compute_hessian != 0)) return rc;
  *score = st.score;
  std::copy(st.g, st.g + 6, gradient);
  if (compute_hessian) std::copy(st.H, st.H + 36, hessian);
  return GORIO_OK;
}

// computeHessian, NDT:540-645
int gorio_ndt_hessian(gorio_ndt_t* h, const double* p, double* hessian) {
  if (const int rc = ndt_ready(h, "hessian")) return rc;
  if (!p || !hessian) return ndt_fail(GORIO_ERR_INVALID, "hessian: null argument");
  float T[16];
  double acc[28];
  ndt_pose_matrix(p, T);
  const gorio::NdtEval ev = ndt_make_eval(h, p, T);
  if (const int rc = ndt_evaluate(h, ev, 2, acc)) return rc;
  ndt_unpack_hessian(acc, hessian);
  return GORIO_OK;
}

// calculateScore, NDT:935-983
int gorio_ndt_calculate_score(gorio_ndt_t* h, const float* T, double* score) {
  if (const int rc = ndt_ready(h, "calculate_score")) return rc;
  if (!T || !score) return ndt_fail(GORIO_ERR_INVALID, "calculate_score: null argument");
  double acc[28];
  const gorio::NdtEval ev = ndt_make_eval(h, nullptr, T);
  if (const int rc = ndt_evaluate(h, ev, 3, acc)) return rc;
  *score = acc[0] / (double)h->n_s;  // NDT:982
  return GORIO_OK;
}

// computeTransformation, NDT:81-171
int gorio_ndt_align(gorio_ndt_t* h, const float* guess, float* T_out, int* converged, int* nr_iterations, double* trans_probability, gorio_ndt_diag* diag) {
  if (const int rc = ndt_ready(h, "align")) return rc;
  if (!T_out) return ndt_fail(GORIO_ERR_INVALID, "align: null argument");
  NdtMachine m;
  m.begin(h, guess);
  while (!m.done()) {
    double acc[28];
    const gorio::NdtEval ev = ndt_make_eval(h, m.x_eval, m.st.T);
    if (const int rc = ndt_evaluate(h, ev, m.mode, acc)) return rc;
    m.resume(acc);
  }
  m.results(T_out, converged, nr_iterations, trans_probability, diag);
  return GORIO_OK;
}

// h looks at owner's target state from now on
int gorio_ndt_set_target_shared(gorio_ndt_t* h, gorio_ndt_t* owner) {
  if (!h || !owner) return ndt_fail(GORIO_ERR_INVALID, "set_target_shared: null handle");
  if (h->device != owner->device) return ndt_fail(GORIO_ERR_INVALID, "set_target_shared: both handles must live on one device");
  if (!owner->tgt->has_target) return ndt_fail(GORIO_ERR_STATE, "set_target_shared: the owner has no target");
  if (h == owner || h->tgt == owner->tgt) return GORIO_OK;
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(h->device));  // h's own state may die here
  h->nb_valid = false;
  h->tgt = owner->tgt;  // points and voxel map: one copy on the device, alive until the last handle lets go of it
  h->tgt_owned = false;
  return GORIO_OK;
}

// computeTransformation for many handles, one evaluation of every unfinished handle per round
int gorio_ndt_align_batch(gorio_ndt_t* const* handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* trans_probability,
                          gorio_ndt_diag* diag, gorio_ndt_batch_stats* stats) {
  using namespace gorio;
  if (count == 0) {
    if (stats) *stats = gorio_ndt_batch_stats{0, 0, 0};
    return GORIO_OK;
  }
  if (count < 0 || !handles || !T_out) return ndt_fail(GORIO_ERR_INVALID, "align_batch: bad arguments (count < 0, or no handles, or no T_out)");
  // ---- validation: nothing is built, allocated or launched before every handle has passed
  if (const int rc = ndt_batch_check(handles, count, "align_batch")) return rc;
  gorio_ndt* lead = handles[0];  // its stream carries the rounds, its scratch holds the tables and the sums
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(lead->device));
  if (const int rc = ndt_batch_maps(handles, count, "align_batch")) return rc;
  if (const int rc = ndt_batch_radius_prepare(handles, count, "align_batch")) return rc;
  // ---- scratch for the largest possible round: every handle pending
  size_t max_blocks = 0;
  for (int i = 0; i < count; ++i) max_blocks += (size_t)(handles[i]->n_s + 255) / 256;
  const size_t jobs_bytes = sizeof(NdtJob) * (size_t)count, table_bytes = jobs_bytes + sizeof(int2) * max_blocks;
  GORIO_HIP_CHECK(ndt_fail, lead->b_jobs.reserve(table_bytes, table_bytes + table_bytes / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_h_jobs.reserve(table_bytes, table_bytes + table_bytes / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_partials.reserve(28 * max_blocks, 28 * (max_blocks + max_blocks / 4)));
  GORIO_HIP_CHECK(ndt_fail, lead->b_out.reserve((size_t)28 * count, (size_t)28 * (count + count / 4)));
  GORIO_HIP_CHECK(ndt_fail, lead->b_h_out.reserve(sizeof(double) * 28 * count, sizeof(double) * 28 * (count + count / 4)));
  std::vector<NdtMachine> m;
  std::vector<int> order, rk;
  try {
    m.resize(count);
    order.reserve(count);
    rk.reserve(count);
  } catch (const std::bad_alloc&) {
    return ndt_fail(GORIO_ERR_ALLOC, "align_batch: out of host memory");
  }
  for (int i = 0; i < count; ++i) m[i].begin(handles[i], guesses ? guesses + (size_t)16 * i : nullptr);
  gorio_ndt_batch_stats bs{0, 0, 0};
  NdtJob* const h_jobs = static_cast<NdtJob*>(lead->b_h_jobs.get());
  std::vector<NdtRadiusJob> rjobs;
  const hipStream_t stream = ndt_batch_stream(handles, count);
  for (;;) {
    // the pending evaluations, grouped by neighbourhood source and mode (DIRECT 0, 1, 2, then radius 0, 1, 2): job k of the round belongs
    // to handle order[k]
    order.clear();
    int group_first_block[7] = {0, 0, 0, 0, 0, 0, 0};
    int blocks = 0;
    rk.clear();
    for (int group = 0; group < 6; ++group) {
      group_first_block[group] = blocks;
      for (int i = 0; i < count; ++i)
        if (!m[i].done() && m[i].mode == group % 3 && handles[i]->radius == (group >= 3)) {
          blocks += (handles[i]->n_s + 255) / 256;
          if (group >= 3) rk.push_back((int)order.size());
          order.push_back(i);
        }
    }
    group_first_block[6] = blocks;
    const int njobs = (int)order.size();
    if (njobs == 0) break;
    int2* const h_wg = reinterpret_cast<int2*>(h_jobs + njobs);
    int slot = 0;
    for (int k = 0; k < njobs; ++k) {
      gorio_ndt* h = handles[order[k]];
      const NdtMachine& mk = m[order[k]];
      ndt_fill_job(h_jobs[k], h, mk.mode, slot, ndt_make_eval(h, mk.x_eval, mk.st.T));
      for (int b = 0; b < h_jobs[k].nblk; ++b) h_wg[slot + b] = make_int2(k, b);
      slot += h_jobs[k].nblk;
    }
    const size_t bytes = sizeof(NdtJob) * (size_t)njobs + sizeof(int2) * (size_t)blocks;  // <= table_bytes
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(lead->b_jobs.get(), h_jobs, bytes, hipMemcpyHostToDevice, stream));
    NdtJob* d_jobs = static_cast<NdtJob*>(lead->b_jobs.get());
    const int2* d_wg = reinterpret_cast<const int2*>(d_jobs + njobs);
    if (const int rc = ndt_batch_neighbours(handles, order, rk, h_jobs, d_jobs, d_wg + group_first_block[3], group_first_block[6] - group_first_block[3], stream, rjobs,
                                            &bs.launches))
      return rc;
    for (int group = 0; group < 6; ++group) {
      const int nb = group_first_block[group + 1] - group_first_block[group];
      if (nb == 0) continue;
      ndt_launch_batch(group % 3, group >= 3, nb, stream, d_jobs, d_wg + group_first_block[group], lead->b_partials.get());
      bs.launches++;
    }
    ndt_fold_batch_kernel<<<njobs, 64, 0, stream>>>(d_jobs, lead->b_partials, 28, lead->b_out);
    bs.launches++;
    GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
    GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(lead->b_h_out.get(), lead->b_out, sizeof(double) * 28 * njobs, hipMemcpyDeviceToHost, stream));
    GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(stream));  // the pinned tables are free again after it
    ndt_batch_neighbours_done(handles, order, rk);
    const double* sums = static_cast<const double*>(lead->b_h_out.get());
    for (int k = 0; k < njobs; ++k) m[order[k]].resume(sums + (size_t)28 * k);
    bs.rounds++;
    bs.evaluations += njobs;
  }
  for (int i = 0; i < count; ++i)
    m[i].results(T_out + (size_t)16 * i, converged ? converged + i : nullptr, nr_iterations ? nr_iterations + i : nullptr, trans_probability ? trans_probability + i : nullptr,
                 diag ? diag + i : nullptr);
  if (stats) *stats = bs;
  return GORIO_OK;
}

// calculateScore, NDT:935-983, for many handles: one job table, one score launch, one fold launch, one copy, one synchronisation
int gorio_ndt_calculate_score_batch(gorio_ndt_t* const* handles, int count, const float* T, double* score) {
  using namespace gorio;
  if (count == 0) return GORIO_OK;
  if (count < 0 || !handles || !score) return ndt_fail(GORIO_ERR_INVALID, "calculate_score_batch: bad arguments (count < 0, or no handles, or no score)");
  if (const int rc = ndt_batch_check(handles, count, "calculate_score_batch")) return rc;
  gorio_ndt* lead = handles[0];  // its stream carries the launches, its batch scratch holds the table and the sums
  GORIO_HIP_CHECK(ndt_fail, hipSetDevice(lead->device));
  if (const int rc = ndt_batch_maps(handles, count, "calculate_score_batch")) return rc;
  if (const int rc = ndt_batch_radius_prepare(handles, count, "calculate_score_batch")) return rc;
  size_t blocks = 0;
  for (int i = 0; i < count; ++i) blocks += (size_t)(handles[i]->n_s + 255) / 256;
  if (blocks > (size_t)INT_MAX) return ndt_fail(GORIO_ERR_INVALID, "calculate_score_batch: too many source points in one batch");
  const size_t bytes = sizeof(NdtJob) * (size_t)count + sizeof(int2) * blocks;
  GORIO_HIP_CHECK(ndt_fail, lead->b_jobs.reserve(bytes, bytes + bytes / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_h_jobs.reserve(bytes, bytes + bytes / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_partials.reserve(blocks, blocks + blocks / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_out.reserve((size_t)count, (size_t)count + count / 4));
  GORIO_HIP_CHECK(ndt_fail, lead->b_h_out.reserve(sizeof(double) * count, sizeof(double) * (count + count / 4)));
  static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  NdtJob* const h_jobs = static_cast<NdtJob*>(lead->b_h_jobs.get());
  int2* const h_wg = reinterpret_cast<int2*>(h_jobs + count);
  const hipStream_t stream = ndt_batch_stream(handles, count);
  std::vector<int> order((size_t)count), rk;
  int slot = 0;
  for (int k = 0; k < count; ++k) {  // job k is handle k; its partial slots follow handle order
    order[k] = k;
    ndt_fill_job(h_jobs[k], handles[k], 3, slot, ndt_make_eval(handles[k], nullptr, T ? T + (size_t)16 * k : kIdentity));
    slot += h_jobs[k].nblk;
  }
  // the (job, block) table: the DIRECT jobs' workgroups first, then the radius jobs'.  x < count, y < nblk: what the kernels rely on
  int w = 0, direct_blocks = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) direct_blocks = w;
    for (int k = 0; k < count; ++k) {
      if (handles[k]->radius != (pass == 1)) continue;
      if (pass == 1) rk.push_back(k);
      for (int b = 0; b < h_jobs[k].nblk; ++b) h_wg[w++] = make_int2(k, b);
    }
  }
  const int radius_blocks = (int)blocks - direct_blocks;
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(lead->b_jobs.get(), h_jobs, bytes, hipMemcpyHostToDevice, stream));
  NdtJob* d_jobs = static_cast<NdtJob*>(lead->b_jobs.get());
  const int2* d_wg = reinterpret_cast<const int2*>(d_jobs + count);
  std::vector<NdtRadiusJob> rjobs;
  int launches = 0;
  if (const int rc = ndt_batch_neighbours(handles, order, rk, h_jobs, d_jobs, d_wg + direct_blocks, radius_blocks, stream, rjobs, &launches)) return rc;
  if (direct_blocks) ndt_score_batch_kernel<<<direct_blocks, 256, 0, stream>>>(d_jobs, d_wg, lead->b_partials.get());
  if (radius_blocks) ndt_score_csr_batch_kernel<<<radius_blocks, 256, 0, stream>>>(d_jobs, d_wg + direct_blocks, lead->b_partials.get());
  ndt_fold_batch_kernel<<<count, 64, 0, stream>>>(d_jobs, lead->b_partials, 1, lead->b_out);
  GORIO_HIP_CHECK(ndt_fail, hipGetLastError());
  GORIO_HIP_CHECK(ndt_fail, hipMemcpyAsync(lead->b_h_out.get(), lead->b_out, sizeof(double) * count, hipMemcpyDeviceToHost, stream));
  GORIO_HIP_CHECK(ndt_fail, hipStreamSynchronize(stream));  // the pinned table is free again after it
  ndt_batch_neighbours_done(handles, order, rk);
  const double* sums = static_cast<const double*>(lead->b_h_out.get());
  for (int k = 0; k < count; ++k) score[k] = sums[k] / (double)handles[k]->n_s;  // NDT:982
  return GORIO_OK;
}

}  // extern "C"
