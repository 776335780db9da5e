// apd_voxel.hip -- FastVGICP on the device: Gaussian voxel map of the target, pose-dependent voxel lookups, linearisation over the
// (source point, voxel) pairs.  Included by apd_api.hip after apd_submap.hip (it reuses the LDS bitonic sort of the search-index build and
// the cell grouping of apd_voxel_group.hip: voxel_axis, the bounding-box and key kernels in double, the run starts, the count and the scan).
//
// Reference lines (paths relative to /root/reference/fast_apdgicp/include/fast_gicp/gicp):
//   VG  = impl/fast_vgicp_impl.hpp     VOX = fast_vgicp_voxel.hpp
//
//   cell_coord_bbox_kernel<double>, cell_key_kernel<double> (apd_voxel_group.hip)   voxel_coord (VOX:158-160) of every target point
//   vg_accum_kernel        one lane per voxel: append() in input order and finalize() (VOX:79-122), fp64 -- the order of the sums is the
//                          reference's (create_voxelmap walks the cloud once, VOX:131-151), so the map does not depend on scheduling
//   vgicp_linearize_kernel one lane per (source point, offset) slot: T * mean_A in double, un-fused, column order (VG:84-86), voxel_coord,
//                          lookup (binary search over the ascending ids), RCR and its inverse (VG:110-114), weighted J^T O J / J^T O e /
//                          error (VG:136-168); 28 fp64 accumulators per lane, the wave -> block reduction of linearize_kernel
//   vgicp_error_part       compute_error (VG:183-204) over the slots of the last linearise (inside lm_solve_vgicp_kernel)
//
// Lookup is a binary search and not a hash table: the sorted ids exist anyway once the points are grouped, there is no second build step
// and no load factor to choose, the result cannot depend on an insertion order, and log2(n_voxels) <= 17 probes of an L2-resident 8-byte
// array are small against the ~250 fp64 operations of an occupied slot.
#include <hip/hip_runtime.h>

namespace gorio {

// Eigen Isometry3d * Vector4d (VG:85): ((m0 x + m1 y) + m2 z) + m3 * 1 per row, double, NO fused multiply-add: the voxel a point
// falls into must not depend on how a compiler contracts the sum (this file is built with -ffp-contract=off)
__device__ __forceinline__ void transform_d(const double* __restrict__ T, double x, double y, double z, double& qx, double& qy, double& qz) {
  double a = T[0] * x;
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

// one lane per voxel start of the sorted keys (rank = position in ascending id order, cell_run_start): the
// voxel's points in input order.  mode 0 / 1: AdditiveGaussianVoxel (VOX:105-122; ADDITIVE_WEIGHTED builds the same voxel, VOX:138-141),
// mode 2: MultiplicativeGaussianVoxel (VOX:79-103).  The 4x4 matrices of the reference decouple: row / column 3 of a covariance are zero
// (with (3,3) set to 1 before every inverse), so the 3x3 block is inverted and component 3 of the mean is 1.
__global__ __launch_bounds__(256) void vg_accum_kernel(const unsigned long long* __restrict__ keys, const float4* __restrict__ pts, const double* __restrict__ cov6, int n,
                                                       const int* __restrict__ offsets, int mode, unsigned long long* __restrict__ vkey, double* __restrict__ vmean,
                                                       double* __restrict__ vcov6, int* __restrict__ vnum) {
  const RunStart rs = cell_run_start<31>(keys, n);
  if (!rs.start) return;
  const int p = blockIdx.x * 256 + threadIdx.x, rank = offsets[blockIdx.x] + rs.local;
  const unsigned long long vox = keys[p] >> 31;
  double m0 = 0.0, m1 = 0.0, m2 = 0.0;
  double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
  int cnt = 0;
  for (int j = p; j < n && (keys[j] >> 31) == vox; ++j) {  // input order inside the voxel (the key's low bits ascend)
    const int i = (int)(keys[j] & 0x7fffffffull);
    const float4 v = pts[i];
    const double* c = cov6 + (size_t)i * 6;
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z;
    if (mode != 2) {  // VOX:112-116
      m0 += x; m1 += y; m2 += z;
      s00 += c[0]; s01 += c[1]; s02 += c[2]; s11 += c[3]; s12 += c[4]; s22 += c[5];
    } else {          // VOX:86-94
      double i00, i01, i02, i11, i12, i22;
      inv_sym3(c[0], c[1], c[2], c[3], c[4], c[5], i00, i01, i02, i11, i12, i22);
      s00 += i00; s01 += i01; s02 += i02; s11 += i11; s12 += i12; s22 += i22;
      m0 += (i00 * x + i01 * y) + i02 * z;
      m1 += (i01 * x + i11 * y) + i12 * z;
      m2 += (i02 * x + i12 * y) + i22 * z;
    }
    ++cnt;
  }
  double* om = vmean + (size_t)rank * 3;
  double* oc = vcov6 + (size_t)rank * 6;
  if (mode != 2) {  // VOX:118-121
    const double d = (double)cnt;
    om[0] = m0 / d; om[1] = m1 / d; om[2] = m2 / d;
    oc[0] = s00 / d; oc[1] = s01 / d; oc[2] = s02 / d; oc[3] = s11 / d; oc[4] = s12 / d; oc[5] = s22 / d;
  } else {          // VOX:96-102
    double i00, i01, i02, i11, i12, i22;
    inv_sym3(s00, s01, s02, s11, s12, s22, i00, i01, i02, i11, i12, i22);
    oc[0] = i00; oc[1] = i01; oc[2] = i02; oc[3] = i11; oc[4] = i12; oc[5] = i22;
    om[0] = (i00 * m0 + i01 * m1) + i02 * m2;
    om[1] = (i01 * m0 + i11 * m1) + i12 * m2;
    om[2] = (i02 * m0 + i12 * m1) + i22 * m2;
  }
  vkey[rank] = vox;
  vnum[rank] = cnt;
}

// lookup_voxel (VOX:167-174): position of voxel (c0, c1, c2) in the ascending order, or -1.  A coordinate outside the bounding box of
// the occupied voxels cannot be occupied.
template <typename MapView>  // VoxelMapView, or the float map of apd_ndt_cuda.hip
__device__ __forceinline__ int voxel_lookup(const MapView& vm, int c0, int c1, int c2) {
  const int r0 = c0 - vm.min_c[0], r1 = c1 - vm.min_c[1], r2 = c2 - vm.min_c[2];
  if (r0 < 0 || r1 < 0 || r2 < 0 || r0 >= vm.dim[0] || r1 >= vm.dim[1] || r2 >= vm.dim[2]) return -1;
  const unsigned long long id = ((unsigned long long)r0 * (unsigned long long)vm.dim[1] + (unsigned long long)r1) * (unsigned long long)vm.dim[2] + (unsigned long long)r2;
  int lo = 0, hi = vm.nv;  // first position whose id is >= id
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vm.vkey[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < vm.nv && vm.vkey[lo] == id) ? lo : -1;
}

// neighbour offset `o` of neighbor_offsets(method), VOX:16-43, without a table (a runtime-indexed private array would live in scratch)
__device__ __forceinline__ void voxel_offset(int n_off, int o, int& d0, int& d1, int& d2) {
  d0 = 0; d1 = 0; d2 = 0;
  if (n_off == 27) {  // VOX:36-41: i, j, k loops, (i - 1, j - 1, k - 1)
    d0 = o / 9 - 1;
    d1 = (o / 3) % 3 - 1;
    d2 = o % 3 - 1;
  } else if (n_off == 7 && o > 0) {  // VOX:22-28: centre, +x, -x, +y, -y, +z, -z
    const int axis = (o - 1) >> 1, sgn = (o & 1) ? 1 : -1;
    d0 = axis == 0 ? sgn : 0;
    d1 = axis == 1 ? sgn : 0;
    d2 = axis == 2 ? sgn : 0;
  }
}

// the slot a lane owns: voxel_coord(T * mean_A) + offset -> voxel index (VG:84-93)
__device__ __forceinline__ int voxel_slot(const VoxelMapView& vm, const double* __restrict__ T, float ax, float ay, float az, int n_off, int o) {
  double qx, qy, qz;
  transform_d(T, (double)ax, (double)ay, (double)az, qx, qy, qz);
  int c0, c1, c2, d0, d1, d2;
  bool ok = voxel_axis(qx, vm.res, c0);
  ok = voxel_axis(qy, vm.res, c1) && ok;
  ok = voxel_axis(qz, vm.res, c2) && ok;
  voxel_offset(n_off, o, d0, d1, d2);
  return ok ? voxel_lookup(vm, c0 + d0, c1 + d1, c2 + d2) : -1;
}

// grid: (ceil(n_source * n_off / 256), 1, pairs), block 256.  Writes the slot table, the weighted Mahalanobis blocks (when asked to) and one
// 28-double partial per block in the layout of linearize_kernel: [0..20] upper triangle of H, [21..26] b, [27] error.
__global__ __launch_bounds__(256) void vgicp_linearize_kernel(const PairDesc* __restrict__ descs, const VoxPair* __restrict__ vox) {
  const GridPos gp = xcd_grid_pos();
  const PairDesc& pd = descs[gp.z];
  const VoxPair& vp = vox[gp.z];
  const PairState* __restrict__ st = pd.state;
  if (st->done) return;
  const int n_off = vp.n_off;
  const long long total = (long long)pd.src.n * n_off;
  if ((long long)gp.x * 256 >= total) return;
  const long long t = (long long)gp.x * 256 + threadIdx.x;

  double acc[28];
#pragma unroll
  for (int q = 0; q < 28; ++q) acc[q] = 0.0;

  if (t < total) {
    const int i = (int)(t / n_off), o = (int)(t - (long long)i * n_off);
    double T[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = st->x0[q];
    const float ax = pd.src.x[i], ay = pd.src.y[i], az = pd.src.z[i];
    const int v = voxel_slot(vp.map, T, ax, ay, az, n_off, o);
    vp.slots[t] = v;
    double* om = vp.omega6 + (size_t)t * 6;
    if (v >= 0) {
      // tolerance arithmetic from here on (H, b, error agree with the host restatement to 1e-9): fused multiply-adds allowed
#pragma clang fp contract(fast)
      double cA[6], cB[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        cA[q] = pd.src.cov6[(size_t)i * 6 + q];
        cB[q] = vp.map.cov6[(size_t)v * 6 + q];
      }
      const double bx = vp.map.mean[(size_t)v * 3], by = vp.map.mean[(size_t)v * 3 + 1], bz = vp.map.mean[(size_t)v * 3 + 2];
      const double w = sqrt((double)vp.map.num[v]);  // VG:149
      // RCR = C_voxel + T C_A T^T, VG:110 (3x3 block; (3,3) is set to 1 before and to 0 after the inverse, VG:111-114)
      const double R00 = T[0], R01 = T[1], R02 = T[2], R10 = T[4], R11 = T[5], R12 = T[6], R20 = T[8], R21 = T[9], R22 = T[10];
      const double M00 = R00 * cA[0] + R01 * cA[1] + R02 * cA[2], M01 = R00 * cA[1] + R01 * cA[3] + R02 * cA[4], M02 = R00 * cA[2] + R01 * cA[4] + R02 * cA[5];
      const double M10 = R10 * cA[0] + R11 * cA[1] + R12 * cA[2], M11 = R10 * cA[1] + R11 * cA[3] + R12 * cA[4], M12 = R10 * cA[2] + R11 * cA[4] + R12 * cA[5];
      const double M20 = R20 * cA[0] + R21 * cA[1] + R22 * cA[2], M21 = R20 * cA[1] + R21 * cA[3] + R22 * cA[4], M22 = R20 * cA[2] + R21 * cA[4] + R22 * cA[5];
      const double q00 = cB[0] + (M00 * R00 + M01 * R01 + M02 * R02);
      const double q01 = cB[1] + (M00 * R10 + M01 * R11 + M02 * R12);
      const double q02 = cB[2] + (M00 * R20 + M01 * R21 + M02 * R22);
      const double q11 = cB[3] + (M10 * R10 + M11 * R11 + M12 * R12);
      const double q12 = cB[4] + (M10 * R20 + M11 * R21 + M12 * R22);
      const double q22 = cB[5] + (M20 * R20 + M21 * R21 + M22 * R22);
      double o00, o01, o02, o11, o12, o22;
      inv_sym3(q00, q01, q02, q11, q12, q22, o00, o01, o02, o11, o12, o22);
      o00 *= w; o01 *= w; o02 *= w; o11 *= w; o12 *= w; o22 *= w;  // the pair's weight multiplies H, b and the error alike (VG:150, 162-163)
      if (vp.write_omega) {
        om[0] = o00; om[1] = o01; om[2] = o02; om[3] = o11; om[4] = o12; om[5] = o22;
      }
      const double x = (double)ax, y = (double)ay, z = (double)az;
      const double a0 = T[0] * x + T[1] * y + T[2] * z + T[3];
      const double a1 = T[4] * x + T[5] * y + T[6] * z + T[7];
      const double a2 = T[8] * x + T[9] * y + T[10] * z + T[11];
      const double e0 = bx - a0, e1 = by - a1, e2 = bz - a2;  // VG:146-147
      const double oe0 = o00 * e0 + o01 * e1 + o02 * e2;
      const double oe1 = o01 * e0 + o11 * e1 + o12 * e2;
      const double oe2 = o02 * e0 + o12 * e1 + o22 * e2;
      acc[27] = e0 * oe0 + e1 * oe1 + e2 * oe2;  // VG:150
      // J = [skew(Ta) | -I], VG:156-160; the products as in linearize_kernel
      const double G00 = a2 * o01 - a1 * o02, G01 = a2 * o11 - a1 * o12, G02 = a2 * o12 - a1 * o22;
      const double G10 = -a2 * o00 + a0 * o02, G11 = -a2 * o01 + a0 * o12, G12 = -a2 * o02 + a0 * o22;
      const double G20 = a1 * o00 - a0 * o01, G21 = a1 * o01 - a0 * o11, G22 = a1 * o02 - a0 * o12;
      acc[0] = G01 * a2 - G02 * a1; acc[1] = -G00 * a2 + G02 * a0; acc[2] = G00 * a1 - G01 * a0; acc[3] = -G00; acc[4] = -G01; acc[5] = -G02;
      acc[6] = -G10 * a2 + G12 * a0; acc[7] = G10 * a1 - G11 * a0; acc[8] = -G10; acc[9] = -G11; acc[10] = -G12;
      acc[11] = G20 * a1 - G21 * a0; acc[12] = -G20; acc[13] = -G21; acc[14] = -G22;
      acc[15] = o00; acc[16] = o01; acc[17] = o02;
      acc[18] = o11; acc[19] = o12;
      acc[20] = o22;
      acc[21] = G00 * e0 + G01 * e1 + G02 * e2;
      acc[22] = G10 * e0 + G11 * e1 + G12 * e2;
      acc[23] = G20 * e0 + G21 * e1 + G22 * e2;
      acc[24] = -oe0; acc[25] = -oe1; acc[26] = -oe2;
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
  if (threadIdx.x < 28) pd.partials[(size_t)gp.x * 28 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// compute_error, VG:183-204: the slots (and weighted Mahalanobis blocks) of the last linearise at pose T; this thread's strided share
__device__ double vgicp_error_part(const PairDesc& pd, const VoxPair& vp, const double* __restrict__ T) {
#pragma clang fp contract(fast)
  const long long total = (long long)pd.src.n * vp.n_off;
  double sum = 0.0;
  for (long long t = threadIdx.x; t < total; t += blockDim.x) {
    const int v = vp.slots[t];
    if (v < 0) continue;
    const int i = (int)(t / vp.n_off);
    const double* om = vp.omega6 + (size_t)t * 6;
    const double x = (double)pd.src.x[i], y = (double)pd.src.y[i], z = (double)pd.src.z[i];
    const double e0 = vp.map.mean[(size_t)v * 3] - (T[0] * x + T[1] * y + T[2] * z + T[3]);
    const double e1 = vp.map.mean[(size_t)v * 3 + 1] - (T[4] * x + T[5] * y + T[6] * z + T[7]);
    const double e2 = vp.map.mean[(size_t)v * 3 + 2] - (T[8] * x + T[9] * y + T[10] * z + T[11]);
    const double m0 = om[0] * e0 + om[1] * e1 + om[2] * e2;
    const double m1 = om[1] * e0 + om[3] * e1 + om[4] * e2;
    const double m2 = om[2] * e0 + om[4] * e1 + om[5] * e2;
    sum += e0 * m0 + e1 * m1 + e2 * m2;
  }
  return sum;
}

}  // namespace gorio
