// apd_voxel_group.hip -- grouping the points of a cloud by cell: the device half that every voxel structure of this library shares.
// Included by apd_api.hip before apd_submap.hip.
//
// The pipeline: a cell id per point, keys = cell id << SHIFT | input index (or the bare cell key, SHIFT = 0), the tiled key sort
// (enqueue_tiled_sort, apd_index.hip), the run starts per 256-key block, an exclusive scan of the block counts, and one lane per run start
// that walks its run in input order at the run's rank in ascending cell order.
//   cell_run_start         the preamble of every count / accumulate / centre kernel: is this lane a run start, and which one of its block
//   cell_count_kernel      run starts per 256-key block -> counts[block]
//   block_scan_kernel      ONE workgroup scans the block counts (exclusive, in place) and leaves the total behind them; also the scan of
//                          the ordered compactions (apd_scan.hip, apd_keyframes.hip, apd_map.hip, apd_vgicp_cuda.hip, apd_approx_voxel.hip)
// and, for the floor(x / resolution - 0.5) cell rule of fast_gicp (FastVGICP in double, NDTCuda and FastVGICPCuda in float):
//   voxel_axis             one axis of the rule, one overload per scalar: the two DO put some points in different cells
//   cell_bbox_init_kernel, cell_coord_bbox_kernel   bounding box of the occupied coordinates, range flag
//   cell_key_kernel        keys[i] = linear id inside the box << 31 | i
// pcl::VoxelGrid (apd_submap.hip), the NDT_OMP grid (apd_ndt.hip) and the map cloud (apd_map.hip) follow other libraries' cell rules and
// keep bounding-box and key kernels of their own; they share the run-start preamble, the count and the scan.
#include <hip/hip_runtime.h>

namespace gorio {

struct RunStart {
  bool start;   // this lane's key is the first of its cell's run
  int local;    // run starts of this block before this lane: rank = offsets[block] + local
  int in_block; // run starts of the whole block
};

// EVERY lane of a 256-lane block calls this (it contains the barrier).  Lane p = blockIdx.x * 256 + threadIdx.x looks at sorted key p of n;
// the cell of a key is key >> SHIFT.  SKIP_PAD: the all-ones key starts no run (the map cloud gives it to the non-finite ones of its n
// points, which sort behind the cells).
template <int SHIFT, bool SKIP_PAD = false>
__device__ __forceinline__ RunStart cell_run_start(const unsigned long long* __restrict__ keys, int n) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const bool start = p < n && (!SKIP_PAD || keys[p] != ~0ull) && (p == 0 || (keys[p] >> SHIFT) != (keys[p - 1] >> SHIFT));
  const unsigned long long m = __ballot(start);
  __shared__ int sw[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sw[wv] = __builtin_popcountll(m);
  __syncthreads();
  int local = __builtin_popcountll(m & ((1ull << lane) - 1ull));
  for (int q = 0; q < wv; ++q) local += sw[q];
  return RunStart{start, local, (sw[0] + sw[1]) + (sw[2] + sw[3])};
}

// number of run starts per 256-key block -> counts[block]
template <int SHIFT, bool SKIP_PAD = false>
__global__ __launch_bounds__(256) void cell_count_kernel(const unsigned long long* __restrict__ keys, int n, int* __restrict__ counts) {
  const RunStart rs = cell_run_start<SHIFT, SKIP_PAD>(keys, n);
  if (threadIdx.x == 0) counts[blockIdx.x] = rs.in_block;
}

// grid 1, block 1024.  bcnt[0 .. nb) becomes its exclusive prefix sum, bcnt[nb] the total.  nb is uniform, so every thread makes the
// same number of trips round the loop and meets every barrier.
__global__ __launch_bounds__(1024) void block_scan_kernel(int* __restrict__ bcnt, int nb) {
  __shared__ int wsum[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nb; base += 1024) {
    const int i = base + threadIdx.x;
    const int v = i < nb ? bcnt[i] : 0;
    int s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d);
      if (lane >= d) s += t;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    int woff = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (k < wave) woff += wsum[k];
      tot += wsum[k];
    }
    if (i < nb) bcnt[i] = carry + woff + (s - v);
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) bcnt[nb] = carry;
}

// ---- the floor(x / resolution - 0.5) rule

constexpr int kVoxCoordLimit = 1 << 30;  // |coordinate| below this: +-1 neighbours and the box arithmetic stay inside int32

// one axis of voxel_coord, fast_vgicp_voxel.hpp:158-160: floor(x / resolution - 0.5) in double; false when the value does not fit (or
// is not finite)
__device__ __forceinline__ bool voxel_axis(double v, double res, int& c) {
  double q = v / res;
  q = q - 0.5;
  q = floor(q);
  const bool ok = q > -(double)kVoxCoordLimit && q < (double)kVoxCoordLimit;  // false for NaN
  c = ok ? (int)q : 0;
  return ok;
}
// one axis of calc_voxel_coord, gaussian_voxelmap.cu:118-121: (int)floorf(x / res - 0.5f), in float
__device__ __forceinline__ bool voxel_axis(float v, float res, int& c) {
  float q = v / res;
  q = q - 0.5f;
  q = floorf(q);
  const bool ok = q > -(float)kVoxCoordLimit && q < (float)kVoxCoordLimit;  // false for NaN
  c = ok ? (int)q : 0;
  return ok;
}

// bb[0..2] min, bb[3..5] max of the occupied coordinates, bb[6], bb[7] = 0: flags and counts of the kernel that follows (here bb[6] != 0:
// a point whose coordinate does not fit)
__global__ void cell_bbox_init_kernel(int* __restrict__ bb) {
  if (threadIdx.x < 3) bb[threadIdx.x] = INT_MAX;
  else if (threadIdx.x < 6) bb[threadIdx.x] = INT_MIN;
  else if (threadIdx.x < 8) bb[threadIdx.x] = 0;
}

template <typename Real>
__global__ __launch_bounds__(256) void cell_coord_bbox_kernel(const float4* __restrict__ pts, int n, Real res, int* __restrict__ bb) {
  int lo0 = INT_MAX, lo1 = INT_MAX, lo2 = INT_MAX, hi0 = INT_MIN, hi1 = INT_MIN, hi2 = INT_MIN, bad = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float4 p = pts[i];
    int c0, c1, c2;
    bool ok = voxel_axis((Real)p.x, res, c0);
    ok = voxel_axis((Real)p.y, res, c1) && ok;
    ok = voxel_axis((Real)p.z, res, c2) && ok;
    if (!ok) {
      bad = 1;
      continue;
    }
    lo0 = min(lo0, c0); lo1 = min(lo1, c1); lo2 = min(lo2, c2);
    hi0 = max(hi0, c0); hi1 = max(hi1, c1); hi2 = max(hi2, c2);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo0 = min(lo0, __shfl_down(lo0, off, 64)); lo1 = min(lo1, __shfl_down(lo1, off, 64)); lo2 = min(lo2, __shfl_down(lo2, off, 64));
    hi0 = max(hi0, __shfl_down(hi0, off, 64)); hi1 = max(hi1, __shfl_down(hi1, off, 64)); hi2 = max(hi2, __shfl_down(hi2, off, 64));
    bad |= __shfl_down(bad, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(bb + 0, lo0); atomicMin(bb + 1, lo1); atomicMin(bb + 2, lo2);
    atomicMax(bb + 3, hi0); atomicMax(bb + 4, hi1); atomicMax(bb + 5, hi2);
    if (bad) atomicOr(bb + 6, 1);
  }
}

template <typename Real>
struct CellBox {
  int min_c[3];
  int dim[3];
  Real res;
};
using VoxBox = CellBox<double>;   // FastVGICP
using NdtcBox = CellBox<float>;   // NDTCuda, FastVGICPCuda

// keys[i] = linear voxel id << 31 | i (id < 2^33, checked on the host): the sort puts a voxel's points in INPUT order behind its first
// key; ~0 for the sort's padding
template <typename Real>
__global__ __launch_bounds__(256) void cell_key_kernel(const float4* __restrict__ pts, int n, int npow2, CellBox<Real> g, unsigned long long* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npow2) return;
  unsigned long long key = ~0ull;
  if (i < n) {
    const float4 p = pts[i];
    int c0, c1, c2;
    voxel_axis((Real)p.x, g.res, c0);
    voxel_axis((Real)p.y, g.res, c1);
    voxel_axis((Real)p.z, g.res, c2);
    const unsigned long long id = ((unsigned long long)(c0 - g.min_c[0]) * (unsigned long long)g.dim[1] + (unsigned long long)(c1 - g.min_c[1])) * (unsigned long long)g.dim[2] + (unsigned long long)(c2 - g.min_c[2]);
    key = (id << 31) | (unsigned long long)i;
  }
  keys[i] = key;
}

}  // namespace gorio
