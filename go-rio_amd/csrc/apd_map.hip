// apd_map.hip -- the back end's map cloud from resident keyframes: include/gorio_map.h.  Kernels first, the host side below them.
// Included at the end of apd_api.hip, after apd_keyframes.hip: gorio_kf and KfEntry are complete there, and the ordered compaction's block
// scan (block_scan_kernel, apd_voxel_group.hip) and the tiled key sort (enqueue_tiled_sort, apd_index.hip) are reused from there.
//
// MCG = src/radar_graph_slam/map_cloud_generator.cpp, RGS = apps/radar_graph_slam_nodelet.cpp of the Go-RIO sources.
//
// Arithmetic: include/gorio_map.h fixes every operation, and tests/map_cloud_restatement.py restates them in NumPy; the kernels must give
// those bits.  Floating-point contraction is OFF for this file (the library's Makefile passes -ffp-contract=off, and the pragma below
// repeats it for a build that does not): every product and sum is rounded by itself.  No floating-point atomics anywhere: integer atomics
// on ranks, cell coordinates and counts give the same result in any order.
#include <hip/hip_runtime.h>

#include "../../include/gorio_map.h"

#pragma clang fp contract(off)

namespace gorio {

// ---------------------------------------------------------------------------------------------------------------- stage A (MCG:22-32)
// Three launches, as the submap assembly from keyframes (apd_keyframes.hip), none of which waits for another workgroup:
//   map_gate_count_kernel   per 256-point block of every frame: the points that pass the range gate, one ballot + popcount per wave
//   block_scan_kernel       ONE workgroup scans all block counts (exclusive, in place) and leaves the total behind
//   map_scatter_kernel      every block repeats its ballots and writes each kept point, transformed by the float pose, with its intensity,
//                           at its rank; with `anchor` it also takes the smallest rank whose transformed point is finite
// Blocks are numbered frame by frame (MapFrame::blk0), so ranks ascend in frame order and, inside a frame, in point order.
// grid: (max blocks of one frame, frames), block 256; a block beyond its frame's last one leaves at once (uniform per block).
struct MapFrame {
  const float4* p4;        // the keyframe's packed points (x, y, z, label); null when n == 0
  const float* intensity;  // n floats, or null: the keyframe has no intensity column
  int n;
  int blk0;                // index of this frame's first block in the count array
  float M[12];             // rows 0..2 of the pose cast to float, row-major
};
static_assert(sizeof(MapFrame) == 72, "include/gorio_map.h states what generate uploads per keyframe");

// MCG:25-26: d = src_pt.getVector3fMap().norm() in float, `if (d > 50) continue` in double.  NaN passes, an infinity does not.
__device__ __forceinline__ bool map_gate(const float4& p) {
  const float s = (p.x * p.x + p.y * p.y) + p.z * p.z;
  const float d = (float)sqrt((double)s);  // the correctly rounded float root: 53 bits are more than 2 * 24 + 2
  return !((double)d > 50.0);
}

__global__ __launch_bounds__(256) void map_gate_count_kernel(const MapFrame* __restrict__ frames, int* __restrict__ bcnt) {
  const int n = frames[blockIdx.y].n;
  if ((int)blockIdx.x * 256 >= n) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool k = i < n && map_gate(frames[blockIdx.y].p4[i]);
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) bcnt[frames[blockIdx.y].blk0 + blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

// What comes back to the host in one copy after the cell pass, and what the key and centre passes read.
struct MapRecord {
  int anchor_rank;  // smallest rank with a finite transformed point; INT_MAX without one (set by the host before the scatter)
  int kept;         // stage A's size
  int n_finite;
  int out_of_range; // a cell coordinate with |k| >= 2^30 (or not a number) was met
  int min_k[3], max_k[3];
  float q0[3];      // the anchor point
};
static_assert(sizeof(MapRecord) == 52, "include/gorio_map.h states the size of the record");

__device__ __forceinline__ bool map_finite(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__global__ __launch_bounds__(256) void map_scatter_kernel(const MapFrame* __restrict__ frames, const int* __restrict__ boffs, float4* __restrict__ out, int cap,
                                                          MapRecord* __restrict__ anchor) {
  const MapFrame& f = frames[blockIdx.y];
  const int n = f.n;
  if ((int)blockIdx.x * 256 >= n) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) p = f.p4[i];
  const bool k = i < n && map_gate(p);
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if (lane == 0) w[wave] = __popcll(b);
  __syncthreads();
  int pos = boffs[f.blk0 + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int q = 0; q < wave; ++q) pos += w[q];
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k) {
    q.x = ((f.M[0] * p.x + f.M[1] * p.y) + f.M[2] * p.z) + f.M[3];
    q.y = ((f.M[4] * p.x + f.M[5] * p.y) + f.M[6] * p.z) + f.M[7];
    q.z = ((f.M[8] * p.x + f.M[9] * p.y) + f.M[10] * p.z) + f.M[11];
    q.w = f.intensity ? f.intensity[i] : 0.0f;
    if (pos >= 0 && pos < cap) out[pos] = q;  // the ranks come from this call's own counts; cap is what the buffer holds
  }
  if (!anchor) return;
  // ranks ascend with the lane, so the wave's first finite kept lane holds its smallest such rank.  One atomic per wave at the most, and
  // none once a lower rank is known (the plain read may be stale, which only costs an atomic).
  const unsigned long long fin = __ballot(k && map_finite(q));
  if (fin != 0ull && lane == __ffsll((long long)fin) - 1 && pos < *(volatile int*)&anchor->anchor_rank) atomicMin(&anchor->anchor_rank, pos);
}

// ---------------------------------------------------------------------------------------------------------------- stage B (MCG:41-50)
//   map_cells_kernel          the anchor point, per finite point its cell k = floor((q - a) / res), the range flag, the integer box and the
//                             finite count (wave reductions, then integer atomics); grid-stride over a bounded grid
//   -- one copy of MapRecord to the host, where the limits are checked --
//   map_key_kernel            key = (kx - min) << 42 | (ky - min) << 21 | (kz - min); non-finite points and the padding get ~0
//   enqueue_tiled_sort        (apd_index.hip)
//   cell_count_kernel<0, true>  first occurrences of a key per 256-key block (apd_voxel_group.hip); block_scan_kernel scans them
//   map_centre_kernel         one centre per first occurrence at its rank, computed from the key: no gather of points
struct MapLattice {
  double a[3];   // (double)q0 - res / 2
  double res;
  int min_k[3];
};

__device__ __forceinline__ double map_cell(float q, double a, double res) { return floor(((double)q - a) / res); }

constexpr int kMapCellBlocks = 1024;  // 4096 waves: enough to fill the device, few enough that their atomics are noise

__global__ __launch_bounds__(256) void map_cells_kernel(const float4* __restrict__ pts, const int* __restrict__ kept_total, int cap, double res, MapRecord* __restrict__ rec) {
  const int kept = min(*kept_total, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) rec->kept = kept;
  const int r0 = rec->anchor_rank;  // written by the launch before this one
  if (r0 < 0 || r0 >= kept) return;  // no finite point: nothing to count (uniform for the whole grid)
  const float4 q0 = pts[r0];
  if (blockIdx.x == 0 && threadIdx.x == 0) rec->q0[0] = q0.x, rec->q0[1] = q0.y, rec->q0[2] = q0.z;
  const double a[3] = {(double)q0.x - res / 2, (double)q0.y - res / 2, (double)q0.z - res / 2};
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  int nfin = 0, bad = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < kept; i += gridDim.x * 256) {
    const float4 q = pts[i];
    if (!map_finite(q)) continue;
    ++nfin;
    const double kd[3] = {map_cell(q.x, a[0], res), map_cell(q.y, a[1], res), map_cell(q.z, a[2], res)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (!(fabs(kd[c]) < 1073741824.0)) {  // also catches a quotient that overflowed
        bad = 1;
      } else {
        const int k = (int)kd[c];
        lo[c] = min(lo[c], k);
        hi[c] = max(hi[c], k);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    nfin += __shfl_down(nfin, off, 64);
    bad |= __shfl_down(bad, off, 64);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = min(lo[c], __shfl_down(lo[c], off, 64));
      hi[c] = max(hi[c], __shfl_down(hi[c], off, 64));
    }
  }
  if ((threadIdx.x & 63) != 0 || nfin == 0) return;
  atomicAdd(&rec->n_finite, nfin);
  if (bad) atomicOr(&rec->out_of_range, 1);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (lo[c] <= hi[c]) {
      atomicMin(&rec->min_k[c], lo[c]);
      atomicMax(&rec->max_k[c], hi[c]);
    }
  }
}

// grid: ceil(npow2 / 256).  The host has checked that every finite point's cell lies within 2^21 - 1 of min_k; a key that would not fit
// is still written as padding rather than trusted.
__global__ __launch_bounds__(256) void map_key_kernel(const float4* __restrict__ pts, int kept, int npow2, MapLattice g, unsigned long long* __restrict__ keys) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= npow2) return;
  unsigned long long key = ~0ull;
  if (i < kept) {
    const float4 q = pts[i];
    if (map_finite(q)) {
      const double d0 = map_cell(q.x, g.a[0], g.res) - (double)g.min_k[0];
      const double d1 = map_cell(q.y, g.a[1], g.res) - (double)g.min_k[1];
      const double d2 = map_cell(q.z, g.a[2], g.res) - (double)g.min_k[2];
      if (d0 >= 0.0 && d0 < 2097152.0 && d1 >= 0.0 && d1 < 2097152.0 && d2 >= 0.0 && d2 < 2097152.0)
        key = ((unsigned long long)d0 << 42) | ((unsigned long long)d1 << 21) | (unsigned long long)d2;
    }
  }
  keys[i] = key;
}

// grid: ceil(n / 256) over the sorted keys of the kept points (the padding lies behind them).  A cell is a whole key, and the all-ones
// key of a non-finite point starts none: cell_run_start<0, true>.
__global__ __launch_bounds__(256) void map_centre_kernel(const unsigned long long* __restrict__ keys, int n, const int* __restrict__ offsets, MapLattice g, float4* __restrict__ out,
                                                         int cap) {
  const RunStart rs = cell_run_start<0, true>(keys, n);
  if (!rs.start) return;
  const int rank = offsets[blockIdx.x] + rs.local;
  if (rank < 0 || rank >= cap) return;
  const unsigned long long key = keys[blockIdx.x * 256 + threadIdx.x];
  const double k0 = (double)((long long)(key >> 42) + (long long)g.min_k[0]);
  const double k1 = (double)((long long)((key >> 21) & 0x1fffffull) + (long long)g.min_k[1]);
  const double k2 = (double)((long long)(key & 0x1fffffull) + (long long)g.min_k[2]);
  // genLeafNodeCenterFromOctreeKey: (key + 0.5) * resolution + lower corner, in double, rounded to float once
  out[rank] = make_float4((float)((k0 + 0.5) * g.res + g.a[0]), (float)((k1 + 0.5) * g.res + g.a[1]), (float)((k2 + 0.5) * g.res + g.a[2]), 0.0f);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_map.h)
namespace {
thread_local std::string g_map_err;
int map_fail(int code, const std::string& m) {
  g_map_err = m;
  return code;
}
}  // namespace

constexpr int kMapGetChunk = 1 << 18;  // points per staging chunk of gorio_map_get: 4 MiB

struct gorio_map {
  int device = 0;
  // device buffers: they grow and are kept when a smaller map follows
  DevBuf<void> d_frames;               // the frame table
  DevBuf<int> d_bcnt;                  // block counts of stage A, then of the voxel starts; [blocks] is the total
  DevBuf<float4> d_stage;              // stage A's output
  DevBuf<unsigned long long> d_keys;
  DevBuf<float4> d_result;             // the cloud of the last successful generate: stage A's output copied, or the centres
  DevBuf<void> d_rec;                  // one MapRecord
  PinnedBuf h_get;                     // two staging chunks of gorio_map_get
  hipStream_t stream = nullptr;        // the device's launch stream, known from the first generate on
  int n_result = 0;
  gorio_map_info_t info = {};
  long long generates = 0, points_downloaded = 0, bytes_uploaded = 0;
};

extern "C" {

const char* gorio_map_last_error(void) { return g_map_err.c_str(); }

int gorio_map_create(gorio_map_t** out, int device) {
  if (!out) return map_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  if (device < 0) return map_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  gorio_map* m = new (std::nothrow) gorio_map();
  if (!m) return map_fail(GORIO_ERR_ALLOC, "create: out of memory");
  m->device = device;
  *out = m;
  return GORIO_OK;
}

void gorio_map_destroy(gorio_map_t* m) {
  if (!m) return;
  if (m->stream) {
    hipSetDevice(m->device);  // the buffers are freed with their device current
    hipStreamSynchronize(m->stream);
  }
  delete m;
}

int gorio_map_generate(gorio_map_t* m, gorio_kf_t* kf, const int* ids, const double* poses, int count, double resolution, int* n_points) {
  if (!m || !kf || !ids || !poses || !n_points) return map_fail(GORIO_ERR_INVALID, "generate: null argument");
  if (count <= 0) return map_fail(GORIO_ERR_INVALID, "generate: count <= 0 (keyframes empty)");  // MCG:14-17
  if (count > 65535) return map_fail(GORIO_ERR_UNSUPPORTED, "generate: more than 65535 keyframes in one call");  // one grid row per keyframe
  if (std::isnan(resolution)) return map_fail(GORIO_ERR_INVALID, "generate: resolution is not a number");
  if (m->device != kf->device) return map_fail(GORIO_ERR_INVALID, "generate: the map and the store must live on one device");
  for (size_t q = 0; q < (size_t)count * 16; ++q) {
    if ((q & 15) < 12 && !std::isfinite(poses[q])) return map_fail(GORIO_ERR_INVALID, "generate: pose " + std::to_string(q / 16) + " has a non-finite entry");
  }
  std::vector<gorio::MapFrame> fr;
  std::vector<std::shared_ptr<DevCloud>> held;  // a share of every listed cloud for the duration of the call
  try {
    fr.resize(count);
    held.reserve(count);
  } catch (const std::bad_alloc&) {
    return map_fail(GORIO_ERR_ALLOC, "generate: out of memory");
  }
  long long total = 0, nblocks = 0;
  int max_blocks = 0;
  for (int k = 0; k < count; ++k) {
    int rc = GORIO_OK;
    std::string why;
    const KfEntry* e = kf_entry(kf, ids[k], &rc, &why);
    if (!e) return map_fail(rc, "generate: " + why);
    held.push_back(e->cloud);
    const int nb = (e->n + 255) / 256;
    fr[k].p4 = e->n > 0 ? e->cloud->p4.get() : nullptr;
    fr[k].intensity = (e->n > 0 && e->has_intensity) ? e->intensity.get() : nullptr;
    fr[k].n = e->n;
    fr[k].blk0 = (int)nblocks;
    for (int q = 0; q < 12; ++q) fr[k].M[q] = (float)poses[(size_t)k * 16 + q];
    total += e->n;
    nblocks += nb;
    max_blocks = std::max(max_blocks, nb);
    if (total > (long long)INT_MAX / 2) return map_fail(GORIO_ERR_INVALID, "generate: too many points");
  }
  gorio_map_info_t info = {};
  info.n_listed = (int)total;
  const bool voxels = resolution > 0.0;
  int kept = 0, n_out = 0;
  gorio::MapRecord rec = {}, rec0 = {};
  gorio::MapLattice lat = {};
  long long uploaded = 0;
  hipStream_t st = nullptr;
  if (total > 0) {
    // a keyframe exists, so the store has its device side: its stream is the device's launch stream, on which every keyframe was written
    st = kf->up->stream;
    GORIO_HIP_CHECK(map_fail, hipSetDevice(m->device));
    m->stream = st;
    const size_t fbytes = sizeof(gorio::MapFrame) * (size_t)count;
    GORIO_HIP_CHECK(map_fail, m->d_frames.reserve(fbytes, fbytes + fbytes / 2));
    GORIO_HIP_CHECK(map_fail, m->d_bcnt.reserve((size_t)nblocks + 1, (size_t)nblocks + 1 + (size_t)nblocks / 8));
    GORIO_HIP_CHECK(map_fail, m->d_stage.reserve((size_t)total, (size_t)total + (size_t)total / 8));
    GORIO_HIP_CHECK(map_fail, m->d_rec.reserve(sizeof(gorio::MapRecord)));
    const gorio::MapFrame* d_fr = static_cast<const gorio::MapFrame*>(m->d_frames.get());
    gorio::MapRecord* d_rec = static_cast<gorio::MapRecord*>(m->d_rec.get());
    const int cap = (int)std::min<size_t>(m->d_stage.cap(), (size_t)INT_MAX);
    GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(m->d_frames, fr.data(), fbytes, hipMemcpyHostToDevice, st));
    uploaded = (long long)fbytes;
    if (voxels) {
      rec0.anchor_rank = INT_MAX;
      for (int c = 0; c < 3; ++c) rec0.min_k[c] = INT_MAX, rec0.max_k[c] = INT_MIN;
      GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(d_rec, &rec0, sizeof(rec0), hipMemcpyHostToDevice, st));
      uploaded += (long long)sizeof(rec0);
    }
    const dim3 grid(max_blocks, count);
    gorio::map_gate_count_kernel<<<grid, 256, 0, st>>>(d_fr, m->d_bcnt);
    gorio::block_scan_kernel<<<1, 1024, 0, st>>>(m->d_bcnt, (int)nblocks);
    gorio::map_scatter_kernel<<<grid, 256, 0, st>>>(d_fr, m->d_bcnt, m->d_stage, cap, voxels ? d_rec : nullptr);
    if (voxels) {
      gorio::map_cells_kernel<<<(int)std::min<long long>(gorio::kMapCellBlocks, (total + 255) / 256), 256, 0, st>>>(m->d_stage, m->d_bcnt.get() + nblocks, cap, resolution, d_rec);
      GORIO_HIP_CHECK(map_fail, hipGetLastError());
      GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(&rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, st));  // THE read-back of stage A
      GORIO_HIP_CHECK(map_fail, hipStreamSynchronize(st));  // also covers the pageable frame table
      kept = rec.kept;
    } else {
      GORIO_HIP_CHECK(map_fail, hipGetLastError());
      GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(&kept, m->d_bcnt.get() + nblocks, sizeof(int), hipMemcpyDeviceToHost, st));
      GORIO_HIP_CHECK(map_fail, hipStreamSynchronize(st));
    }
    if (kept < 0 || kept > total) return map_fail(GORIO_ERR_NO_DEVICE, "generate: the device returned an impossible count");
  }
  info.n_kept = kept;
  n_out = kept;
  if (voxels) {
    n_out = 0;
    if (kept > 0 && rec.anchor_rank < kept) {  // there is a finite point
      if (rec.out_of_range) return map_fail(GORIO_ERR_UNSUPPORTED, "generate: a cell coordinate reaches 2^30 at this resolution");
      for (int c = 0; c < 3; ++c) {
        if (rec.min_k[c] > rec.max_k[c]) return map_fail(GORIO_ERR_NO_DEVICE, "generate: the device returned an impossible box");
        if ((long long)rec.max_k[c] - (long long)rec.min_k[c] + 1 >= (1ll << 21))
          return map_fail(GORIO_ERR_UNSUPPORTED, "generate: the occupied voxels span 2^21 cells or more on an axis at this resolution");
      }
      info.n_finite = rec.n_finite;
      lat.res = resolution;
      for (int c = 0; c < 3; ++c) {
        lat.a[c] = (double)rec.q0[c] - resolution / 2;
        lat.min_k[c] = rec.min_k[c];
        info.anchor[c] = lat.a[c];
        info.min_k[c] = rec.min_k[c];
        info.max_k[c] = rec.max_k[c];
      }
      const int npow2 = sort_padded_size(kept);
      const int vblocks = (kept + 255) / 256;  // <= nblocks: d_bcnt holds them
      GORIO_HIP_CHECK(map_fail, m->d_keys.reserve((size_t)npow2));
      gorio::map_key_kernel<<<npow2 / 256, 256, 0, st>>>(m->d_stage, kept, npow2, lat, m->d_keys);
      enqueue_tiled_sort(st, SortKeys{m->d_keys, npow2}, 1, npow2);
      gorio::cell_count_kernel<0, true><<<vblocks, 256, 0, st>>>(m->d_keys, kept, m->d_bcnt);
      gorio::block_scan_kernel<<<1, 1024, 0, st>>>(m->d_bcnt, vblocks);
      GORIO_HIP_CHECK(map_fail, hipGetLastError());
      GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(&n_out, m->d_bcnt.get() + vblocks, sizeof(int), hipMemcpyDeviceToHost, st));  // the voxel count
      GORIO_HIP_CHECK(map_fail, hipStreamSynchronize(st));
      if (n_out <= 0 || n_out > rec.n_finite) return map_fail(GORIO_ERR_NO_DEVICE, "generate: the device returned an impossible voxel count");
    }
    info.n_voxels = n_out;
  }
  // every check has passed: from here on the result held is replaced
  if (n_out > 0) {
    if (m->d_result.cap() < (size_t)n_out) {
      m->n_result = 0;
      m->info = gorio_map_info_t{};
    }
    GORIO_HIP_CHECK(map_fail, m->d_result.reserve((size_t)n_out, (size_t)n_out + (size_t)n_out / 8));
    if (voxels) {
      gorio::map_centre_kernel<<<(kept + 255) / 256, 256, 0, st>>>(m->d_keys, kept, m->d_bcnt, lat, m->d_result, n_out);
      GORIO_HIP_CHECK(map_fail, hipGetLastError());
    } else {
      GORIO_HIP_CHECK(map_fail, hipMemcpyAsync(m->d_result, m->d_stage, sizeof(float4) * (size_t)n_out, hipMemcpyDeviceToDevice, st));
    }
    GORIO_HIP_CHECK(map_fail, hipStreamSynchronize(st));
  }
  m->n_result = n_out;
  m->info = info;
  ++m->generates;
  m->bytes_uploaded += uploaded;
  *n_points = n_out;
  return GORIO_OK;
}

int gorio_map_get(gorio_map_t* m, float* xyz, float* intensity, int stride_bytes, int capacity) {
  if (!m) return map_fail(GORIO_ERR_INVALID, "get: null handle");
  if (stride_bytes < 4 || (stride_bytes % 4) != 0 || (xyz && stride_bytes < 12) || capacity < 0) return map_fail(GORIO_ERR_INVALID, "get: bad arguments");
  const int n = m->n_result;
  if (capacity < n) return map_fail(GORIO_ERR_INVALID, "get: capacity too small");
  if (n == 0 || (!xyz && !intensity)) return GORIO_OK;
  GORIO_HIP_CHECK(map_fail, hipSetDevice(m->device));
  // through two pinned chunks: the copy of the next chunk runs while this one is spread over the caller's strided arrays
  GORIO_HIP_CHECK(map_fail, m->h_get.reserve(2 * sizeof(float4) * (size_t)kMapGetChunk));
  float4* const stage = static_cast<float4*>(m->h_get.get());
  const size_t s = stride_bytes / 4;
  const int chunks = (n + kMapGetChunk - 1) / kMapGetChunk;
  auto enqueue = [&](int c) {
    const int first = c * kMapGetChunk, len = std::min(kMapGetChunk, n - first);
    return hipMemcpyAsync(stage + (size_t)(c & 1) * kMapGetChunk, m->d_result.get() + first, sizeof(float4) * (size_t)len, hipMemcpyDeviceToHost, m->stream);
  };
  GORIO_HIP_CHECK(map_fail, enqueue(0));
  for (int c = 0; c < chunks; ++c) {
    GORIO_HIP_CHECK(map_fail, hipStreamSynchronize(m->stream));  // chunk c has arrived; the other half is free
    if (c + 1 < chunks) GORIO_HIP_CHECK(map_fail, enqueue(c + 1));
    const float4* pts = stage + (size_t)(c & 1) * kMapGetChunk;
    const int first = c * kMapGetChunk, len = std::min(kMapGetChunk, n - first);
    for (int i = 0; i < len; ++i) {
      const size_t o = s * (size_t)(first + i);
      if (xyz) {
        xyz[o] = pts[i].x;
        xyz[o + 1] = pts[i].y;
        xyz[o + 2] = pts[i].z;
      }
      if (intensity) intensity[o] = pts[i].w;
    }
  }
  m->points_downloaded += n;
  return GORIO_OK;
}

int gorio_map_info(const gorio_map_t* m, gorio_map_info_t* out) {
  if (!m || !out) return map_fail(GORIO_ERR_INVALID, "info: null argument");
  *out = m->info;
  return GORIO_OK;
}

int gorio_map_get_counters(const gorio_map_t* m, long long* generates, long long* points_downloaded, long long* bytes_uploaded) {
  if (!m) return map_fail(GORIO_ERR_INVALID, "get_counters: null handle");
  if (generates) *generates = m->generates;
  if (points_downloaded) *points_downloaded = m->points_downloaded;
  if (bytes_uploaded) *bytes_uploaded = m->bytes_uploaded;
  return GORIO_OK;
}

int gorio_map_get_capacities(const gorio_map_t* m, long long* capacities) {
  if (!m || !capacities) return map_fail(GORIO_ERR_INVALID, "get_capacities: null argument");
  capacities[0] = (long long)m->d_frames.cap();
  capacities[1] = (long long)m->d_bcnt.cap();
  capacities[2] = (long long)m->d_stage.cap();
  capacities[3] = (long long)m->d_keys.cap();
  capacities[4] = (long long)m->d_result.cap();
  capacities[5] = (long long)m->d_rec.cap();
  return GORIO_OK;
}

}  // extern "C"
