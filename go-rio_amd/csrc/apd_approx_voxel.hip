// apd_approx_voxel.hip -- pcl::ApproximateVoxelGrid on the device.  Included by apd_api.hip after apd_submap.hip (it reuses block_scan_kernel of
// apd_voxel_group.hip).
//
// PCL is not in the image: the definition below is RECALLED from PCL 1.10 filters/impl/approximate_voxel_grid.hpp (parity: as recalled,
// unpinned), and it is what tests/approx_voxel_restatement.py restates.
//
// A point is a row of F float fields, 3 <= F <= 8, the first three x, y, z (downsample_all_data_ = true averages all fields alike; F = 3 is
// downsample_all_data_ = false).
//   inv[a]  = 1.0f / (float)leaf[a]                                   float division, one leaf per axis
//   cell    c[a] = (int)floorf(p[a] * inv[a])                         float product
//   bucket  h = (uint32)(c0 * 7171 + c1 * 3079 + c2 * 4231) & 511     32-bit wrap (the reference's signed overflow, as it behaves); histsize_ = 512
//   history 512 entries (count, cell, float sum[F]), empty at the start.  For each point in input order: an entry of its bucket that holds
//           ANOTHER cell is flushed (sum[f] / (float)count appended to the output) and emptied; then count++, sum[f] = sum[f] + p[f].
//   after the last point every non-empty entry is flushed in ascending bucket order.
// Deviation: the reference converts NaN to int.  Here a cloud with a non-finite coordinate, or a cell coordinate outside (-2^30, 2^30), is
// refused (n_out = -1, nothing written).  Non-finite values in the other fields are averaged as given.
//
// The parallel form (bit for bit the sequential loop, order included):
//   1. points are ordered stably by bucket: a 512-bin counting sort over kAvgWaves chunks of the input, one wave per chunk
//        avg_hist_kernel         cells with the refusal flag, buckets, one histogram per chunk
//        avg_bucket_scan_kernel  chunk offsets inside every bucket, bucket starts, rank of every non-empty bucket among the non-empty ones
//        avg_scatter_kernel      (cell, input index) at the sorted position; equal buckets of one 64-point tile keep their lane order
//   2. inside a bucket a RUN starts where the cell differs from its predecessor's; a run is one output point
//        avg_flag_kernel         0 = inside a run, 1 = first run of its bucket, 2 = a later run: its first point EVICTS the run before it
//   3. an evicted run is put out when its evictor arrives: its position is the number of evicting points with a smaller input index
//        avg_count_kernel + block_scan_kernel + avg_rank_kernel   exclusive prefix sum of the evictor flags in input order; n_out
//      the last run of every bucket follows all evicted runs, in ascending bucket order
//   4. avg_accumulate_kernel     float sums strictly in input order, the division, the store at the run's position
// Eight launches whatever n is; the host reads back n_out (4 bytes) and nothing else.
//
// The sum of a run cannot be reassociated, and a cloud inside one cell is ONE run of n points.  avg_accumulate_kernel gives every 64 sorted
// positions to a wave: each lane gathers its own point (independent loads), runs that end inside the tile are summed lane-parallel out
// of registers, and the one run that can leave the tile (its last) is continued by the WHOLE wave: 256 positions are gathered per round
// with independent loads, and the adds are taken in order from registers (v_readlane).  No lane ever walks a chain of dependent loads.
#include <hip/hip_runtime.h>

namespace gorio {

constexpr int kAvgBuckets = 512;   // histsize_
constexpr int kAvgWaves = 256;     // chunks of the counting sort
constexpr int kAvgMaxFields = 8;
constexpr int kAvgMaxPoints = 1 << 28;
enum { kAvgMetaRefused = 0, kAvgMetaFinal = 1, kAvgMetaNOut = 2, kAvgMetaInts = 4 };

struct AvgCols {  // field f of point i is c[f][i * stride]
  const float* c[kAvgMaxFields];
  int stride;
};
struct AvgColsOut {
  float* c[kAvgMaxFields];
  int stride;
};
struct AvgGrid {
  float inv[3];
};

__device__ inline int avg_bucket(int c0, int c1, int c2) { return (int)(((unsigned)c0 * 7171u + (unsigned)c1 * 3079u + (unsigned)c2 * 4231u) & (unsigned)(kAvgBuckets - 1)); }

// the cell of point i; false when a coordinate is not finite or a cell coordinate leaves (-2^30, 2^30)
__device__ inline bool avg_cell(const AvgCols& in, int i, const AvgGrid& g, int c[3]) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float fl = floorf(in.c[a][(size_t)i * in.stride] * g.inv[a]);
    ok = ok && fabsf(fl) < 1073741824.0f;
    c[a] = (int)fl;
  }
  return ok;
}

// grid kAvgWaves / 4, block 256: wave w of the grid owns points [w chunk, (w + 1) chunk); chunk is a multiple of 64
__global__ __launch_bounds__(256) void avg_hist_kernel(AvgCols in, int n, int chunk, AvgGrid g, int* __restrict__ hist, int* __restrict__ evflag, int* __restrict__ meta) {
  __shared__ int sh[4][kAvgBuckets];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = lane; k < kAvgBuckets; k += 64) sh[wv][k] = 0;
  __syncthreads();
  const int gw = blockIdx.x * 4 + wv;
  const int begin = gw * chunk;
  bool bad = false;
  for (int t = 0; t < chunk; t += 64) {
    const int i = begin + t + lane;
    if (i < n) {
      int c[3];
      if (!avg_cell(in, i, g, c)) bad = true;
      atomicAdd(&sh[wv][avg_bucket(c[0], c[1], c[2])], 1);
      evflag[i] = 0;
    }
  }
  if (bad) atomicOr(meta + kAvgMetaRefused, 1);
  __syncthreads();
  for (int k = lane; k < kAvgBuckets; k += 64) hist[gw * kAvgBuckets + k] = sh[wv][k];
}

// one block of 512: hist[w][b] becomes the number of points of bucket b in the chunks before w; bstart[b] the bucket's first sorted
// position; finrank[b] the number of non-empty buckets below b, their total in meta
__global__ __launch_bounds__(kAvgBuckets) void avg_bucket_scan_kernel(int* __restrict__ hist, int* __restrict__ bstart, int* __restrict__ finrank, int* __restrict__ meta) {
  if (meta[kAvgMetaRefused]) return;
  __shared__ int s[kAvgBuckets], f[kAvgBuckets];
  const int b = threadIdx.x;
  int total = 0;
  for (int w = 0; w < kAvgWaves; ++w) {
    const int v = hist[w * kAvgBuckets + b];
    hist[w * kAvgBuckets + b] = total;
    total += v;
  }
  s[b] = total;
  f[b] = total > 0;
  __syncthreads();
  for (int off = 1; off < kAvgBuckets; off <<= 1) {
    const int ts = b >= off ? s[b - off] : 0, tf = b >= off ? f[b - off] : 0;
    __syncthreads();
    s[b] += ts;
    f[b] += tf;
    __syncthreads();
  }
  bstart[b] = s[b] - total;
  finrank[b] = f[b] - (total > 0);
  if (b == kAvgBuckets - 1) meta[kAvgMetaFinal] = f[b];
}

// grid and block of avg_hist_kernel: scell[sorted position] = (cell, input index), stable inside every bucket
__global__ __launch_bounds__(256) void avg_scatter_kernel(AvgCols in, int n, int chunk, AvgGrid g, const int* __restrict__ hist, const int* __restrict__ bstart,
                                                          const int* __restrict__ meta, int4* __restrict__ scell) {
  if (meta[kAvgMetaRefused]) return;
  __shared__ int off[4][kAvgBuckets];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int gw = blockIdx.x * 4 + wv;
  for (int k = lane; k < kAvgBuckets; k += 64) off[wv][k] = hist[gw * kAvgBuckets + k] + bstart[k];
  __syncthreads();
  const int begin = gw * chunk;
  for (int t = 0; t < chunk; t += 64) {  // the same trip count in every wave of the block
    const int i = begin + t + lane;
    const bool valid = i < n;
    int c[3] = {0, 0, 0};
    if (valid) avg_cell(in, i, g, c);
    const int b = avg_bucket(c[0], c[1], c[2]);
    unsigned long long peers = __ballot(valid);  // the lanes of this tile in my bucket
#pragma unroll
    for (int bit = 0; bit < 9; ++bit) {
      const bool one = (b >> bit) & 1;
      const unsigned long long bal = __ballot(valid && one);
      peers &= one ? bal : ~bal;
    }
    const int rank = __builtin_popcountll(peers & ((1ull << lane) - 1ull));
    const int base = valid ? off[wv][b] : 0;
    __syncthreads();
    if (valid) {
      scell[base + rank] = make_int4(c[0], c[1], c[2], i);
      if (rank == __builtin_popcountll(peers) - 1) off[wv][b] = base + rank + 1;
    }
    __syncthreads();
  }
}

// grid ceil(n / 256): the run flags by sorted position, and evflag[i] = 1 for every point i that evicts a run
__global__ __launch_bounds__(256) void avg_flag_kernel(const int4* __restrict__ scell, int n, const int* __restrict__ meta, unsigned char* __restrict__ sflag,
                                                       int* __restrict__ evflag) {
  if (meta[kAvgMetaRefused]) return;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const int4 c = scell[p];
  int flag = 1;
  if (p > 0) {
    const int4 q = scell[p - 1];
    if (q.x == c.x && q.y == c.y && q.z == c.z) flag = 0;
    else if (avg_bucket(q.x, q.y, q.z) == avg_bucket(c.x, c.y, c.z)) {
      flag = 2;
      evflag[c.w] = 1;
    }
  }
  sflag[p] = (unsigned char)flag;
}

// evictors per 256 points of the input -> counts[block]
__global__ __launch_bounds__(256) void avg_count_kernel(const int* __restrict__ evflag, int n, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long m = __ballot(i < n && evflag[i] != 0);
  __shared__ int sw[4];
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = __builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// evflag[i] becomes the number of evictors below i (in place); n_out = evictors + non-empty buckets, or -1 for a refused cloud
__global__ __launch_bounds__(256) void avg_rank_kernel(int* __restrict__ evflag, int n, const int* __restrict__ offsets, int nblocks, int* __restrict__ meta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(i < n && evflag[i] != 0);
  __shared__ int sw[4];
  if (lane == 0) sw[wv] = __builtin_popcountll(m);
  __syncthreads();
  int rank = offsets[blockIdx.x] + __builtin_popcountll(m & ((1ull << lane) - 1ull));
  for (int q = 0; q < wv; ++q) rank += sw[q];
  if (i < n) evflag[i] = rank;
  if (blockIdx.x == 0 && threadIdx.x == 0) meta[kAvgMetaNOut] = meta[kAvgMetaRefused] ? -1 : offsets[nblocks] + meta[kAvgMetaFinal];
}

__device__ inline float avg_readlane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }

// grid ceil(n / 256), block 256: one wave per 64 sorted positions (header comment)
template <int F>
__global__ __launch_bounds__(256) void avg_accumulate_kernel(AvgCols in, int n, const int4* __restrict__ scell, const unsigned char* __restrict__ sflag,
                                                             const int* __restrict__ evrank, const int* __restrict__ finrank, const int* __restrict__ meta, AvgColsOut out,
                                                             int capacity) {
  const int n_out = meta[kAvgMetaNOut];
  if (n_out < 0 || n_out > capacity) return;  // refused, or the output does not fit: nothing is written
  const int nev = n_out - meta[kAvgMetaFinal];
  const int lane = threadIdx.x & 63;
  const int base = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  if (base >= n) return;
  const int p = base + lane;
  const bool valid = p < n;
  const int4 c = valid ? scell[p] : make_int4(0, 0, 0, 0);
  const int fl = valid ? (int)sflag[p] : 0;
  float v[F];
#pragma unroll
  for (int f = 0; f < F; ++f) v[f] = valid ? in.c[f][(size_t)c.w * in.stride] : 0.0f;
  const unsigned long long m = __ballot(fl != 0);
  if (m == 0) return;  // the whole tile lies inside a run that an earlier tile's wave sums
  const int nvalid = min(64, n - base);
  const unsigned long long higher = lane < 63 ? m >> (lane + 1) : 0ull;
  const int next = higher ? lane + 1 + __builtin_ctzll(higher) : nvalid;  // where my run ends inside the tile
  const int len = fl ? next - lane : 0;
  float acc[F];
#pragma unroll
  for (int f = 0; f < F; ++f) acc[f] = 0.0f;
  for (int k = 0; k < 64; ++k) {  // every lane that starts a run adds its points in order; the others ride along
    if (__ballot(k < len) == 0) break;
#pragma unroll
    for (int f = 0; f < F; ++f) {
      const float t = __shfl(v[f], (lane + k) & 63, 64);
      if (k < len) acc[f] = acc[f] + t;
    }
  }
  int cnt = len, end = base + next;
  const int tile_end = base + 64;
  if (tile_end < n && sflag[tile_end] == 0) {  // the tile's last run goes on: the whole wave continues it
    const int L = 63 - __builtin_clzll(m);
    float r[F];
#pragma unroll
    for (int f = 0; f < F; ++f) r[f] = __shfl(acc[f], L, 64);
    int rcnt = __shfl(len, L, 64);
    int e = n;
    for (int cb = tile_end; cb < n; cb += 256) {
      int fu[4];
      float w[4][F];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = cb + u * 64 + lane;
        const bool ok = q < n;
        fu[u] = ok ? (int)sflag[q] : 1;  // the end of the cloud ends the run like a start
        const int idx = ok ? scell[q].w : 0;
#pragma unroll
        for (int f = 0; f < F; ++f) w[u][f] = ok ? in.c[f][(size_t)idx * in.stride] : 0.0f;
      }
      bool done = false;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (done) break;
        const unsigned long long mm = __ballot(fu[u] != 0);
        const int take = mm ? __builtin_ctzll(mm) : 64;
        for (int k = 0; k < take; ++k) {
#pragma unroll
          for (int f = 0; f < F; ++f) r[f] = r[f] + avg_readlane(w[u][f], k);
        }
        rcnt += take;
        if (mm) {
          e = cb + u * 64 + take;
          done = true;
        }
      }
      if (done) break;
    }
    if (lane == L) {
#pragma unroll
      for (int f = 0; f < F; ++f) acc[f] = r[f];
      cnt = rcnt;
      end = e;
    }
  }
  if (!fl) return;
  const bool evicted = end < n && sflag[end] == 2;
  const int pos = evicted ? evrank[scell[end].w] : nev + finrank[avg_bucket(c.x, c.y, c.z)];
  if (pos < 0 || pos >= capacity) return;
  const float d = (float)cnt;
#pragma unroll
  for (int f = 0; f < F; ++f) out.c[f][(size_t)pos * out.stride] = acc[f] / d;
}

// ---- host: the scratch of one filter call and the launches.  Every buffer is a DevBuf; the first five grow together (capacity `cap`).
struct AvgScratch {
  DevBuf<int4> scell;
  DevBuf<unsigned char> sflag;
  DevBuf<int> evflag, counts;
  size_t cap = 0;
  DevBuf<int> tables;  // hist[kAvgWaves][512], bstart[512], finrank[512], meta[kAvgMetaInts]
  DevBuf<float> stage_in, stage_out;  // the host-pointer form's columns
  void reset() {
    scell.reset(), sflag.reset(), evflag.reset(), counts.reset(), tables.reset(), stage_in.reset(), stage_out.reset();
    cap = 0;
  }
};

// Enqueues the filter of n points (0 < n <= kAvgMaxPoints) with n_fields fields on `stream`.  *d_n_out is where n_out (or -1: refused)
// will stand on the device.
inline hipError_t avg_enqueue(hipStream_t stream, AvgScratch& w, const AvgCols& in, int n, int n_fields, const float leaf[3], const AvgColsOut& out, int capacity,
                              const int** d_n_out) {
  const size_t grown = (size_t)n + (size_t)n / 8;
  hipError_t e = reserve_group(w.cap, n, grown, w.scell, grown, w.sflag, grown, w.evflag, grown, w.counts, grown / 256 + 2);
  if (e != hipSuccess) return e;
  constexpr size_t kTables = (size_t)kAvgWaves * kAvgBuckets + 2 * kAvgBuckets + kAvgMetaInts;
  e = w.tables.reserve(kTables);
  if (e != hipSuccess) return e;
  int* hist = w.tables;
  int* bstart = hist + (size_t)kAvgWaves * kAvgBuckets;
  int* finrank = bstart + kAvgBuckets;
  int* meta = finrank + kAvgBuckets;
  AvgGrid g;
  for (int a = 0; a < 3; ++a) g.inv[a] = 1.0f / leaf[a];
  const int chunk = ((n + kAvgWaves - 1) / kAvgWaves + 63) / 64 * 64;
  const int nblocks = (n + 255) / 256;
  e = hipMemsetAsync(meta, 0, sizeof(int) * kAvgMetaInts, stream);
  if (e != hipSuccess) return e;
  avg_hist_kernel<<<kAvgWaves / 4, 256, 0, stream>>>(in, n, chunk, g, hist, w.evflag, meta);
  avg_bucket_scan_kernel<<<1, kAvgBuckets, 0, stream>>>(hist, bstart, finrank, meta);
  avg_scatter_kernel<<<kAvgWaves / 4, 256, 0, stream>>>(in, n, chunk, g, hist, bstart, meta, w.scell);
  avg_flag_kernel<<<nblocks, 256, 0, stream>>>(w.scell, n, meta, w.sflag, w.evflag);
  avg_count_kernel<<<nblocks, 256, 0, stream>>>(w.evflag, n, w.counts);
  block_scan_kernel<<<1, 1024, 0, stream>>>(w.counts, nblocks);
  avg_rank_kernel<<<nblocks, 256, 0, stream>>>(w.evflag, n, w.counts, nblocks, meta);
  switch (n_fields) {
#define GORIO_AVG_CASE(F) \
  case F: avg_accumulate_kernel<F><<<nblocks, 256, 0, stream>>>(in, n, w.scell, w.sflag, w.evflag, finrank, meta, out, capacity); break;
    GORIO_AVG_CASE(3) GORIO_AVG_CASE(4) GORIO_AVG_CASE(5) GORIO_AVG_CASE(6) GORIO_AVG_CASE(7) GORIO_AVG_CASE(8)
#undef GORIO_AVG_CASE
    default: return hipErrorInvalidValue;
  }
  *d_n_out = meta + kAvgMetaNOut;
  return hipGetLastError();
}

}  // namespace gorio
