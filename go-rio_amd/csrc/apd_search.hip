// apd_search.hip -- exact batched k-NN and radius queries of ARBITRARY query points against a cloud that lives on the device
// (include/gorio_search.h).  Kernels first, the host side below them.  Included at the end of apd_api.hip: the cloud and its index are a
// DevCloud, built by run_index_build and shared with registration handles and keyframe stores by the DevCloud's shared_ptr.
//
//   search_finite_kernel         is every point of a device cloud finite (a non-finite cloud is refused)
//   search_query_keys_kernel     Morton keys of the queries in the CLOUD's bounding-box frame (clamped: a query outside the box takes
//                                the code of the nearest cell), sorted by enqueue_tiled_sort: the 64 queries of a wave are spatial
//                                neighbours, so the wave-uniform box tests prune.  Self queries take the index order as it is.
//   search_knn_kernel            k-NN: one wave per workgroup, one lane per query, the scalar-load tile walk of sor_mean_distance_kernel
//   search_radius_kernel<MODE>   radius: count pass / fill pass, the tile walk of radius_neighbours_kernel
//   search_scan_kernel           exclusive scans of the found and the kept counts, one workgroup
//   search_segment_sort_kernel   sorts every segment of at most kSegLdsMax keys inside LDS and emits its kept part
//   search_long_*_kernel         long segments: into padded slots, enqueue_tiled_sort over all of them at once, emit
//   search_*_batch_kernel        the radius kernels once more over a JOB TABLE (search_radius_batch_core, gorio_search_radius_batch): every
//                                kernel above keeps its body in a __device__ per-workgroup function that its batched twin calls too
//
// Exactness is the argument of apd_index.hip: the lower bound of a box is evaluated with the float expression of a point distance, so
// bound <= distance holds in float arithmetic and a tile is skipped only when no point of it can enter the result.  The k-NN list holds
// 64-bit keys (float bits of d) << 32 | original index (non-negative float bits order as unsigned integers), a TOTAL order: whatever
// order the tiles are visited in, the list ends as the k smallest keys, i.e. ties go to the lowest original index.  A tile whose bound
// EQUALS the k-th distance is therefore still visited (it may hold an equal distance with a lower index).
#include <hip/hip_runtime.h>

#include "search_plan.h"

namespace gorio {

static_assert(search_plan::kSortTileKeys == kSortTile, "search_plan.h sizes the slots of long segments by the tile of the tiled sort");

// where the queries of a call come from
struct SearchQueries {
  const float* q;                  // device: the first x; null = the cloud's own points (sorted position p is query orig[p])
  const unsigned long long* keys;  // [>= nq] sorted (Morton code << 31 | query index); unused for self queries
  int stride_f;                    // floats between queries
  int nq;
};

__global__ __launch_bounds__(256) void search_finite_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, int* __restrict__ flag) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (!(isfinite(x[i]) && isfinite(y[i]) && isfinite(z[i]))) *flag = 1;  // every writer stores the same value
}

// grid: ceil(npow2 / 256), block 256.  bb: the cloud's bounding box as run_index_build left it (ordered encodings, IndexJob::bb).
// A non-finite query takes the largest code: such queries gather at the tail of the order, before the padding keys (~0).
__device__ __forceinline__ void search_query_key(const float* __restrict__ q, int stride_f, int nq, int npow2, const unsigned int* __restrict__ bb,
                                                 unsigned long long* __restrict__ keys, int i) {
  if (i >= npow2) return;
  if (i >= nq) {
    keys[i] = ~0ull;
    return;
  }
  float ext = 1e-6f, lo[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = ord2f(bb[a]);
    ext = fmaxf(ext, ord2f(bb[3 + a]) - lo[a]);
  }
  const float* p = q + (size_t)i * stride_f;
  const float v[3] = {p[0], p[1], p[2]};
  unsigned long long code = (1ull << 33) - 1;
  if (isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2])) {
    unsigned int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float t = (v[a] - lo[a]) / ext * 2047.0f;
      t = fminf(fmaxf(t, 0.0f), 2047.0f);
      c[a] = (unsigned int)t;
    }
    code = spread11(c[0]) | (spread11(c[1]) << 1) | (spread11(c[2]) << 2);
  }
  keys[i] = (code << 31) | (unsigned long long)i;
}
__global__ __launch_bounds__(256) void search_query_keys_kernel(const float* __restrict__ q, int stride_f, int nq, int npow2, const unsigned int* __restrict__ bb,
                                                                unsigned long long* __restrict__ keys) {
  search_query_key(q, stride_f, nq, npow2, bb, keys, blockIdx.x * 256 + threadIdx.x);
}

// the query of sorted position p.  exists: p is a query of the call; live: it is one with finite coordinates (the cloud's own points
// always are).  A query that is not live gets coordinates 0: it takes part in no bound and no result, and no NaN enters the arithmetic.
struct LaneQuery {
  float x, y, z;
  int qi;  // original query index
  bool exists, live;
};
__device__ __forceinline__ LaneQuery load_query(const SearchIndex& si, const SearchQueries& sq, int p) {
  LaneQuery r{0.f, 0.f, 0.f, 0, false, false};
  if (!sq.q) {
    if (p < si.n) {
      const float4 v = si.s4[p];
      r.x = v.x, r.y = v.y, r.z = v.z;
      r.qi = __float_as_int(v.w);
      r.exists = r.live = true;
    }
  } else if (p < sq.nq) {
    r.qi = (int)(sq.keys[p] & 0x7fffffffull);
    const float* s = sq.q + (size_t)r.qi * sq.stride_f;
    const float x = s[0], y = s[1], z = s[2];
    r.exists = true;
    r.live = isfinite(x) && isfinite(y) && isfinite(z);
    if (r.live) r.x = x, r.y = y, r.z = z;
  }
  return r;
}

// box of the wave's LIVE queries (lo = +inf, hi = -inf without one: every box bound is then +inf)
__device__ __forceinline__ void wave_query_box(const LaneQuery& q, float (&qlo)[3], float (&qhi)[3]) {
  qlo[0] = wave_min(q.live ? q.x : INFINITY), qlo[1] = wave_min(q.live ? q.y : INFINITY), qlo[2] = wave_min(q.live ? q.z : INFINITY);
  qhi[0] = wave_max(q.live ? q.x : -INFINITY), qhi[1] = wave_max(q.live ? q.y : -INFINITY), qhi[2] = wave_max(q.live ? q.z : -INFINITY);
}

// the 64-tile group a cross-query wave starts its walk in: the group of the super tile (512 points) whose box is nearest to the wave's
// query box, so that the k-th distances are small before the far groups are tested.  Any group is a valid start.
__device__ __forceinline__ int home_group(const SearchIndex& si, const float (&qlo)[3], const float (&qhi)[3], int lane) {
  const float4* __restrict__ sb4 = reinterpret_cast<const float4*>(si.sbox);
  unsigned long long best = ~0ull;
  for (int s0 = 0; s0 < si.n_super; s0 += 64) {
    const int s = s0 + lane;
    if (s < si.n_super) {
      const float b = box_box_bound(qlo, qhi, sb4[2 * (size_t)s], sb4[2 * (size_t)s + 1]);
      const unsigned long long key = ((unsigned long long)__float_as_uint(b) << 32) | (unsigned int)s;
      best = key < best ? key : best;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o < best ? o : best;
  }
  const int s = (int)(best & 0xffffffffull);
  return __builtin_amdgcn_readfirstlane(s < si.n_super ? s / 4 : 0);
}

// ---- k-NN.  grid: ceil(queries / 64) (self queries: ceil(n / 64)), block 64.
// The per-lane list is ascending in 64-bit keys; a candidate c enters by K[t] = max(K[t-1], min(K[t], c)) -- the median of the three,
// what knn_kth_kernel does on distances with v_med3_f32, here on (distance, index) keys.  ONE list length for every k <= 32: the 32 - k
// slots below the list proper hold key 0, which no candidate moves (the -inf padding of sor_mean_distance_kernel), so K[31] is the k-th
// smallest throughout.  Empty slots hold (+inf, -1), which is above every real key and is what an unused output slot holds.
constexpr unsigned long long kKnnEmpty = (0x7f800000ull << 32) | 0xffffffffull;
__global__ __launch_bounds__(64) void search_knn_kernel(SearchIndex si, SearchQueries sq, int k, int* __restrict__ idx_out, float* __restrict__ sqd_out, int* __restrict__ count_out) {
  constexpr int K = 32;
  const int lane = threadIdx.x;
  const int p = blockIdx.x * 64 + lane;
  const LaneQuery q = load_query(si, sq, p);
  float qlo[3], qhi[3];
  wave_query_box(q, qlo, qhi);
  const scalar_fp tx = as_scalar(si.sx);
  const scalar_fp ty = as_scalar(si.sy);
  const scalar_fp tz = as_scalar(si.sz);
  const scalar_ip to = (scalar_ip)si.orig;
  const float4* __restrict__ tb4 = reinterpret_cast<const float4*>(si.tbox);
  const int ng = (si.n_tiles + 63) / 64;
  const int g0 = sq.q ? home_group(si, qlo, qhi, lane) : blockIdx.x / 32;  // self: the group of this wave's own tiles
  unsigned long long L[K];
#pragma unroll
  for (int t = 0; t < K; ++t) L[t] = t < K - k ? 0ull : kKnnEmpty;
  for (int v = 0; v < 2 * ng; ++v) {
    const int off = (v + 1) >> 1;
    const int g = (v & 1) ? g0 - off : g0 + off;
    if (g < 0 || g >= ng) continue;
    const int tl = g * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (tl < si.n_tiles) {
      lo = tb4[2 * (size_t)tl];
      hi = tb4[2 * (size_t)tl + 1];
    }
    // the wave's bound: the largest k-th distance of its LIVE lanes (-inf without one: nothing is visited)
    const float wb = wave_max(q.live ? __uint_as_float((unsigned int)(L[K - 1] >> 32)) : -INFINITY);
    // (tl < n_tiles explicitly: past the last tile the bound is +inf, and +inf <= wb holds while a list is not full)
    unsigned long long mask = __ballot(tl < si.n_tiles && box_box_bound(qlo, qhi, lo, hi) <= wb);
    while (mask) {
      const int tlane = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float bx[8] = {lane_f(lo.x, tlane), lane_f(lo.y, tlane), lane_f(lo.z, tlane), 0.f, lane_f(hi.x, tlane), lane_f(hi.y, tlane), lane_f(hi.z, tlane), 0.f};
      const float kth = q.live ? __uint_as_float((unsigned int)(L[K - 1] >> 32)) : -INFINITY;
      if (__ballot(box_bound(q.x, q.y, q.z, bx) <= kth) == 0) continue;
      const int j0 = (g * 64 + tlane) * 32;
#pragma unroll 2
      for (int u = 0; u < 32; ++u) {
        const float d = sqdist3(q.x, q.y, q.z, tx[j0 + u], ty[j0 + u], tz[j0 + u]);
        const int o = to[j0 + u];
        // padding positions (original index 0x7fffffff) and lanes without a live query offer the largest key: it never enters
        const unsigned long long c = (o != 0x7fffffff && q.live) ? (((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)o) : ~0ull;
        if (__ballot(c < L[K - 1]) == 0) continue;
#pragma unroll
        for (int t = K - 1; t > 0; --t) {
          const unsigned long long m = c < L[t] ? c : L[t];
          L[t] = L[t - 1] > m ? L[t - 1] : m;
        }
        L[0] = c < L[0] ? c : L[0];
      }
    }
  }
  if (q.exists) {
    int cnt = 0;
    int* io = idx_out + (size_t)q.qi * k;
    float* so = sqd_out + (size_t)q.qi * k;
#pragma unroll
    for (int t = 0; t < K; ++t) {
      if (t >= K - k) {
        const int i = (int)(unsigned int)(L[t] & 0xffffffffull);
        io[t - (K - k)] = i;
        so[t - (K - k)] = __uint_as_float((unsigned int)(L[t] >> 32));
        cnt += i != -1 ? 1 : 0;
      }
    }
    if (count_out) count_out[q.qi] = cnt;
  }
}

// every query of a call against an EMPTY cloud: no neighbour
__global__ __launch_bounds__(256) void search_knn_empty_kernel(int nq, int k, int* __restrict__ idx_out, float* __restrict__ sqd_out, int* __restrict__ count_out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)nq * k) {
    idx_out[i] = -1;
    sqd_out[i] = INFINITY;
  }
  if (count_out && i < (size_t)nq) count_out[i] = 0;
}

// ---- radius.  MODE 0: found[query] = neighbours with d < r2; MODE 1: their keys to keys_out[found_offs[query] ...] in the order met.
// grid: ceil(queries / 64), block 64.
// The work of ONE wave (= one workgroup): queries [64 wave, 64 wave + 64) of the call.  search_radius_kernel runs it for a single call,
// search_radius_batch_kernel for a job of a batch: one body, one arithmetic, the same bits.
template <int MODE>
__device__ __forceinline__ void search_radius_wave(const SearchIndex& si, const SearchQueries& sq, float r2, int wave, int* __restrict__ found,
                                                   const long long* __restrict__ found_offs, unsigned long long* __restrict__ keys_out) {
  const int lane = threadIdx.x;
  const int p = wave * 64 + lane;
  const LaneQuery q = load_query(si, sq, p);
  float qlo[3], qhi[3];
  wave_query_box(q, qlo, qhi);
  const float r2q = q.live ? r2 : 0.0f;  // no distance is below 0
  const float wb = wave_max(r2q);
  const scalar_fp tx = as_scalar(si.sx);
  const scalar_fp ty = as_scalar(si.sy);
  const scalar_fp tz = as_scalar(si.sz);
  const scalar_ip to = (scalar_ip)si.orig;
  const float4* __restrict__ tb4 = reinterpret_cast<const float4*>(si.tbox);
  const int ng = (si.n_tiles + 63) / 64;
  int cnt = 0;
  unsigned long long* out = nullptr;
  if (MODE == 1 && q.exists) out = keys_out + found_offs[q.qi];
  for (int g = 0; g < ng; ++g) {
    const int tl = g * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (tl < si.n_tiles) {
      lo = tb4[2 * (size_t)tl];
      hi = tb4[2 * (size_t)tl + 1];
    }
    unsigned long long mask = __ballot(tl < si.n_tiles && box_box_bound(qlo, qhi, lo, hi) < wb);
    while (mask) {
      const int tlane = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float bx[8] = {lane_f(lo.x, tlane), lane_f(lo.y, tlane), lane_f(lo.z, tlane), 0.f, lane_f(hi.x, tlane), lane_f(hi.y, tlane), lane_f(hi.z, tlane), 0.f};
      if (__ballot(box_bound(q.x, q.y, q.z, bx) < r2q) == 0) continue;
      const int j0 = (g * 64 + tlane) * 32;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) {
        const float d = sqdist3(q.x, q.y, q.z, tx[j0 + u], ty[j0 + u], tz[j0 + u]);
        if (d < r2q) {  // padding points sit at 1e30: d = inf, and inf < r2 never holds
          if (MODE == 1) out[cnt] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)to[j0 + u];
          ++cnt;
        }
      }
    }
  }
  if (MODE == 0 && q.exists) found[q.qi] = cnt;
}
template <int MODE>
__global__ __launch_bounds__(64) void search_radius_kernel(SearchIndex si, SearchQueries sq, float r2, int* __restrict__ found, const long long* __restrict__ found_offs,
                                                           unsigned long long* __restrict__ keys_out) {
  search_radius_wave<MODE>(si, sq, r2, blockIdx.x, found, found_offs, keys_out);
}

// Exclusive scans of found[] and of kept[] = min(found, max_nn) (max_nn > 0), nq + 1 entries each; what
// search_plan::offsets_from_counts computes on the host.  ONE workgroup: a thread sums a contiguous share of the queries, the 1024 sums
// are scanned in LDS, the thread then writes its share.  grid: 1, block 1024.
__device__ __forceinline__ void search_scan_block(const int* __restrict__ found, int nq, int max_nn, long long* __restrict__ found_offs, long long* __restrict__ kept_offs) {
  __shared__ long long sf[2][1024], sk[2][1024];
  const int tid = threadIdx.x;
  const int share = (nq + 1023) / 1024;
  const long long b = (long long)tid * share;
  const long long e = b + share < nq ? b + share : nq;
  long long f = 0, k = 0;
  for (long long q = b; q < e; ++q) {
    const int c = found[q];
    f += c;
    k += (max_nn > 0 && c > max_nn) ? max_nn : c;
  }
  sf[0][tid] = f;
  sk[0][tid] = k;
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < 1024; off <<= 1, cur ^= 1) {
    sf[cur ^ 1][tid] = sf[cur][tid] + (tid >= off ? sf[cur][tid - off] : 0);
    sk[cur ^ 1][tid] = sk[cur][tid] + (tid >= off ? sk[cur][tid - off] : 0);
    __syncthreads();
  }
  long long of = sf[cur][tid] - f, ok = sk[cur][tid] - k;
  for (long long q = b; q < e; ++q) {
    const int c = found[q];
    const int kc = (max_nn > 0 && c > max_nn) ? max_nn : c;
    found_offs[q] = of;
    kept_offs[q] = ok;
    of += c;
    ok += kc;
  }
  if (tid == 1023) {
    found_offs[nq] = sf[cur][1023];
    kept_offs[nq] = sk[cur][1023];
  }
}
__global__ __launch_bounds__(1024) void search_scan_kernel(const int* __restrict__ found, int nq, int max_nn, long long* __restrict__ found_offs, long long* __restrict__ kept_offs) {
  search_scan_block(found, nq, max_nn, found_offs, kept_offs);
}

// One workgroup per query: a segment of 1 .. kSegLdsMax found keys is sorted ascending in LDS (bitonic, padded to a power of two with
// ~0) and its first kept keys are emitted as (index, distance).  Longer segments are left to the long path.  grid: nq, block 256.
__device__ __forceinline__ void search_segment_sort_block(const unsigned long long* __restrict__ keys, const long long* __restrict__ found_offs,
                                                          const long long* __restrict__ kept_offs, int* __restrict__ idx_out, float* __restrict__ sqd_out, int q) {
  __shared__ unsigned long long s[search_plan::kSegLdsMax];
  const int tid = threadIdx.x;
  const long long b = found_offs[q];
  const long long len64 = found_offs[q + 1] - b;
  if (len64 <= 0 || len64 > search_plan::kSegLdsMax) return;  // workgroup-uniform
  const int len = (int)len64;
  const long long ob = kept_offs[q];
  const int kept = (int)(kept_offs[q + 1] - ob);
  int m = 2;
  while (m < len) m <<= 1;
  for (int i = tid; i < m; i += 256) s[i] = i < len ? keys[b + i] : ~0ull;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < m / 2; t += 256) {
        const int lo = ((t / j) * 2 * j) + (t % j), hi = lo + j;
        unsigned long long a = s[lo], c = s[hi];
        cmpx(a, c, (lo & k) == 0);
        s[lo] = a;
        s[hi] = c;
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < kept; i += 256) {
    idx_out[ob + i] = (int)(unsigned int)(s[i] & 0xffffffffull);
    sqd_out[ob + i] = __uint_as_float((unsigned int)(s[i] >> 32));
  }
}
__global__ __launch_bounds__(256) void search_segment_sort_kernel(const unsigned long long* __restrict__ keys, const long long* __restrict__ found_offs,
                                                                  const long long* __restrict__ kept_offs, int* __restrict__ idx_out, float* __restrict__ sqd_out) {
  search_segment_sort_block(keys, found_offs, kept_offs, idx_out, sqd_out, blockIdx.x);
}

// long segments (search_plan::LongSeg): into their slots, padded with ~0.  grid: (blocks, segments), block 256
__device__ __forceinline__ void search_long_pad_seg(const search_plan::LongSeg& sg, const unsigned long long* __restrict__ keys, unsigned long long* __restrict__ slots) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < sg.npow2; i += gridDim.x * 256) slots[sg.slot + i] = i < sg.len ? keys[sg.src + i] : ~0ull;
}
__global__ __launch_bounds__(256) void search_long_pad_kernel(const search_plan::LongSeg* __restrict__ segs, const unsigned long long* __restrict__ keys,
                                                              unsigned long long* __restrict__ slots) {
  const search_plan::LongSeg sg = segs[blockIdx.y];
  search_long_pad_seg(sg, keys, slots);
}
// the key arrays enqueue_tiled_sort sorts: the slot of segment blockIdx.y
struct LongSegKeys {
  const search_plan::LongSeg* segs;
  unsigned long long* slots;
  __device__ SortKeys get() const { return SortKeys{slots + segs[blockIdx.y].slot, segs[blockIdx.y].npow2}; }
};
// grid: (blocks, segments), block 256
__device__ __forceinline__ void search_long_emit_seg(const search_plan::LongSeg& sg, const unsigned long long* __restrict__ slots, int* __restrict__ idx_out,
                                                     float* __restrict__ sqd_out) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < sg.kept; i += gridDim.x * 256) {
    const unsigned long long key = slots[sg.slot + i];
    idx_out[sg.out + i] = (int)(unsigned int)(key & 0xffffffffull);
    sqd_out[sg.out + i] = __uint_as_float((unsigned int)(key >> 32));
  }
}
__global__ __launch_bounds__(256) void search_long_emit_kernel(const search_plan::LongSeg* __restrict__ segs, const unsigned long long* __restrict__ slots, int* __restrict__ idx_out,
                                                               float* __restrict__ sqd_out) {
  const search_plan::LongSeg sg = segs[blockIdx.y];
  search_long_emit_seg(sg, slots, idx_out, sqd_out);
}

// ---- the batched radius search (search_radius_batch_core): the launches above once more, each over the jobs of a table.  A workgroup
// finds its job through tables that every lane reads at the same address, read through the scalar data path (load_uniform, scalar_ip): the
// job's record lands in SGPRs as the arguments of the single kernels do, and the bodies are the single kernels' bodies.
struct SearchJob {
  SearchIndex si;
  SearchQueries sq;
  const unsigned int* bb;      // the cloud's bounding box (query keys)
  unsigned long long* qkeys;   // [npow2] the job's own query keys (= sq.keys); null for self queries
  int* found;                  // [nq]
  long long* found_offs;       // [nq + 1] the job's part of the batch's shared found offsets
  long long* kept_offs;        // [nq + 1] the job's own
  unsigned long long* keys;    // the found keys, the job's own (set after the plan)
  int* ridx;                   // the result, the job's own (set after the plan)
  float* rsqd;
  float r2;
  int max_nn;
  int npow2;                   // size of the query-key segment (0: self queries)
  int nq;                      // 0: the job takes part in no launch (no query, or an empty cloud)
};
static_assert(sizeof(SearchJob) % 8 == 0, "the tables behind the job records are 8-byte aligned");

// *p through scalar loads: p must be the same in every lane of the wave
template <class T>
__device__ __forceinline__ T load_uniform(const T* p) {
  static_assert(sizeof(T) % 4 == 0 && std::is_trivially_copyable<T>::value, "words of a plain record");
  union U {
    T v;
    int w[sizeof(T) / 4];
    __device__ U() {}
  } u;
  const scalar_ip s = (scalar_ip) reinterpret_cast<const int*>(p);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); ++i) u.w[i] = s[i];
  return u.v;
}

// grid: the key segments' 256-key blocks added up (BatchLayout::key_items), block 256
__global__ __launch_bounds__(256) void search_query_keys_batch_kernel(const SearchJob* __restrict__ jobs, const int* __restrict__ key_first, const int* __restrict__ key_jobs,
                                                                      int nsegs) {
  const scalar_ip kf = (scalar_ip)key_first;
  const int sg = search_plan::job_of(kf, nsegs, (int)blockIdx.x);
  const SearchJob j = load_uniform(jobs + ((scalar_ip)key_jobs)[sg]);
  search_query_key(j.sq.q, j.sq.stride_f, j.sq.nq, j.npow2, j.bb, j.qkeys, (int)(blockIdx.x - kf[sg]) * 256 + (int)threadIdx.x);
}
// the key arrays of the one tiled sort over all jobs' query keys: segment blockIdx.y
struct BatchQueryKeys {
  const SearchJob* jobs;
  const int* key_jobs;
  __device__ SortKeys get() const {
    const SearchJob* j = jobs + ((scalar_ip)key_jobs)[blockIdx.y];
    return SortKeys{j->qkeys, j->npow2};
  }
};
// grid: the jobs' waves added up, block 64
template <int MODE>
__global__ __launch_bounds__(64) void search_radius_batch_kernel(const SearchJob* __restrict__ jobs, const search_plan::WaveRef* __restrict__ wave_tab) {
  const search_plan::WaveRef w = load_uniform(wave_tab + blockIdx.x);
  const SearchJob j = load_uniform(jobs + w.job);
  search_radius_wave<MODE>(j.si, j.sq, j.r2, w.wave, j.found, j.found_offs, j.keys);
}
// grid: the jobs, block 1024
__global__ __launch_bounds__(1024) void search_scan_batch_kernel(const SearchJob* __restrict__ jobs) {
  const SearchJob j = load_uniform(jobs + blockIdx.x);
  if (j.nq == 0) return;  // workgroup-uniform
  search_scan_block(j.found, j.nq, j.max_nn, j.found_offs, j.kept_offs);
}
// grid: the jobs' queries added up, block 256
__global__ __launch_bounds__(256) void search_segment_sort_batch_kernel(const SearchJob* __restrict__ jobs, const int* __restrict__ query_first, int count) {
  const scalar_ip qf = (scalar_ip)query_first;
  const int k = search_plan::job_of(qf, count, (int)blockIdx.x);
  const SearchJob j = load_uniform(jobs + k);
  search_segment_sort_block(j.keys, j.found_offs, j.kept_offs, j.ridx, j.rsqd, (int)blockIdx.x - qf[k]);
}
// grid: (blocks, segments), block 256
__global__ __launch_bounds__(256) void search_long_pad_batch_kernel(const SearchJob* __restrict__ jobs, const search_plan::BatchLongSeg* __restrict__ segs,
                                                                    unsigned long long* __restrict__ slots) {
  const search_plan::BatchLongSeg sg = load_uniform(segs + blockIdx.y);
  search_long_pad_seg(sg.seg, jobs[sg.job].keys, slots);
}
struct BatchLongSegKeys {
  const search_plan::BatchLongSeg* segs;
  unsigned long long* slots;
  __device__ SortKeys get() const { return SortKeys{slots + segs[blockIdx.y].seg.slot, segs[blockIdx.y].seg.npow2}; }
};
__global__ __launch_bounds__(256) void search_long_emit_batch_kernel(const SearchJob* __restrict__ jobs, const search_plan::BatchLongSeg* __restrict__ segs,
                                                                     const unsigned long long* __restrict__ slots) {
  const search_plan::BatchLongSeg sg = load_uniform(segs + blockIdx.y);
  search_long_emit_seg(sg.seg, slots, jobs[sg.job].ridx, jobs[sg.job].rsqd);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_search.h)

struct gorio_search_handle {
  int device = 0;
  gorio_apd* up = nullptr;  // a private registration handle: its SOURCE is the cloud held (own or shared), its stream the device's launch stream
  DevCloud* cloud = nullptr;  // set only by a search state that lives INSIDE a registration handle (apd_gicp_mp.hip): the cloud searched instead of up's source
  long long point_uploads = 0, index_builds = 0, result_downloads = 0;
  DevBuf<int> d_flag;
  // queries and k-NN results of the host forms
  DevBuf<float> d_q;
  DevBuf<unsigned long long> d_qkeys;
  DevBuf<int> d_idx, d_cnt;
  DevBuf<float> d_sqd;
  // radius: counts and offsets (one group of capacity rq_cap queries), the found keys, the slots of long segments, the result
  DevBuf<int> d_found;
  DevBuf<long long> d_found_offs, d_kept_offs;
  size_t rq_cap = 0;
  DevBuf<unsigned long long> d_keys, d_slots;
  DevBuf<search_plan::LongSeg> d_segs;
  DevBuf<int> d_ridx;
  DevBuf<float> d_rsqd;
  size_t r_cap = 0;  // entries d_ridx / d_rsqd hold
  bool r_valid = false;
  int r_nq = 0;
  std::vector<long long> r_offs;  // kept offsets of the result held, nq + 1
  // a batch this state LEADS (search_radius_batch_core): the job records and tables, the found offsets of all jobs, the merged long segments
  // (their slots are d_slots)
  DevBuf<unsigned char> b_tab;
  DevBuf<long long> b_found_offs;
  DevBuf<search_plan::BatchLongSeg> b_segs;
  gorio_apd::Pinned pin_tab, pin_segs;
  PinnedBuf b_h_offs;
};

namespace {
thread_local std::string g_search_err;
int search_fail(int code, const std::string& m) {
  g_search_err = m;
  return code;
}

// arguments of a query call, checked before anything touches the device.  The handle comes last: the argument rules hold without one.
int search_check_queries(const char* who, const gorio_search_handle* s, int nq, int stride_bytes) {
  if (nq < 0) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": nq must not be negative");
  if (stride_bytes < 12 || (stride_bytes % 4) != 0) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": stride_bytes must be a multiple of 4, at least 12");
  if (!s) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": null handle");
  return GORIO_OK;
}
int search_check_knn(const char* who, const gorio_search_handle* s, int nq, int stride_bytes, int k, const int* idx_out, const float* sqd_out) {
  if (k > GORIO_SEARCH_MAX_K) return search_fail(GORIO_ERR_UNSUPPORTED, std::string(who) + ": k must be at most 32");
  if (k < 1) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": k must be at least 1");
  if (!idx_out || !sqd_out) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": null output");
  return search_check_queries(who, s, nq, stride_bytes);
}
int search_check_radius(const char* who, const gorio_search_handle* s, int nq, int stride_bytes, double radius, int max_nn, const long long* total) {
  if (!(radius > 0.0) || !std::isfinite(radius)) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": radius must be finite and > 0");
  if (max_nn < 0) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": max_nn must not be negative");
  if (!total) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": null total");
  return search_check_queries(who, s, nq, stride_bytes);
}

DevCloud& search_cloud(gorio_search_handle* s) { return s->cloud ? *s->cloud : *s->up->src; }
int search_cloud_n(const gorio_search_handle* s) {
  const DevCloud& c = s->cloud ? *s->cloud : *s->up->src;
  return c.present ? c.n : 0;
}

// the index of `cloud` through `owner` (the handle whose launches and scratch build it), unless it is built already
int search_build_index(gorio_apd* owner, DevCloud* cloud, bool* built) {
  *built = !cloud->idx_valid;
  if (cloud->idx_valid) return GORIO_OK;
  std::vector<std::pair<gorio_apd*, DevCloud*>> one = {{owner, cloud}};
  const int rc = run_index_build(owner, one);
  if (rc) return search_fail(rc, owner->err);
  return GORIO_OK;
}

// 1 when the device cloud has a non-finite point, 0 when not, negative on an error
int search_device_cloud_nonfinite(gorio_search_handle* s, const float* x, const float* y, const float* z, int n) {
  gorio_apd* h = s->up;
  GORIO_HIP_CHECK(search_fail, s->d_flag.reserve(1));
  GORIO_HIP_CHECK(search_fail, hipMemsetAsync(s->d_flag, 0, sizeof(int), h->stream));
  search_finite_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(x, y, z, n, s->d_flag);
  GORIO_HIP_CHECK(search_fail, hipGetLastError());
  int flag = 0;
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(&flag, s->d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));
  return flag ? 1 : 0;
}

// a cloud of another owner becomes the cloud held: finite check, index through the owner, then the share itself
int search_share(gorio_search_handle* s, const char* who, gorio_apd* owner, const std::shared_ptr<DevCloud>& c) {
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  const int bad = search_device_cloud_nonfinite(s, c->x, c->y, c->z, c->n);
  if (bad < 0) return bad;
  if (bad) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": the cloud has a non-finite point");
  bool built = false;
  if (int rc = search_build_index(owner, c.get(), &built)) return rc;
  s->up->src = c;  // points and index: one copy on the device, alive until the last holder lets go of it
  return GORIO_OK;
}

// the queries of a call as the kernels see them: cross queries get their Morton keys made and sorted (d_q: device pointer)
int search_prepare_queries(gorio_search_handle* s, const float* d_q, int nq, int stride_bytes, SearchQueries* sq, int* waves) {
  gorio_apd* h = s->up;
  const DevCloud& c = search_cloud(s);
  if (!d_q) {
    *sq = SearchQueries{nullptr, nullptr, 0, c.n};
    *waves = (c.n + 63) / 64;
    return GORIO_OK;
  }
  const int npow2 = sort_padded_size(nq);
  GORIO_HIP_CHECK(search_fail, s->d_qkeys.reserve((size_t)npow2));
  search_query_keys_kernel<<<(npow2 + 255) / 256, 256, 0, h->stream>>>(d_q, stride_bytes / 4, nq, npow2, c.bb, s->d_qkeys);
  enqueue_tiled_sort(h->stream, SortKeys{s->d_qkeys, npow2}, 1, npow2);
  GORIO_HIP_CHECK(search_fail, hipGetLastError());
  *sq = SearchQueries{d_q, s->d_qkeys, stride_bytes / 4, nq};
  *waves = (nq + 63) / 64;
  return GORIO_OK;
}

// host queries -> packed device copy (12 bytes per query)
int search_upload_queries(gorio_search_handle* s, const float* q_xyz, int nq, int stride_bytes) {
  gorio_apd* h = s->up;
  std::vector<float> buf((size_t)nq * 3);
  const size_t st = stride_bytes / 4;
  for (int i = 0; i < nq; ++i) {
    const float* p = q_xyz + (size_t)i * st;
    buf[3 * (size_t)i] = p[0], buf[3 * (size_t)i + 1] = p[1], buf[3 * (size_t)i + 2] = p[2];
  }
  GORIO_HIP_CHECK(search_fail, s->d_q.reserve((size_t)nq * 3, search_plan::grown((size_t)nq * 3)));
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(s->d_q, buf.data(), sizeof(float) * 3 * (size_t)nq, hipMemcpyHostToDevice, h->stream));
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));  // buf is pageable
  return GORIO_OK;
}

int search_self_nq(const char* who, gorio_search_handle* s, const float* q, int nq) {
  if (!q && nq != search_cloud_n(s)) return search_fail(GORIO_ERR_INVALID, std::string(who) + ": with q_xyz == NULL nq must be the size of the cloud");
  return GORIO_OK;
}

// k-NN with device pointers throughout; enqueues only
int search_knn_core(gorio_search_handle* s, const float* d_q, int nq, int stride_bytes, int k, int* d_idx, float* d_sqd, int* d_cnt) {
  gorio_apd* h = s->up;
  if (nq == 0) return GORIO_OK;
  if (search_cloud_n(s) == 0) {
    search_knn_empty_kernel<<<(unsigned)(((size_t)nq * k + 255) / 256), 256, 0, h->stream>>>(nq, k, d_idx, d_sqd, d_cnt);
    GORIO_HIP_CHECK(search_fail, hipGetLastError());
    return GORIO_OK;
  }
  SearchQueries sq;
  int waves = 0;
  if (int rc = search_prepare_queries(s, d_q, nq, stride_bytes, &sq, &waves)) return rc;
  search_knn_kernel<<<waves, 64, 0, h->stream>>>(search_cloud(s).index_view(), sq, k, d_idx, d_sqd, d_cnt);
  GORIO_HIP_CHECK(search_fail, hipGetLastError());
  return GORIO_OK;
}

// radius with a device pointer for the queries: the whole pipeline; the CSR stays in d_ridx / d_rsqd, its offsets in r_offs
int search_radius_core(gorio_search_handle* s, const float* d_q, int nq, int stride_bytes, double radius, int max_nn, int* count_out, long long* total) {
  gorio_apd* h = s->up;
  *total = 0;
  if (nq == 0 || search_cloud_n(s) == 0) {
    s->r_offs.assign((size_t)nq + 1, 0);
    if (count_out) std::fill(count_out, count_out + nq, 0);
    s->r_nq = nq;
    s->r_valid = true;
    return GORIO_OK;
  }
  const float r2 = (float)(radius * radius);
  SearchQueries sq;
  int waves = 0;
  if (int rc = search_prepare_queries(s, d_q, nq, stride_bytes, &sq, &waves)) return rc;
  const size_t qcap = search_plan::grown((size_t)nq + 1);
  GORIO_HIP_CHECK(search_fail, reserve_group(s->rq_cap, (size_t)nq + 1, qcap, s->d_found, qcap, s->d_found_offs, qcap, s->d_kept_offs, qcap));
  const SearchIndex si = search_cloud(s).index_view();
  search_radius_kernel<0><<<waves, 64, 0, h->stream>>>(si, sq, r2, s->d_found, nullptr, nullptr);
  search_scan_kernel<<<1, 1024, 0, h->stream>>>(s->d_found, nq, max_nn, s->d_found_offs, s->d_kept_offs);
  GORIO_HIP_CHECK(search_fail, hipGetLastError());
  std::vector<long long> foffs((size_t)nq + 1);
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(foffs.data(), s->d_found_offs, sizeof(long long) * ((size_t)nq + 1), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));
  // ---- the plan: totals, which sort every segment takes, the slots of the long ones.  Nothing is allocated or filled before this check.
  if (foffs[nq] > search_plan::kMaxTotal) return search_fail(GORIO_ERR_UNSUPPORTED, "radius: more than 2^31 - 1 neighbours found");
  search_plan::Plan plan;
  if (!search_plan::make_plan(foffs.data(), nq, max_nn, plan)) return search_fail(GORIO_ERR_UNSUPPORTED, "radius: the neighbours found cannot be planned (more than 2^31 - 1, or a segment too long to sort)");
  std::vector<int> cnt((size_t)nq);
  std::vector<long long> koffs((size_t)nq + 1);
  for (int q = 0; q < nq; ++q) cnt[q] = (int)(foffs[q + 1] - foffs[q]);
  search_plan::offsets_from_counts(cnt.data(), nq, max_nn, foffs.data(), koffs.data());
  const size_t found = (size_t)plan.found_total, kept = (size_t)plan.kept_total;
  if (found > 0) {
    GORIO_HIP_CHECK(search_fail, s->d_keys.reserve(found, search_plan::grown(found)));
    s->r_valid = false;  // from here on the result held is being replaced; a call refused above has left it as it was
    GORIO_HIP_CHECK(search_fail, reserve_group(s->r_cap, kept, search_plan::grown(kept), s->d_ridx, search_plan::grown(kept), s->d_rsqd, search_plan::grown(kept)));
    search_radius_kernel<1><<<waves, 64, 0, h->stream>>>(si, sq, r2, nullptr, s->d_found_offs, s->d_keys);
    search_segment_sort_kernel<<<nq, 256, 0, h->stream>>>(s->d_keys, s->d_found_offs, s->d_kept_offs, s->d_ridx, s->d_rsqd);
    GORIO_HIP_CHECK(search_fail, hipGetLastError());
    if (!plan.long_segs.empty()) {
      const int nl = (int)plan.long_segs.size();
      GORIO_HIP_CHECK(search_fail, s->d_segs.reserve((size_t)nl, search_plan::grown((size_t)nl)));
      GORIO_HIP_CHECK(search_fail, s->d_slots.reserve((size_t)plan.slot_keys, search_plan::grown((size_t)plan.slot_keys)));
      GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(s->d_segs, plan.long_segs.data(), sizeof(search_plan::LongSeg) * (size_t)nl, hipMemcpyHostToDevice, h->stream));
      const dim3 grid((unsigned)std::min(64, (plan.max_pow2 + 255) / 256), (unsigned)nl);
      search_long_pad_kernel<<<grid, 256, 0, h->stream>>>(s->d_segs, s->d_keys, s->d_slots);
      enqueue_tiled_sort(h->stream, LongSegKeys{s->d_segs, s->d_slots}, nl, plan.max_pow2);
      search_long_emit_kernel<<<grid, 256, 0, h->stream>>>(s->d_segs, s->d_slots, s->d_ridx, s->d_rsqd);
      GORIO_HIP_CHECK(search_fail, hipGetLastError());
      GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));  // plan.long_segs is pageable
    }
  }
  if (count_out) {
    for (int q = 0; q < nq; ++q) count_out[q] = (int)(koffs[q + 1] - koffs[q]);
  }
  s->r_offs.swap(koffs);
  s->r_nq = nq;
  s->r_valid = true;
  *total = plan.kept_total;
  return GORIO_OK;
}

// ---- the batched radius search: `count` calls of search_radius_core, each against its own state, run by ONE set of launches on the stream
// of job 0.  Launches and synchronisations do not grow with count: query keys (one launch + one tiled sort over the jobs' segments), count,
// scan, ONE copy back of all found offsets + one synchronisation, fill, segment sort, and for the long segments of all jobs one table, one
// pad launch, one tiled sort, one emit launch.  Every job's result is bit for bit that of search_radius_core for it alone: the kernels run
// the single kernels' bodies over the job's own buffers.
struct SearchBatchJob {
  gorio_search_handle* s;
  const float* d_q;  // device; null = the cloud's own points
  int nq, stride_bytes;
  double radius;
  int max_nn;
  int* count_out;    // host, may be null
  long long total;   // out
};
struct SearchBatchStats {
  int launches = 0, syncs = 0;
};

int tiled_sort_launches(int max_pow2) {
  int n = 1;
  for (int k = 2 * kSortTile; k <= max_pow2; k <<= 1) {
    for (int j = k >> 1; j >= kSortTile; j >>= 1) ++n;
    ++n;
  }
  return n;
}

int search_upload_staged(hipStream_t stream, gorio_apd::Pinned& b, void* dst, const void* src, size_t bytes) {
  if (b.pending) {
    GORIO_HIP_CHECK(search_fail, hipEventSynchronize(b.ev));
    b.pending = false;
  }
  GORIO_HIP_CHECK(search_fail, b.buf.reserve(bytes, bytes + bytes / 2 + 256));
  if (!b.ev) GORIO_HIP_CHECK(search_fail, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
  std::memcpy(b.buf, src, bytes);
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(dst, b.buf, bytes, hipMemcpyHostToDevice, stream));
  GORIO_HIP_CHECK(search_fail, hipEventRecord(b.ev, stream));
  b.pending = true;
  return GORIO_OK;
}

int search_radius_batch_core(SearchBatchJob* jobs, int count, SearchBatchStats* stats) {
  SearchBatchStats st;
  for (int j = 0; j < count; ++j) jobs[j].total = 0;
  if (count <= 0) return GORIO_OK;
  gorio_search_handle* lead = jobs[0].s;
  hipStream_t stream = lead->up->stream;
  // ---- the layout: which job owns which wave, query, offset and key segment
  std::vector<search_plan::BatchJobShape> shapes((size_t)count);
  for (int j = 0; j < count; ++j) shapes[j] = search_plan::BatchJobShape{jobs[j].nq, jobs[j].d_q == nullptr, jobs[j].nq > 0 && search_cloud_n(jobs[j].s) > 0};
  search_plan::BatchLayout lay;
  if (!search_plan::make_batch_layout(shapes.data(), count, lay)) return search_fail(GORIO_ERR_INVALID, "radius_batch: too many queries in one batch");
  const int n_waves = lay.wave_first[count], n_queries = lay.query_first[count], n_segs = (int)lay.key_jobs.size();
  const size_t n_offs = (size_t)lay.offs_first[count];
  std::vector<search_plan::Plan> plans((size_t)count);
  std::vector<std::vector<long long>> koffs((size_t)count);
  if (n_waves > 0) {
    // ---- the table: job records, wave table, query_first, key_first, key_jobs
    const size_t o_wave = sizeof(SearchJob) * (size_t)count, o_qf = o_wave + sizeof(search_plan::WaveRef) * (size_t)n_waves, o_kf = o_qf + sizeof(int) * ((size_t)count + 1),
                 o_kj = o_kf + sizeof(int) * ((size_t)n_segs + 1), tab_bytes = o_kj + sizeof(int) * (size_t)n_segs;
    GORIO_HIP_CHECK(search_fail, lead->b_tab.reserve(tab_bytes, tab_bytes + tab_bytes / 4 + 256));
    GORIO_HIP_CHECK(search_fail, lead->b_found_offs.reserve(n_offs, search_plan::grown(n_offs)));
    GORIO_HIP_CHECK(search_fail, lead->b_h_offs.reserve(sizeof(long long) * n_offs, sizeof(long long) * search_plan::grown(n_offs)));
    std::vector<unsigned char> tab(tab_bytes);
    SearchJob* const rec = reinterpret_cast<SearchJob*>(tab.data());
    std::memset(tab.data(), 0, tab_bytes);
    for (int j = 0; j < count; ++j) {
      if (!shapes[j].active) continue;
      gorio_search_handle* s = jobs[j].s;
      const int nq = jobs[j].nq;
      const DevCloud& c = search_cloud(s);
      SearchJob& r = rec[j];
      r.si = c.index_view();
      if (shapes[j].self) {
        r.sq = SearchQueries{nullptr, nullptr, 0, c.n};
      } else {
        r.npow2 = search_plan::key_pow2(nq);
        GORIO_HIP_CHECK(search_fail, s->d_qkeys.reserve((size_t)r.npow2));
        r.sq = SearchQueries{jobs[j].d_q, s->d_qkeys, jobs[j].stride_bytes / 4, nq};
        r.qkeys = s->d_qkeys;
      }
      const size_t qcap = search_plan::grown((size_t)nq + 1);
      GORIO_HIP_CHECK(search_fail, reserve_group(s->rq_cap, (size_t)nq + 1, qcap, s->d_found, qcap, s->d_found_offs, qcap, s->d_kept_offs, qcap));
      r.bb = c.bb;
      r.found = s->d_found;
      r.found_offs = lead->b_found_offs + lay.offs_first[j];
      r.kept_offs = s->d_kept_offs;
      r.r2 = (float)(jobs[j].radius * jobs[j].radius);
      r.max_nn = jobs[j].max_nn;
      r.nq = nq;
    }
    std::memcpy(tab.data() + o_wave, lay.wave_tab.data(), sizeof(search_plan::WaveRef) * (size_t)n_waves);
    std::memcpy(tab.data() + o_qf, lay.query_first.data(), sizeof(int) * ((size_t)count + 1));
    std::memcpy(tab.data() + o_kf, lay.key_first.data(), sizeof(int) * ((size_t)n_segs + 1));
    if (n_segs > 0) std::memcpy(tab.data() + o_kj, lay.key_jobs.data(), sizeof(int) * (size_t)n_segs);
    if (int rc = search_upload_staged(stream, lead->pin_tab, lead->b_tab, tab.data(), tab_bytes)) return rc;
    const unsigned char* d_tab = lead->b_tab;
    const SearchJob* d_jobs = reinterpret_cast<const SearchJob*>(d_tab);
    const search_plan::WaveRef* d_wave = reinterpret_cast<const search_plan::WaveRef*>(d_tab + o_wave);
    const int* d_qf = reinterpret_cast<const int*>(d_tab + o_qf);
    const int* d_kf = reinterpret_cast<const int*>(d_tab + o_kf);
    const int* d_kj = reinterpret_cast<const int*>(d_tab + o_kj);
    if (n_segs > 0) {
      search_query_keys_batch_kernel<<<(unsigned)lay.key_items, 256, 0, stream>>>(d_jobs, d_kf, d_kj, n_segs);
      enqueue_tiled_sort(stream, BatchQueryKeys{d_jobs, d_kj}, n_segs, lay.max_key_pow2);
      st.launches += 1 + tiled_sort_launches(lay.max_key_pow2);
    }
    search_radius_batch_kernel<0><<<n_waves, 64, 0, stream>>>(d_jobs, d_wave);
    search_scan_batch_kernel<<<count, 1024, 0, stream>>>(d_jobs);
    st.launches += 2;
    GORIO_HIP_CHECK(search_fail, hipGetLastError());
    long long* const foffs = static_cast<long long*>(lead->b_h_offs.get());
    GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(foffs, lead->b_found_offs, sizeof(long long) * n_offs, hipMemcpyDeviceToHost, stream));
    GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(stream));
    ++st.syncs;
    // ---- the plans.  Nothing of any job's held result is replaced before every job has passed.
    for (int j = 0; j < count; ++j) {
      if (!shapes[j].active) continue;
      const long long* fo = foffs + lay.offs_first[j];
      const int nq = jobs[j].nq;
      if (fo[nq] > search_plan::kMaxTotal) return search_fail(GORIO_ERR_UNSUPPORTED, "radius_batch: job " + std::to_string(j) + ": more than 2^31 - 1 neighbours found");
      if (!search_plan::make_plan(fo, nq, jobs[j].max_nn, plans[j]))
        return search_fail(GORIO_ERR_UNSUPPORTED, "radius_batch: job " + std::to_string(j) + ": the neighbours found cannot be planned (more than 2^31 - 1, or a segment too long to sort)");
    }
    search_plan::BatchLongPlan lp;
    search_plan::merge_long_segs(plans.data(), count, lp);
    bool any_found = false;
    for (int j = 0; j < count; ++j) {
      if (!shapes[j].active) continue;
      gorio_search_handle* s = jobs[j].s;
      const long long* fo = foffs + lay.offs_first[j];
      const int nq = jobs[j].nq;
      std::vector<int> cnt((size_t)nq);
      std::vector<long long> f2((size_t)nq + 1);
      koffs[j].resize((size_t)nq + 1);
      for (int q = 0; q < nq; ++q) cnt[q] = (int)(fo[q + 1] - fo[q]);
      search_plan::offsets_from_counts(cnt.data(), nq, jobs[j].max_nn, f2.data(), koffs[j].data());
      const size_t found = (size_t)plans[j].found_total, kept = (size_t)plans[j].kept_total;
      if (found == 0) continue;
      any_found = true;
      GORIO_HIP_CHECK(search_fail, s->d_keys.reserve(found, search_plan::grown(found)));
      s->r_valid = false;  // from here on this job's held result is being replaced
      GORIO_HIP_CHECK(search_fail, reserve_group(s->r_cap, kept, search_plan::grown(kept), s->d_ridx, search_plan::grown(kept), s->d_rsqd, search_plan::grown(kept)));
      rec[j].keys = s->d_keys;
      rec[j].ridx = s->d_ridx;
      rec[j].rsqd = s->d_rsqd;
    }
    if (any_found) {
      // the job records once more, now with the buffers the totals sized
      if (int rc = search_upload_staged(stream, lead->pin_tab, lead->b_tab, tab.data(), o_wave)) return rc;
      search_radius_batch_kernel<1><<<n_waves, 64, 0, stream>>>(d_jobs, d_wave);
      search_segment_sort_batch_kernel<<<n_queries, 256, 0, stream>>>(d_jobs, d_qf, count);
      st.launches += 2;
      GORIO_HIP_CHECK(search_fail, hipGetLastError());
      if (!lp.segs.empty()) {
        const int nl = (int)lp.segs.size();
        GORIO_HIP_CHECK(search_fail, lead->b_segs.reserve((size_t)nl, search_plan::grown((size_t)nl)));
        GORIO_HIP_CHECK(search_fail, lead->d_slots.reserve((size_t)lp.slot_keys, search_plan::grown((size_t)lp.slot_keys)));
        if (int rc = search_upload_staged(stream, lead->pin_segs, lead->b_segs, lp.segs.data(), sizeof(search_plan::BatchLongSeg) * (size_t)nl)) return rc;
        const dim3 grid((unsigned)std::min(64, (lp.max_pow2 + 255) / 256), (unsigned)nl);
        search_long_pad_batch_kernel<<<grid, 256, 0, stream>>>(d_jobs, lead->b_segs, lead->d_slots);
        enqueue_tiled_sort(stream, BatchLongSegKeys{lead->b_segs, lead->d_slots}, nl, lp.max_pow2);
        search_long_emit_batch_kernel<<<grid, 256, 0, stream>>>(d_jobs, lead->b_segs, lead->d_slots);
        st.launches += 2 + tiled_sort_launches(lp.max_pow2);
        GORIO_HIP_CHECK(search_fail, hipGetLastError());
      }
    }
  }
  // ---- every job's result becomes the one its state holds
  for (int j = 0; j < count; ++j) {
    gorio_search_handle* s = jobs[j].s;
    const int nq = jobs[j].nq;
    if (!shapes[j].active) koffs[j].assign((size_t)nq + 1, 0);
    if (jobs[j].count_out)
      for (int q = 0; q < nq; ++q) jobs[j].count_out[q] = (int)(koffs[j][q + 1] - koffs[j][q]);
    s->r_offs.swap(koffs[j]);
    s->r_nq = nq;
    s->r_valid = true;
    jobs[j].total = plans[j].kept_total;
  }
  if (stats) {
    stats->launches += st.launches;
    stats->syncs += st.syncs;
  }
  return GORIO_OK;
}

}  // namespace

extern "C" {

const char* gorio_search_last_error(void) { return g_search_err.c_str(); }

int gorio_search_create(gorio_search_t** out, int device) {
  if (!out) return search_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  if (device < 0) return search_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  gorio_search_handle* s = new (std::nothrow) gorio_search_handle();
  if (!s) return search_fail(GORIO_ERR_ALLOC, "create: out of memory");
  s->device = device;
  const int rc = gorio_apd_create(&s->up, device);
  if (rc) {
    delete s;
    return search_fail(rc, rc == GORIO_ERR_INVALID ? "create: bad device ordinal" : "create: no usable HIP device (there is no CPU fallback)");
  }
  s->up->params.search = GORIO_SEARCH_PRUNED;
  *out = s;
  return GORIO_OK;
}

void gorio_search_destroy(gorio_search_t* s) {
  if (!s) return;
  hipSetDevice(s->device);
  hipStreamSynchronize(s->up->stream);
  gorio_apd* up = s->up;
  delete s;  // the buffers, with the device current
  gorio_apd_destroy(up);
}

int gorio_search_set_cloud(gorio_search_t* s, const float* xyz, int n, int stride_bytes) {
  if (n < 0 || (n > 0 && !xyz) || stride_bytes < 12 || (stride_bytes % 4) != 0) return search_fail(GORIO_ERR_INVALID, "set_cloud: bad cloud arguments");
  if (!s) return search_fail(GORIO_ERR_INVALID, "set_cloud: null handle");
  const size_t st = stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + (size_t)i * st;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return search_fail(GORIO_ERR_INVALID, "set_cloud: point " + std::to_string(i) + " is not finite");
  }
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  if (n == 0) {
    gorio_apd_clear_source(s->up);
    return GORIO_OK;
  }
  int rc = gorio_apd_set_source(s->up, xyz, nullptr, n, stride_bytes);  // detaches a shared cloud first
  if (rc) return search_fail(rc, "set_cloud: " + s->up->err);
  ++s->point_uploads;
  bool built = false;
  if ((rc = search_build_index(s->up, s->up->src.get(), &built))) return rc;
  s->index_builds += built ? 1 : 0;
  return GORIO_OK;
}

int gorio_search_set_cloud_device(gorio_search_t* s, const float* x, const float* y, const float* z, int n) {
  if (n < 0 || (n > 0 && (!x || !y || !z))) return search_fail(GORIO_ERR_INVALID, "set_cloud_device: bad cloud arguments");
  if (!s) return search_fail(GORIO_ERR_INVALID, "set_cloud_device: null handle");
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  if (n == 0) {
    gorio_apd_clear_source(s->up);
    return GORIO_OK;
  }
  const int bad = search_device_cloud_nonfinite(s, x, y, z, n);
  if (bad < 0) return bad;
  if (bad) return search_fail(GORIO_ERR_INVALID, "set_cloud_device: the cloud has a non-finite point");
  int rc = gorio_apd_set_source_device(s->up, x, y, z, nullptr, n);
  if (rc) return search_fail(rc, "set_cloud_device: " + s->up->err);
  bool built = false;
  if ((rc = search_build_index(s->up, s->up->src.get(), &built))) return rc;
  s->index_builds += built ? 1 : 0;
  return GORIO_OK;
}

int gorio_search_set_cloud_from_apd(gorio_search_t* s, gorio_apd_t* apd, int which) {
  if (!s || !apd) return search_fail(GORIO_ERR_INVALID, "set_cloud_from_apd: null argument");
  if (which != 0 && which != 1) return search_fail(GORIO_ERR_INVALID, "set_cloud_from_apd: which must be 0 (source) or 1 (target)");
  if (s->device != apd->device) return search_fail(GORIO_ERR_INVALID, "set_cloud_from_apd: both handles must live on one device");
  const std::shared_ptr<DevCloud>& c = which == 0 ? apd->src : apd->tgt;
  if (!c->present) return search_fail(GORIO_ERR_STATE, which == 0 ? "set_cloud_from_apd: the registration handle has no input source" : "set_cloud_from_apd: the registration handle has no input target");
  return search_share(s, "set_cloud_from_apd", apd, c);
}

int gorio_search_set_cloud_from_keyframe(gorio_search_t* s, gorio_kf_t* kf, int id) {
  if (!s || !kf) return search_fail(GORIO_ERR_INVALID, "set_cloud_from_keyframe: null argument");
  if (s->device != kf->device) return search_fail(GORIO_ERR_INVALID, "set_cloud_from_keyframe: the store and the handle must live on one device");
  int rc = GORIO_OK;
  std::string why;
  const KfEntry* e = kf_entry(kf, id, &rc, &why);
  if (!e) return search_fail(rc, "set_cloud_from_keyframe: " + why);
  if (e->n == 0 || !e->cloud->present) {  // an empty keyframe: the empty cloud
    GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
    gorio_apd_clear_source(s->up);
    return GORIO_OK;
  }
  return search_share(s, "set_cloud_from_keyframe", kf->up, e->cloud);
}

int gorio_search_cloud_size(const gorio_search_t* s, int* n) {
  if (!s || !n) return search_fail(GORIO_ERR_INVALID, "cloud_size: null argument");
  *n = search_cloud_n(s);
  return GORIO_OK;
}

int gorio_search_get_counters(const gorio_search_t* s, long long* point_uploads, long long* index_builds, long long* result_downloads) {
  if (!s) return search_fail(GORIO_ERR_INVALID, "get_counters: null handle");
  if (point_uploads) *point_uploads = s->point_uploads;
  if (index_builds) *index_builds = s->index_builds;
  if (result_downloads) *result_downloads = s->result_downloads;
  return GORIO_OK;
}

int gorio_search_knn_device(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, int k, int* idx_out, float* sqd_out, int* count_out) {
  if (int rc = search_check_knn("knn_device", s, nq, stride_bytes, k, idx_out, sqd_out)) return rc;
  if (int rc = search_self_nq("knn_device", s, q_xyz, nq)) return rc;
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  return search_knn_core(s, q_xyz, nq, stride_bytes, k, idx_out, sqd_out, count_out);
}

int gorio_search_knn(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, int k, int* idx_out, float* sqd_out, int* count_out) {
  if (int rc = search_check_knn("knn", s, nq, stride_bytes, k, idx_out, sqd_out)) return rc;
  if (int rc = search_self_nq("knn", s, q_xyz, nq)) return rc;
  if (nq == 0) return GORIO_OK;
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  gorio_apd* h = s->up;
  if (q_xyz) {
    if (int rc = search_upload_queries(s, q_xyz, nq, stride_bytes)) return rc;
  }
  const size_t m = (size_t)nq * k;
  GORIO_HIP_CHECK(search_fail, s->d_idx.reserve(m, search_plan::grown(m)));
  GORIO_HIP_CHECK(search_fail, s->d_sqd.reserve(m, search_plan::grown(m)));
  GORIO_HIP_CHECK(search_fail, s->d_cnt.reserve((size_t)nq, search_plan::grown((size_t)nq)));
  if (int rc = search_knn_core(s, q_xyz ? s->d_q.get() : nullptr, nq, 12, k, s->d_idx, s->d_sqd, s->d_cnt)) return rc;
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(idx_out, s->d_idx, sizeof(int) * m, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(sqd_out, s->d_sqd, sizeof(float) * m, hipMemcpyDeviceToHost, h->stream));
  if (count_out) GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(count_out, s->d_cnt, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));
  ++s->result_downloads;
  return GORIO_OK;
}

int gorio_search_radius_device(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, double radius, int max_nn, int* count_out, long long* total) {
  if (int rc = search_check_radius("radius_device", s, nq, stride_bytes, radius, max_nn, total)) return rc;
  if (int rc = search_self_nq("radius_device", s, q_xyz, nq)) return rc;
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  return search_radius_core(s, q_xyz, nq, stride_bytes, radius, max_nn, count_out, total);
}

int gorio_search_radius(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, double radius, int max_nn, int* count_out, long long* total) {
  if (int rc = search_check_radius("radius", s, nq, stride_bytes, radius, max_nn, total)) return rc;
  if (int rc = search_self_nq("radius", s, q_xyz, nq)) return rc;
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  if (q_xyz && nq > 0) {
    if (int rc = search_upload_queries(s, q_xyz, nq, stride_bytes)) return rc;
  }
  return search_radius_core(s, (q_xyz && nq > 0) ? s->d_q.get() : nullptr, nq, 12, radius, max_nn, count_out, total);
}

int gorio_search_radius_batch(gorio_search_t** handles, int count, const float* const* q_xyz, const int* nq, const int* stride_bytes, const double* radius, const int* max_nn,
                              int* const* count_out, long long* totals) {
  if (count == 0) return GORIO_OK;
  if (count < 0) return search_fail(GORIO_ERR_INVALID, "radius_batch: count must not be negative");
  if (!handles || !q_xyz || !nq || !stride_bytes || !radius || !max_nn || !totals) return search_fail(GORIO_ERR_INVALID, "radius_batch: null array");
  // ---- every job's arguments, before any device call and before any state changes
  std::unordered_set<const gorio_search_handle*> distinct;
  for (int j = 0; j < count; ++j) {
    const std::string who = "radius_batch: job " + std::to_string(j);
    if (!handles[j]) return search_fail(GORIO_ERR_INVALID, who + ": null handle");
    if (handles[j]->device != handles[0]->device) return search_fail(GORIO_ERR_INVALID, who + ": all handles of a batch must live on one device");
    if (!distinct.insert(handles[j]).second) return search_fail(GORIO_ERR_INVALID, who + ": the same handle appears twice in a batch (it holds one result)");
    if (int rc = search_check_radius(who.c_str(), handles[j], nq[j], stride_bytes[j], radius[j], max_nn[j], totals)) return rc;
    if (int rc = search_self_nq(who.c_str(), handles[j], q_xyz[j], nq[j])) return rc;
  }
  GORIO_HIP_CHECK(search_fail, hipSetDevice(handles[0]->device));
  hipStream_t stream = handles[0]->up->stream;
  // ---- the queries: packed on the host, every job into the buffer of its own state, one synchronisation for all of them
  std::vector<std::vector<float>> packed((size_t)count);
  std::vector<SearchBatchJob> jobs((size_t)count);
  for (int j = 0; j < count; ++j) {
    gorio_search_handle* s = handles[j];
    const bool cross = q_xyz[j] && nq[j] > 0;
    if (cross) {
      std::vector<float>& buf = packed[j];
      buf.resize((size_t)nq[j] * 3);
      const size_t st = stride_bytes[j] / 4;
      for (int i = 0; i < nq[j]; ++i) {
        const float* p = q_xyz[j] + (size_t)i * st;
        buf[3 * (size_t)i] = p[0], buf[3 * (size_t)i + 1] = p[1], buf[3 * (size_t)i + 2] = p[2];
      }
      GORIO_HIP_CHECK(search_fail, s->d_q.reserve(buf.size(), search_plan::grown(buf.size())));
      GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(s->d_q, buf.data(), sizeof(float) * buf.size(), hipMemcpyHostToDevice, stream));
    }
    jobs[j] = SearchBatchJob{s, cross ? s->d_q.get() : nullptr, nq[j], 12, radius[j], max_nn[j], count_out ? count_out[j] : nullptr, 0};
  }
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(stream));  // the packed queries are pageable
  if (int rc = search_radius_batch_core(jobs.data(), count, nullptr)) return rc;
  for (int j = 0; j < count; ++j) totals[j] = jobs[j].total;
  return GORIO_OK;
}

int gorio_search_radius_get(gorio_search_t* s, long long* offsets_out, int* idx_out, float* sqd_out, long long capacity) {
  if (!s) return search_fail(GORIO_ERR_INVALID, "radius_get: null handle");
  if (!s->r_valid) return search_fail(GORIO_ERR_STATE, "radius_get: no radius result is held");
  const long long total = s->r_offs[(size_t)s->r_nq];
  if (!search_plan::capacity_ok(capacity, total)) return search_fail(GORIO_ERR_INVALID, "radius_get: capacity " + std::to_string(capacity) + " is below the total " + std::to_string(total));
  GORIO_HIP_CHECK(search_fail, hipSetDevice(s->device));
  gorio_apd* h = s->up;
  if (total > 0 && idx_out) GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(idx_out, s->d_ridx, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  if (total > 0 && sqd_out) GORIO_HIP_CHECK(search_fail, hipMemcpyAsync(sqd_out, s->d_rsqd, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(search_fail, hipStreamSynchronize(h->stream));
  if (offsets_out) std::copy(s->r_offs.begin(), s->r_offs.end(), offsets_out);
  ++s->result_downloads;
  return GORIO_OK;
}

}  // extern "C"
