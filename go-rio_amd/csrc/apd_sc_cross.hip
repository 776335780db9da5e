// apd_sc_cross.hip -- Scan Context matching between two databases (include/gorio_sc_cross.h): listed pairs, whole matrices, the K best
// matches per row and a detect over lists, each with the query side read from one handle and the database side from another.  Included by
// apd_api.hip after apd_sc_pairs.hip, whose records, staging, row minimum and host helpers it uses.  An extension, like apd_sc_pairs.hip.
//
//   listed pairs     sc_xpairs_kernel   sc_pairs_kernel with the two sides in two databases (gorio_sc_cross_distance_pairs,
//                                       gorio_sc_cross_detect, the latter followed by sc_rowmin_kernel)
//   matrix tiles     sc_xtile_kernel    the matrix form of sc_tile_kernel, row records staged from Q and column records from D
//                                       (gorio_sc_cross_distance_matrix)
//   K-best tiles     sc_top_kernel      the folding form of its own: a workgroup walks a run of column tiles and every wave keeps the k
//                                       best (dist, column) of its row across its lanes 0 .. k - 1 (gorio_sc_cross_top_matches)
//   K row minimum    sc_rowtop_kernel   one wave per row: the k smallest (dist, column) keys of the runs' partial lists
// Every distance comes out of sc_pair_eval, so it has the bits gorio_sc_distance gives.  No floating-point atomics, no waits between
// workgroups; what is kept and in which order is decided by the (dist, column) keys, never by timing.
#include <hip/hip_runtime.h>

#include <algorithm>

namespace gorio {

constexpr int kScTopMax = GORIO_SC_TOP_MAX;
static_assert(kScTopMax <= 64 && kScTopMax * 2 == 16, "a wave keeps its list in its first lanes; the merge of a row's two lists indexes 16 slots");

// sc_pairs_kernel with the query side in dq and the candidate side in dd.
__global__ __launch_bounds__(kScThreads) void sc_xpairs_kernel(const ScPairRef* __restrict__ pairs, int n_pairs, ScDb dq, ScDb dd, ScBest* __restrict__ out) {
  __shared__ ScPairScratch scratch[kScThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long pair = (long long)blockIdx.x * (kScThreads / 64) + w;
  const bool live = pair < n_pairs;
  const ScPairRef P = live ? pairs[pair] : ScPairRef{0, 0};
  const size_t q = P.q, c = P.c;
  double m = 0.0;
  int arg = 0;
  sc_pair_eval(live, lane, scratch[w], dq.sector + q * kScSectors, dd.sector + c * kScSectors, dq.colnorm + q * kScSectors, dd.colnorm + c * kScSectors,
               dq.desc + q * kScBins, dd.desc + c * kScBins, m, arg);
  if (live && lane == 0) out[pair] = ScBest{m, P.c, arg};
}

// The matrix form of sc_tile_kernel (its shape, its staging, its wave-to-pair map) with the row records staged from dq and the column
// records from dd; one column tile per workgroup (A.run_tiles, A.min_gap and A.partial are not read).
//   LDS 122,304 B static, 65 VGPRs, scratch 0, no spills, 4 waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage); LDS traffic is
//   ds_read / ds_write only.  One column tile per workgroup, so both index lists are filled before one barrier and both record sets
//   staged before the next.
__global__ __launch_bounds__(kScTileThreads) void sc_xtile_kernel(ScTileArgs A, ScDb dq, ScDb dd) {
  __shared__ __attribute__((aligned(16))) double rec[(kScTileR + kScTileC) * kScRecord];
  __shared__ ScPairScratch scratch[kScTileWaves];
  __shared__ int ridx[kScTileR], cidx[kScTileC];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int tr = blockIdx.x / A.n_ctiles, tc = blockIdx.x % A.n_ctiles;
  const int r0 = tr * kScTileR, nr = min(kScTileR, A.n_rows - r0);
  const int c0 = tc * kScTileC, nc = min(kScTileC, A.n_cols - c0);
  if (t < nr) ridx[t] = A.rows ? A.rows[r0 + t] : r0 + t;
  if (t >= 64 && t - 64 < nc) cidx[t - 64] = A.cols ? A.cols[c0 + t - 64] : c0 + t - 64;
  __syncthreads();
  sc_stage_records(rec, ridx, nr, dq, t);
  sc_stage_records(rec + kScTileR * kScRecord, cidx, nc, dd, t);
  __syncthreads();
  const int ri = w >> 1, cbase = (w & 1) * kScPairsPerWave;
  const double* R = rec + ri * kScRecord;
#pragma unroll 1
  for (int i = 0; i < kScPairsPerWave; ++i) {
    const int ci = cbase + i;
    const bool live = ri < nr && ci < nc;
    const double* C = rec + (kScTileR + ci) * kScRecord;
    double m = 0.0;
    int arg = 0;
    sc_pair_eval(live, lane, scratch[w], R + kScBins, C + kScBins, R + kScBins + kScSectors, C + kScBins + kScSectors, R, C, m, arg);
    if (live && lane == 0) {
      const size_t o = (size_t)(r0 + ri) * A.n_cols + (c0 + ci);
      if (A.dist) A.dist[o] = m;
      if (A.shift) A.shift[o] = arg;
    }
  }
}

struct ScTopArgs {
  const int* rows;     // query index of row i, or null: i
  const int* col_end;  // row i takes the columns 0 .. col_end[i] - 1, or null: n_cols for every row
  int n_rows, n_cols;  // n_cols: the largest col_end; column j is database index j
  int n_ctiles;        // column tiles in all
  int run_tiles;       // column tiles one workgroup walks
  int n_runs;          // runs per row tile
  int k;               // 1 .. kScTopMax
  ScBest* partial;     // [n_rows][n_runs][k], each list ascending in (d, c), unused slots {1e7, -1, 0}
};

// The K-best form of the tile kernel: sc_tile_kernel<true>'s walk over a run of column tiles, with a list of the k best instead of one
// running best.  The list of a wave lies ACROSS its lanes, lane j < k holding the j-th smallest (d, c) key of the wave's row so far in
// three scalars of its own (kd, kc, ks; c = -1: unused, and unused slots come last).  A new pair (m, c) is inserted by ballot: its
// position is the number of lanes whose key is smaller, the lanes behind it take their left neighbour's entry (one __shfl_up each for
// d, c and s) and the lane at the position takes the pair; what falls off lane k - 1 lands in lanes that are never read.  Nothing is
// indexed at run time, so the list costs 4 VGPRs and no scratch; k stays a runtime argument.  Keys of a row are unique (its columns are),
// so the order in which pairs arrive does not matter.
// At the end every wave writes its list to LDS, and the 16 slots of a row's two waves (which saw interleaved column groups) are merged
// by rank: a slot's position in the output is the number of the row's keys below its own.
//   LDS 124,384 B static (the matrix form's 122,304 B + 16 lists of 8 x 16 B + the rows' col_end), 100 VGPRs, scratch 0, no spills,
//   4 waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage); no flat access to LDS.  The two outer loops stay rolled, as in
//   sc_tile_kernel.
__global__ __launch_bounds__(kScTileThreads) void sc_top_kernel(ScTopArgs A, ScDb dq, ScDb dd) {
  __shared__ __attribute__((aligned(16))) double rec[(kScTileR + kScTileC) * kScRecord];
  __shared__ ScPairScratch scratch[kScTileWaves];
  __shared__ int ridx[kScTileR], rend[kScTileR], cidx[kScTileC];
  __shared__ double top_d[kScTileWaves][kScTopMax];
  __shared__ int top_c[kScTileWaves][kScTopMax], top_s[kScTileWaves][kScTopMax];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int tr = blockIdx.x / A.n_runs, run = blockIdx.x % A.n_runs;
  const int r0 = tr * kScTileR, nr = min(kScTileR, A.n_rows - r0);
  if (t < nr) {
    ridx[t] = A.rows ? A.rows[r0 + t] : r0 + t;
    rend[t] = A.col_end ? A.col_end[r0 + t] : A.n_cols;
  }
  __syncthreads();
  sc_stage_records(rec, ridx, nr, dq, t);
  int limit = 0;  // one past the largest column any row of this tile accepts
  for (int i = 0; i < nr; ++i) limit = max(limit, rend[i]);
  const int ri = w >> 1, cbase = (w & 1) * kScPairsPerWave;
  const int my_end = ri < nr ? rend[ri] : 0;
  const double* R = rec + ri * kScRecord;
  double kd = 10000000.0;
  int kc = -1, ks = 0;
  const int tc_end = min(A.n_ctiles, (run + 1) * A.run_tiles);
#pragma unroll 1
  for (int tc = run * A.run_tiles; tc < tc_end; ++tc) {
    const int c0 = tc * kScTileC, nc = min(kScTileC, A.n_cols - c0);
    if (c0 >= limit) break;  // uniform over the workgroup
    __syncthreads();         // the previous tile's records and indices are no longer read
    if (t < nc) cidx[t] = c0 + t;
    __syncthreads();
    sc_stage_records(rec + kScTileR * kScRecord, cidx, nc, dd, t);
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < kScPairsPerWave; ++i) {
      const int ci = cbase + i, c = c0 + ci;
      const bool live = ci < nc && c < my_end;  // uniform over the wave
      const double* C = rec + (kScTileR + ci) * kScRecord;
      double m = 0.0;
      int arg = 0;
      sc_pair_eval(live, lane, scratch[w], R + kScBins, C + kScBins, R + kScBins + kScSectors, C + kScBins + kScSectors, R, C, m, arg);
      if (live) {
        const double nd = __shfl(m, 0, 64);  // lane 0 holds the pair's result
        const int ns = __shfl(arg, 0, 64);
        if (nd < 10000000.0) {
          const bool below = lane < A.k && kc >= 0 && (kd < nd || (kd == nd && kc < c));
          const int pos = __popcll(__ballot(below));
          const double ud = __shfl_up(kd, 1, 64);
          const int uc = __shfl_up(kc, 1, 64), us = __shfl_up(ks, 1, 64);
          if (lane > pos) {
            kd = ud;
            kc = uc;
            ks = us;
          } else if (lane == pos) {
            kd = nd;
            kc = c;
            ks = ns;
          }
        }
      }
    }
  }
  if (lane < kScTopMax) {
    top_d[w][lane] = kd;
    top_c[w][lane] = kc;
    top_s[w][lane] = ks;
  }
  __syncthreads();
  if (t < nr * 2 * kScTopMax) {  // thread (row, slot j of the 16 of the row's two waves)
    const int row = t / (2 * kScTopMax), j = t % (2 * kScTopMax);
    const int mw = 2 * row + j / kScTopMax, ms = j % kScTopMax;
    const double d = top_d[mw][ms];
    const int c = top_c[mw][ms];
    const bool have = ms < A.k && c >= 0;
    int rank = 0, n_have = 0;
#pragma unroll 1
    for (int o = 0; o < 2 * kScTopMax; ++o) {
      const int ow = 2 * row + o / kScTopMax, os = o % kScTopMax;
      const int oc = top_c[ow][os];
      if (os < A.k && oc >= 0) {
        const double od = top_d[ow][os];
        n_have += 1;
        rank += (od < d || (od == d && oc < c)) ? 1 : 0;
      }
    }
    ScBest* out = A.partial + ((size_t)(r0 + row) * A.n_runs + run) * A.k;
    if (have && rank < A.k) out[rank] = ScBest{d, c, top_s[mw][ms]};
    if (j < A.k && j >= n_have) out[j] = ScBest{10000000.0, -1, 0};  // ranks 0 .. n_have - 1 are taken by the entries, the rest is unused
  }
}

// One wave per row of `per_row` items (the runs' lists; unused slots have c = -1): the k items with the smallest (d, c) keys in
// ascending order, {1e7, -1, 0} where fewer exist.  The keys of a row are unique, so round j takes the smallest key above the one
// round j - 1 took: exact, and independent of where the items lie.  Compared as doubles: 1 - mean cosine can round below 0.
__global__ __launch_bounds__(kScThreads) void sc_rowtop_kernel(const ScBest* __restrict__ items, int n_rows, int per_row, int k, ScBest* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (kScThreads / 64) + (threadIdx.x >> 6);
  if (row >= n_rows) return;
  const ScBest* it = items + (size_t)row * per_row;
  double ld = 0.0;
  int lc = -1;
  bool first = true;
  for (int j = 0; j < k; ++j) {
    double bd = 10000000.0;
    int bc = INT_MAX, bp = -1;
    for (int p = lane; p < per_row; p += 64) {
      const double d = it[p].d;
      const int c = it[p].c;
      if (c >= 0 && (first || d > ld || (d == ld && c > lc)) && (d < bd || (d == bd && c < bc))) {
        bd = d;
        bc = c;
        bp = p;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(bd, off, 64);
      const int oc = __shfl_xor(bc, off, 64), op = __shfl_xor(bp, off, 64);
      if (od < bd || (od == bd && oc < bc)) {
        bd = od;
        bc = oc;
        bp = op;
      }
    }
    if (lane == 0) out[(size_t)row * k + j] = bp < 0 ? ScBest{10000000.0, -1, 0} : ScBest{bd, bc, it[bp].s};
    // nothing found: (1e7, INT_MAX), above which no item lies, so the later rounds find nothing either
    ld = bd;
    lc = bc;
    first = false;
  }
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_sc_cross.h)
namespace {

// The checks on the pair of handles that every call of the header starts with.
int scc_check_handles(const gorio_sc* Q, const gorio_sc* D, const char* fn) {
  if (!Q || !D) return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": null " + (!Q ? "query" : "database") + " handle");
  if (Q->device != D->device)
    return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": the query handle is on device " + std::to_string(Q->device) + ", the database handle on device " + std::to_string(D->device));
  if (Q->p.azimuth_range != D->p.azimuth_range)
    return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": azimuth_range differs, " + std::to_string(Q->p.azimuth_range) + " in the query handle and " + std::to_string(D->p.azimuth_range) +
                                          " in the database handle: the descriptors are not comparable");
  return GORIO_OK;
}

int scc_not_added(const char* fn, const std::string& what, int value, bool query_side, int n) {
  return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": " + what + " = " + std::to_string(value) + " has not been added to the " + (query_side ? "query" : "database") + " handle (" +
                                        std::to_string(n) + " scans)");
}

// rows / cols of the matrix calls on one side: null means 0 .. n - 1 of that side's handle, so the extent must be its scan count.
int scc_check_indices(const gorio_sc* h, bool query_side, const char* fn, const char* what, const int* idx, int n) {
  if (!idx) {
    if (n != h->n)
      return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": null " + what + " means all " + std::to_string(h->n) + " scans of the " + (query_side ? "query" : "database") +
                                            " handle, but the extent is " + std::to_string(n));
    return GORIO_OK;
  }
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= h->n) return scc_not_added(fn, std::string(what) + "[" + std::to_string(i) + "]", idx[i], query_side, h->n);
  return GORIO_OK;
}

void scc_count(gorio_sc* Q, long long pairs, int launches) {
  Q->cx_calls += 1;
  Q->cx_pairs += pairs;
  Q->cx_launches += launches;
  Q->cx_syncs += 1;
}

}  // namespace

extern "C" {

int gorio_sc_cross_distance_pairs(gorio_sc_t* Q, gorio_sc_t* D, const int* q, const int* c, int count, double* dist, int* shift) {
  if (scc_check_handles(Q, D, "cross_distance_pairs")) return GORIO_ERR_INVALID;
  if (count < 0) return sc_fail(GORIO_ERR_INVALID, "cross_distance_pairs: count < 0");
  if (count == 0) return GORIO_OK;
  if (!q || !c || !dist || !shift) return sc_fail(GORIO_ERR_INVALID, "cross_distance_pairs: null argument");
  for (int k = 0; k < count; ++k) {
    if (q[k] < 0 || q[k] >= Q->n) return scc_not_added("cross_distance_pairs", "q[" + std::to_string(k) + "]", q[k], true, Q->n);
    if (c[k] < 0 || c[k] >= D->n) return scc_not_added("cross_distance_pairs", "c[" + std::to_string(k) + "]", c[k], false, D->n);
  }
  std::vector<gorio::ScPairRef> tab(count);
  for (int k = 0; k < count; ++k) tab[k] = gorio::ScPairRef{q[k], c[k]};
  std::vector<gorio::ScBest> res(count);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(Q->device));
  if (scx_reserve(Q, sizeof(gorio::ScPairRef) * tab.size(), sizeof(gorio::ScBest) * res.size())) return GORIO_ERR_ALLOC;
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(Q->d_px_in, tab.data(), sizeof(gorio::ScPairRef) * tab.size(), hipMemcpyHostToDevice, Q->stream));
  hipLaunchKernelGGL(gorio::sc_xpairs_kernel, dim3((unsigned)(((long long)count + 3) / 4)), dim3(gorio::kScThreads), 0, Q->stream, (const gorio::ScPairRef*)Q->d_px_in.get(), count, Q->db(),
                     D->db(), (gorio::ScBest*)Q->d_px_out.get());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), Q->d_px_out, sizeof(gorio::ScBest) * res.size(), hipMemcpyDeviceToHost, Q->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(Q->stream));
  scc_count(Q, count, 1);
  for (int k = 0; k < count; ++k) {
    dist[k] = res[k].d;
    shift[k] = res[k].s;
  }
  return GORIO_OK;
}

int gorio_sc_cross_distance_matrix(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* cols, int n_cols, double* dist, int* shift) {
  if (scc_check_handles(Q, D, "cross_distance_matrix")) return GORIO_ERR_INVALID;
  if (n_rows < 0 || n_cols < 0) return sc_fail(GORIO_ERR_INVALID, "cross_distance_matrix: negative extent");
  if (n_rows == 0 || n_cols == 0) return GORIO_OK;
  if (!dist && !shift) return sc_fail(GORIO_ERR_INVALID, "cross_distance_matrix: both outputs are null");
  if (scc_check_indices(Q, true, "cross_distance_matrix", "rows", rows, n_rows) || scc_check_indices(D, false, "cross_distance_matrix", "cols", cols, n_cols)) return GORIO_ERR_INVALID;
  const long long total = (long long)n_rows * n_cols;
  if (total > (long long)INT_MAX)
    return sc_fail(GORIO_ERR_UNSUPPORTED, "cross_distance_matrix: " + std::to_string(n_rows) + " x " + std::to_string(n_cols) + " pairs exceed 2^31 - 1");
  const size_t b_rows = rows ? scx_align16(sizeof(int) * n_rows) : 0, b_cols = cols ? scx_align16(sizeof(int) * n_cols) : 0;
  const size_t b_dist = dist ? scx_align16(sizeof(double) * total) : 0, b_shift = shift ? sizeof(int) * total : 0;
  std::vector<char> blob(b_rows + b_cols);
  if (rows) std::memcpy(blob.data(), rows, sizeof(int) * n_rows);
  if (cols) std::memcpy(blob.data() + b_rows, cols, sizeof(int) * n_cols);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(Q->device));
  if (scx_reserve(Q, blob.size(), b_dist + b_shift)) return GORIO_ERR_ALLOC;
  if (!blob.empty()) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(Q->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, Q->stream));
  gorio::ScTileArgs A{};
  A.rows = rows ? (const int*)Q->d_px_in.get() : nullptr;
  A.cols = cols ? (const int*)((const char*)Q->d_px_in.get() + b_rows) : nullptr;
  A.n_rows = n_rows, A.n_cols = n_cols;
  A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
  A.run_tiles = 1, A.n_runs = A.n_ctiles;
  A.dist = dist ? (double*)Q->d_px_out.get() : nullptr;
  A.shift = shift ? (int*)((char*)Q->d_px_out.get() + b_dist) : nullptr;
  const long long n_groups = (long long)((n_rows + gorio::kScTileR - 1) / gorio::kScTileR) * A.n_ctiles;  // <= 2^31 / 8 + n_rows + n_cols
  hipLaunchKernelGGL(gorio::sc_xtile_kernel, dim3((unsigned)n_groups), dim3(gorio::kScTileThreads), 0, Q->stream, A, Q->db(), D->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  if (dist) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(dist, A.dist, sizeof(double) * total, hipMemcpyDeviceToHost, Q->stream));
  if (shift) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(shift, A.shift, sizeof(int) * total, hipMemcpyDeviceToHost, Q->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(Q->stream));
  scc_count(Q, total, 1);
  return GORIO_OK;
}

int gorio_sc_cross_top_matches(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* col_end, int k, int* index, double* dist, int* shift) {
  if (scc_check_handles(Q, D, "cross_top_matches")) return GORIO_ERR_INVALID;
  if (n_rows < 0) return sc_fail(GORIO_ERR_INVALID, "cross_top_matches: negative extent");
  if (n_rows == 0) return GORIO_OK;
  if (!index || !dist) return sc_fail(GORIO_ERR_INVALID, "cross_top_matches: null output");
  if (k < 1) return sc_fail(GORIO_ERR_INVALID, "cross_top_matches: k = " + std::to_string(k) + " must be >= 1");
  if (k > GORIO_SC_TOP_MAX)
    return sc_fail(GORIO_ERR_UNSUPPORTED, "cross_top_matches: k = " + std::to_string(k) + " exceeds GORIO_SC_TOP_MAX = " + std::to_string(GORIO_SC_TOP_MAX));
  if (scc_check_indices(Q, true, "cross_top_matches", "rows", rows, n_rows)) return GORIO_ERR_INVALID;
  int n_cols = col_end ? 0 : D->n;  // the largest col_end
  long long pairs = col_end ? 0 : (long long)n_rows * D->n;
  if (col_end)
    for (int i = 0; i < n_rows; ++i) {
      if (col_end[i] < 0 || col_end[i] > D->n)
        return sc_fail(GORIO_ERR_INVALID, "cross_top_matches: col_end[" + std::to_string(i) + "] = " + std::to_string(col_end[i]) + " is outside 0 .. " + std::to_string(D->n) +
                                              ", the scan count of the database handle");
      n_cols = std::max(n_cols, col_end[i]);
      pairs += col_end[i];
    }
  const size_t n_out = (size_t)n_rows * k;
  std::vector<gorio::ScBest> res(n_out, gorio::ScBest{10000000.0, -1, 0});
  if (n_cols > 0) {
    const int n_rtiles = (n_rows + gorio::kScTileR - 1) / gorio::kScTileR;
    gorio::ScTopArgs A{};
    A.n_rows = n_rows, A.n_cols = n_cols, A.k = k;
    A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
    // enough column runs for about 2048 workgroups, as in gorio_sc_best_matches: the partial lists stay O(k * (n_rows + 8 * 2048))
    const int want_runs = std::min(A.n_ctiles, std::max(1, 2048 / n_rtiles));
    A.run_tiles = (A.n_ctiles + want_runs - 1) / want_runs;
    A.n_runs = (A.n_ctiles + A.run_tiles - 1) / A.run_tiles;
    const size_t n_partial = (size_t)n_rows * A.n_runs * k;
    if (n_partial > (size_t)INT_MAX) return sc_fail(GORIO_ERR_UNSUPPORTED, "cross_top_matches: too many rows");
    // upload: rows | col_end
    const size_t b_rows = rows ? scx_align16(sizeof(int) * (size_t)n_rows) : 0, b_end = col_end ? sizeof(int) * (size_t)n_rows : 0;
    std::vector<char> blob(b_rows + b_end);
    if (rows) std::memcpy(blob.data(), rows, sizeof(int) * (size_t)n_rows);
    if (col_end) std::memcpy(blob.data() + b_rows, col_end, b_end);
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(Q->device));
    if (scx_reserve(Q, blob.size(), sizeof(gorio::ScBest) * (n_partial + n_out))) return GORIO_ERR_ALLOC;
    if (!blob.empty()) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(Q->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, Q->stream));
    A.rows = rows ? (const int*)Q->d_px_in.get() : nullptr;
    A.col_end = col_end ? (const int*)((const char*)Q->d_px_in.get() + b_rows) : nullptr;
    A.partial = (gorio::ScBest*)Q->d_px_out.get();
    gorio::ScBest* d_res = A.partial + n_partial;
    hipLaunchKernelGGL(gorio::sc_top_kernel, dim3((unsigned)(n_rtiles * A.n_runs)), dim3(gorio::kScTileThreads), 0, Q->stream, A, Q->db(), D->db());
    hipLaunchKernelGGL(gorio::sc_rowtop_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(gorio::kScThreads), 0, Q->stream, (const gorio::ScBest*)A.partial, n_rows, A.n_runs * k, k, d_res);
    GORIO_HIP_CHECK(sc_fail, hipGetLastError());
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), d_res, sizeof(gorio::ScBest) * n_out, hipMemcpyDeviceToHost, Q->stream));
    GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(Q->stream));
    scc_count(Q, pairs, 2);
  }
  for (size_t i = 0; i < n_out; ++i) {
    index[i] = res[i].c;
    dist[i] = res[i].d;
    if (shift) shift[i] = res[i].s;
  }
  return GORIO_OK;
}

int gorio_sc_cross_detect(gorio_sc_t* Q, gorio_sc_t* D, int count, const int* qidx, const int* const* cands, const int* ncand, int* loop_id, float* yaw_rad, double* min_dist) {
  if (scc_check_handles(Q, D, "cross_detect")) return GORIO_ERR_INVALID;
  if (count < 0) return sc_fail(GORIO_ERR_INVALID, "cross_detect: count < 0");
  if (count == 0) return GORIO_OK;
  if (!qidx || !cands || !ncand || !loop_id || !yaw_rad || !min_dist) return sc_fail(GORIO_ERR_INVALID, "cross_detect: null argument");
  size_t total = 0;
  for (int i = 0; i < count; ++i) {
    const std::string at = " (query " + std::to_string(i) + ")";
    if (qidx[i] < 0 || qidx[i] >= Q->n)
      return sc_fail(GORIO_ERR_INVALID, "cross_detect: query index " + std::to_string(qidx[i]) + " has not been added to the query handle (" + std::to_string(Q->n) + " scans)" + at);
    if (ncand[i] <= 0 || !cands[i]) return sc_fail(GORIO_ERR_INVALID, "cross_detect: empty candidate list" + at);
    for (int j = 0; j < ncand[i]; ++j)
      if (cands[i][j] < 0 || cands[i][j] >= D->n)
        return sc_fail(GORIO_ERR_INVALID, "cross_detect: candidate " + std::to_string(j) + " = " + std::to_string(cands[i][j]) + " has not been added to the database handle (" +
                                              std::to_string(D->n) + " scans)" + at);
    total += ncand[i];
  }
  if (total > (size_t)INT_MAX) return sc_fail(GORIO_ERR_UNSUPPORTED, "cross_detect: more than 2^31 - 1 candidates in all");
  // CSR of the lists as they are: one segment per query, no early return and no recent-keyframe filter
  std::vector<gorio::ScPairRef> tab;
  tab.reserve(total);
  std::vector<int> off(1, 0);
  for (int i = 0; i < count; ++i) {
    for (int j = 0; j < ncand[i]; ++j) tab.push_back(gorio::ScPairRef{qidx[i], cands[i][j]});
    off.push_back((int)tab.size());
  }
  const int n_pairs = (int)tab.size();
  std::vector<gorio::ScBest> res(count);
  const size_t b_tab = scx_align16(sizeof(gorio::ScPairRef) * tab.size()), b_off = sizeof(int) * off.size();
  std::vector<char> blob(b_tab + b_off);
  std::memcpy(blob.data(), tab.data(), sizeof(gorio::ScPairRef) * tab.size());
  std::memcpy(blob.data() + b_tab, off.data(), b_off);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(Q->device));
  if (scx_reserve(Q, blob.size(), sizeof(gorio::ScBest) * (tab.size() + count))) return GORIO_ERR_ALLOC;
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(Q->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, Q->stream));
  gorio::ScBest* items = (gorio::ScBest*)Q->d_px_out.get();
  gorio::ScBest* d_res = items + tab.size();
  hipLaunchKernelGGL(gorio::sc_xpairs_kernel, dim3((unsigned)(((long long)n_pairs + 3) / 4)), dim3(gorio::kScThreads), 0, Q->stream, (const gorio::ScPairRef*)Q->d_px_in.get(), n_pairs,
                     Q->db(), D->db(), items);
  hipLaunchKernelGGL(gorio::sc_rowmin_kernel, dim3((unsigned)((count + 3) / 4)), dim3(gorio::kScThreads), 0, Q->stream, (const gorio::ScBest*)items,
                     (const int*)((const char*)Q->d_px_in.get() + b_tab), count, d_res);
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), d_res, sizeof(gorio::ScBest) * count, hipMemcpyDeviceToHost, Q->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(Q->stream));
  scc_count(Q, n_pairs, 2);
  const double unit = (Q->p.azimuth_range - (-Q->p.azimuth_range)) / double(GORIO_SC_SECTORS);  // PC_UNIT_SECTOR_ANGLE (SC:72)
  for (int i = 0; i < count; ++i) {
    const gorio::ScBest& o = res[i];
    const int nn_idx = o.c < 0 ? 0 : o.c, nn_align = o.c < 0 ? 0 : o.s;  // SC:312-314: the values the loop starts from
    loop_id[i] = o.d < Q->p.sc_dist_thresh ? nn_idx : -1;                // SC:354-356
    const float deg = (float)(nn_align * unit);                          // deg2rad(float degrees) (SC:18-21, 369)
    yaw_rad[i] = (float)((double)deg * M_PI / 180.0);
    min_dist[i] = o.d;
  }
  return GORIO_OK;
}

int gorio_sc_cross_counters(const gorio_sc_t* Q, long long* calls, long long* pairs, long long* launches, long long* synchronisations) {
  if (!Q) return sc_fail(GORIO_ERR_INVALID, "cross_counters: null handle");
  if (calls) *calls = Q->cx_calls;
  if (pairs) *pairs = Q->cx_pairs;
  if (launches) *launches = Q->cx_launches;
  if (synchronisations) *synchronisations = Q->cx_syncs;
  return GORIO_OK;
}

}  // extern "C"
