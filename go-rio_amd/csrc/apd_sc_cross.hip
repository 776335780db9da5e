// apd_sc_cross.hip -- what Scan Context matching between two databases (include/gorio_sc_cross.h) has of its own: the K best matches
// per row, the check on a pair of handles, and the header's entry points.  Its listed pairs, matrices and detect are the two-handle
// forms of apd_sc_pairs.hip's host paths and run that file's kernels.  Included by apd_api.hip after apd_sc_pairs.hip, whose records,
// staging, tile shape and host helpers it uses.  An extension, like apd_sc_pairs.hip.
//
//   K-best tiles     sc_top_kernel      the folding walk with a list: a workgroup walks a run of column tiles and every wave keeps the k
//                                       best (dist, column) of its row across its lanes 0 .. k - 1 (gorio_sc_cross_top_matches)
//   K row minimum    sc_rowtop_kernel   one wave per row: the k smallest (dist, column) keys of the runs' partial lists
// Every distance comes out of sc_pair_eval, so it has the bits gorio_sc_distance gives.  No floating-point atomics, no waits between
// workgroups; what is kept and in which order is decided by the (dist, column) keys, never by timing.
#include <hip/hip_runtime.h>

#include <algorithm>

namespace gorio {

constexpr int kScTopMax = GORIO_SC_TOP_MAX;
static_assert(kScTopMax <= 64 && kScTopMax * 2 == 16, "a wave keeps its list in its first lanes; the merge of a row's two lists indexes 16 slots");

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

// The K-best form of the folding kernel: sc_tile_kernel's walk over a run of column tiles, between two databases and with a list of the
// k best instead of one running best.  The list of a wave lies ACROSS its lanes, lane j < k holding the j-th smallest (d, c) key of the wave's row so far in
// three scalars of its own (kd, kc, ks; c = -1: unused, and unused slots come last).  A new pair (m, c) is inserted by ballot: its
// position is the number of lanes whose key is smaller, the lanes behind it take their left neighbour's entry (one __shfl_up each for
// d, c and s) and the lane at the position takes the pair; what falls off lane k - 1 lands in lanes that are never read.  Nothing is
// indexed at run time, so the list costs 4 VGPRs and no scratch; k stays a runtime argument.  Keys of a row are unique (its columns are),
// so the order in which pairs arrive does not matter.
// At the end every wave writes its list to LDS, and the 16 slots of a row's two waves (which saw interleaved column groups) are merged
// by rank: a slot's position in the output is the number of the row's keys below its own.
//   LDS 124,384 B static (the matrix kernel's 122,304 B + 16 lists of 8 x 16 B + the rows' col_end), 100 VGPRs, scratch 0, no spills,
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
int sc_check_handles(const gorio_sc* Q, const gorio_sc* D, const char* fn) {
  if (!Q || !D) return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": null " + (!Q ? "query" : "database") + " handle");
  if (Q->device != D->device)
    return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": the query handle is on device " + std::to_string(Q->device) + ", the database handle on device " + std::to_string(D->device));
  if (Q->p.azimuth_range != D->p.azimuth_range)
    return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": azimuth_range differs, " + std::to_string(Q->p.azimuth_range) + " in the query handle and " + std::to_string(D->p.azimuth_range) +
                                          " in the database handle: the descriptors are not comparable");
  return GORIO_OK;
}

}  // namespace

extern "C" {

int gorio_sc_cross_distance_pairs(gorio_sc_t* Q, gorio_sc_t* D, const int* q, const int* c, int count, double* dist, int* shift) {
  if (sc_check_handles(Q, D, "cross_distance_pairs")) return GORIO_ERR_INVALID;
  return sc_distance_pairs(sc_two_handles(Q, D, "cross_distance_pairs"), q, c, count, dist, shift);
}

int gorio_sc_cross_distance_matrix(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* cols, int n_cols, double* dist, int* shift) {
  if (sc_check_handles(Q, D, "cross_distance_matrix")) return GORIO_ERR_INVALID;
  return sc_distance_matrix(sc_two_handles(Q, D, "cross_distance_matrix"), rows, n_rows, cols, n_cols, dist, shift);
}

int gorio_sc_cross_top_matches(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* col_end, int k, int* index, double* dist, int* shift) {
  if (sc_check_handles(Q, D, "cross_top_matches")) return GORIO_ERR_INVALID;
  const ScSides S = sc_two_handles(Q, D, "cross_top_matches");
  if (n_rows < 0) return sc_refuse(S, GORIO_ERR_INVALID, "negative extent");
  if (n_rows == 0) return GORIO_OK;
  if (!index || !dist) return sc_refuse(S, GORIO_ERR_INVALID, "null output");
  if (k < 1) return sc_refuse(S, GORIO_ERR_INVALID, "k = " + std::to_string(k) + " must be >= 1");
  if (k > GORIO_SC_TOP_MAX) return sc_refuse(S, GORIO_ERR_UNSUPPORTED, "k = " + std::to_string(k) + " exceeds GORIO_SC_TOP_MAX = " + std::to_string(GORIO_SC_TOP_MAX));
  if (sc_check_indices(S, true, "rows", rows, n_rows)) return GORIO_ERR_INVALID;
  int n_cols = col_end ? 0 : D->n;  // the largest col_end
  long long pairs = col_end ? 0 : (long long)n_rows * D->n;
  if (col_end)
    for (int i = 0; i < n_rows; ++i) {
      if (col_end[i] < 0 || col_end[i] > D->n)
        return sc_refuse(S, GORIO_ERR_INVALID, "col_end[" + std::to_string(i) + "] = " + std::to_string(col_end[i]) + " is outside 0 .. " + std::to_string(D->n) + ", the scan count of the database handle");
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
    sc_size_runs(n_rtiles, A.n_ctiles, &A.run_tiles, &A.n_runs);
    const size_t n_partial = (size_t)n_rows * A.n_runs * k;
    if (n_partial > (size_t)INT_MAX) return sc_refuse(S, GORIO_ERR_UNSUPPORTED, "too many rows");
    // upload: rows | col_end
    const size_t b_rows = rows ? sc_align16(sizeof(int) * (size_t)n_rows) : 0, b_end = col_end ? sizeof(int) * (size_t)n_rows : 0;
    std::vector<char> blob(b_rows + b_end);
    if (rows) std::memcpy(blob.data(), rows, sizeof(int) * (size_t)n_rows);
    if (col_end) std::memcpy(blob.data() + b_rows, col_end, b_end);
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(Q->device));
    if (sc_reserve(Q, blob.size(), sizeof(gorio::ScBest) * (n_partial + n_out))) return GORIO_ERR_ALLOC;
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
    sc_charge(S, pairs, 2);
  }
  for (size_t i = 0; i < n_out; ++i) {
    index[i] = res[i].c;
    dist[i] = res[i].d;
    if (shift) shift[i] = res[i].s;
  }
  return GORIO_OK;
}

int gorio_sc_cross_detect(gorio_sc_t* Q, gorio_sc_t* D, int count, const int* qidx, const int* const* cands, const int* ncand, int* loop_id, float* yaw_rad, double* min_dist) {
  if (sc_check_handles(Q, D, "cross_detect")) return GORIO_ERR_INVALID;
  // no early return and no recent-keyframe filter: the indices of two sessions are unrelated
  return sc_detect_lists(sc_two_handles(Q, D, "cross_detect"), false, count, qidx, cands, ncand, loop_id, yaw_rad, min_dist);
}

int gorio_sc_cross_counters(const gorio_sc_t* Q, long long* calls, long long* pairs, long long* launches, long long* synchronisations) {
  if (!Q) return sc_fail(GORIO_ERR_INVALID, "cross_counters: null handle");
  return sc_read_counters(Q->cx, calls, pairs, launches, synchronisations);
}

}  // extern "C"
