// apd_sc_pairs.hip -- exhaustive Scan Context matching (include/gorio_sc_pairs.h): listed pairs, whole matrices, best matches per row and
// detectLoopClosureID without its tree stage.  Included by apd_api.hip after apd_sc.hip, whose handle, database and per-pair function
// (sc_pair_eval) it uses.  An extension: the Go-RIO sources have no such mode (they score 3 tree picks per query, SC:294-348).
//
//   listed pairs     sc_pairs_kernel    one wave per (q, c) of a pair table, records read from global memory: sc_pair_kernel's body over
//                                       a table (gorio_sc_distance_pairs, gorio_sc_detect_exhaustive)
//   tiles            sc_tile_kernel     a workgroup stages 8 row and 8 column records in LDS once and evaluates the 64 pairs from there
//                                       (gorio_sc_distance_matrix); in its folding form it walks a run of column tiles and keeps a running
//                                       (dist, index) per row instead of writing the pairs (gorio_sc_best_matches)
//   row minimum      sc_rowmin_kernel   one wave per segment of items: the lexicographic (dist, position) minimum on doubles, of the column
//                                       runs' partial results (best_matches) or of a query's kept candidates (detect_exhaustive)
// Every distance comes out of sc_pair_eval, so it has the bits gorio_sc_distance gives.  No floating-point atomics, no waits between
// workgroups; the order in which minima are folded is fixed by positions, not by timing.
#include <hip/hip_runtime.h>

#include <algorithm>

namespace gorio {

constexpr int kScTileR = GORIO_SC_TILE_ROWS, kScTileC = GORIO_SC_TILE_COLS;
constexpr int kScTileWaves = 16, kScTileThreads = 64 * kScTileWaves;
constexpr int kScRecord = kScBins + 2 * kScSectors;                  // doubles per staged record: descriptor, sector key, column norms (6720 B)
constexpr int kScPairsPerWave = kScTileR * kScTileC / kScTileWaves;  // 4
static_assert(kScThreads / 64 == GORIO_SC_PAIRS_PER_GROUP, "the header documents the pairs per workgroup of the listed-pairs kernel");
static_assert(kScTileWaves == 2 * kScTileR && kScPairsPerWave * 2 == kScTileC, "wave w owns row w / 2 and columns 4 (w % 2) .. + 3 of a tile");
static_assert(kScRecord % 2 == 0 && kScBins % 2 == 0 && kScSectors % 2 == 0, "records are staged in 16-byte pieces");

// One evaluated pair, or the best of several: d = 1e7 and c = -1 when nothing scored below 1e7.
struct ScBest {
  double d;
  int c, s;
};

struct ScPairRef {
  int q, c;
};

// sc_pair_kernel's body over a pair table.
__global__ __launch_bounds__(kScThreads) void sc_pairs_kernel(const ScPairRef* __restrict__ pairs, int n_pairs, ScDb db, ScBest* __restrict__ out) {
  __shared__ ScPairScratch scratch[kScThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long pair = (long long)blockIdx.x * (kScThreads / 64) + w;
  const bool live = pair < n_pairs;
  const ScPairRef P = live ? pairs[pair] : ScPairRef{0, 0};
  const size_t q = P.q, c = P.c;
  double m = 0.0;
  int arg = 0;
  sc_pair_eval(live, lane, scratch[w], db.sector + q * kScSectors, db.sector + c * kScSectors, db.colnorm + q * kScSectors, db.colnorm + c * kScSectors,
                           db.desc + q * kScBins, db.desc + c * kScBins, m, arg);
  if (live && lane == 0) out[pair] = ScBest{m, P.c, arg};
}

struct ScTileArgs {
  const int* rows;  // database index of row i, or null: i
  const int* cols;  // the same for columns
  int n_rows, n_cols;
  int n_ctiles;    // column tiles in all
  int run_tiles;   // column tiles one workgroup walks: 1 for the matrix
  int n_runs;      // runs per row tile
  int min_gap;     // folding form: pair (r, c) counts iff c <= r - min_gap
  double* dist;    // matrix form, either may be null: [n_rows][n_cols]
  int* shift;
  ScBest* partial;  // folding form: [n_rows][n_runs]
};

// Copies the records of `count` database entries into LDS in 16-byte pieces, all threads of the workgroup taking part.
__device__ __forceinline__ void sc_stage_records(double* lds, const int* idx, int count, const ScDb& db, int t) {
  constexpr int kPieces = kScRecord / 2, kDescPieces = kScBins / 2, kKeyPieces = kScSectors / 2;
  for (int i = t; i < count * kPieces; i += kScTileThreads) {
    const int rec = i / kPieces, k = i % kPieces;
    const size_t e = idx[rec];
    const double* src = k < kDescPieces ? db.desc + e * kScBins + 2 * k
                                        : (k < kDescPieces + kKeyPieces ? db.sector + e * kScSectors + 2 * (k - kDescPieces) : db.colnorm + e * kScSectors + 2 * (k - kDescPieces - kKeyPieces));
    *reinterpret_cast<double2*>(lds + rec * kScRecord + 2 * k) = *reinterpret_cast<const double2*>(src);
  }
}

// The tile kernel.  Shape: 8 row records + 8 column records per workgroup, 1024 threads = 16 waves, wave w evaluating row w / 2 against
// columns 4 (w % 2) .. + 3, one pair at a time through sc_pair_eval.  A workgroup above 80 KB of LDS has its CU to itself, so the shape is
// the one that still gives every SIMD 4 waves: 16 records = 107,520 B, + 16 x 920 B of per-wave scratch, + indices and fold slots.
//   kFold = false: LDS 122,304 B static, 94 VGPRs; kFold = true: LDS 122,560 B, 102 VGPRs; scratch 0, no spills, 4 waves per SIMD
//   (hipcc -Rpass-analysis=kernel-resource-usage).  LDS traffic is ds_read / ds_write only (no flat access), staging is
//   global_load_dwordx4 + ds_write_b128.  The two outer loops are kept rolled: unrolled, the folding form spilled.
// Per pair the records cost 16 * 6720 / 64 = 1680 B of global traffic instead of the listed-pairs kernel's 13,440 B.
// The descriptor stays ring-major in LDS: in the column walk lane j reads [r * 20 + j], so across lanes the addresses are contiguous
// doubles (20 of them, 40 banks of 64) and the three shift groups read the same 20 addresses, which broadcast; the stride of 20 is only
// a lane's own step from one ring to the next.  No padding or transposition is needed for a conflict-free read.
// Partial tiles stage and evaluate only the entries that exist; indices may repeat (each slot holds its own copy).
template <bool kFold>
__global__ __launch_bounds__(kScTileThreads) void sc_tile_kernel(ScTileArgs A, ScDb db) {
  __shared__ __attribute__((aligned(16))) double rec[(kScTileR + kScTileC) * kScRecord];
  __shared__ ScPairScratch scratch[kScTileWaves];
  __shared__ int ridx[kScTileR], cidx[kScTileC];
  __shared__ double fold_d[kScTileWaves];
  __shared__ int fold_c[kScTileWaves], fold_s[kScTileWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int tr = blockIdx.x / A.n_runs, run = blockIdx.x % A.n_runs;
  const int r0 = tr * kScTileR, nr = min(kScTileR, A.n_rows - r0);
  if (t < nr) ridx[t] = A.rows ? A.rows[r0 + t] : r0 + t;
  __syncthreads();
  sc_stage_records(rec, ridx, nr, db, t);
  int limit = 0;  // folding form: the largest column any row of this tile accepts
  if (kFold) {
    limit = -1;
    for (int i = 0; i < nr; ++i) limit = max(limit, ridx[i] - A.min_gap);
  }
  const int ri = w >> 1, cbase = (w & 1) * kScPairsPerWave;
  const double* R = rec + ri * kScRecord;
  // lane 0 of each wave: the best of this wave's row over the columns it has seen, in ascending column order
  double best_d = 10000000.0;
  int best_c = -1, best_s = 0;
  const int tc_end = min(A.n_ctiles, (run + 1) * A.run_tiles);
#pragma unroll 1
  for (int tc = run * A.run_tiles; tc < tc_end; ++tc) {
    const int c0 = tc * kScTileC, nc = min(kScTileC, A.n_cols - c0);
    if (kFold && c0 > limit) break;  // uniform over the workgroup
    __syncthreads();                  // the previous tile's records and indices are no longer read
    if (t < nc) cidx[t] = A.cols ? A.cols[c0 + t] : c0 + t;
    __syncthreads();
    sc_stage_records(rec + kScTileR * kScRecord, cidx, nc, db, t);
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < kScPairsPerWave; ++i) {
      const int ci = cbase + i;
      bool live = ri < nr && ci < nc;
      if (kFold) live = live && cidx[ci] <= ridx[ri] - A.min_gap;
      const double* C = rec + (kScTileR + ci) * kScRecord;
      double m = 0.0;
      int arg = 0;
      sc_pair_eval(live, lane, scratch[w], R + kScBins, C + kScBins, R + kScBins + kScSectors, C + kScBins + kScSectors, R, C, m, arg);
      if (live && lane == 0) {
        if (kFold) {
          if (m < best_d) {  // strict: the lower column stays on a tie
            best_d = m;
            best_c = cidx[ci];
            best_s = arg;
          }
        } else {
          const size_t o = (size_t)(r0 + ri) * A.n_cols + (c0 + ci);
          if (A.dist) A.dist[o] = m;
          if (A.shift) A.shift[o] = arg;
        }
      }
    }
  }
  if (kFold) {
    if (lane == 0) {
      fold_d[w] = best_d;
      fold_c[w] = best_c;
      fold_s[w] = best_s;
    }
    __syncthreads();
    if (t < nr) {  // the two waves of a row saw interleaved column groups: (dist, column) decides
      const int a = 2 * t, b = 2 * t + 1;
      const bool take_b = fold_c[b] >= 0 && (fold_c[a] < 0 || fold_d[b] < fold_d[a] || (fold_d[b] == fold_d[a] && fold_c[b] < fold_c[a]));
      const int k = take_b ? b : a;
      ScBest* o = A.partial + ((size_t)(r0 + t) * A.n_runs + run);
      o->d = fold_d[k];
      o->c = fold_c[k];
      o->s = fold_s[k];
    }
  }
}

// One wave per segment [seg_off[s], seg_off[s + 1]) of items: the item with the lexicographically smallest (d, position) among those
// below 1e7, {1e7, -1, 0} when there is none.  Compared as doubles: 1 - mean cosine can round below 0.  No item is NaN (sc_pair_eval
// returns 1e7 instead).
__global__ __launch_bounds__(kScThreads) void sc_rowmin_kernel(const ScBest* __restrict__ items, const int* __restrict__ seg_off, int n_seg, ScBest* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * (kScThreads / 64) + (threadIdx.x >> 6);
  if (s >= n_seg) return;
  const int b = seg_off[s], e = seg_off[s + 1];
  double bd = 10000000.0;
  int bp = INT_MAX;
  for (int p = b + lane; p < e; p += 64) {
    const double d = items[p].d;
    if (d < bd) {  // a lane's positions ascend: strict keeps the first
      bd = d;
      bp = p;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double od = __shfl_xor(bd, off, 64);
    const int op = __shfl_xor(bp, off, 64);
    if (od < bd || (od == bd && op < bp)) {
      bd = od;
      bp = op;
    }
  }
  if (lane == 0) out[s] = bp == INT_MAX ? ScBest{10000000.0, -1, 0} : items[bp];
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_sc_pairs.h)
namespace {

// Grows the two scratch buffers of this header's calls (by half beyond the need).
int scx_reserve(gorio_sc* h, size_t in_bytes, size_t out_bytes) {
  in_bytes = std::max<size_t>(in_bytes, 16), out_bytes = std::max<size_t>(out_bytes, 16);
  if (h->d_px_in.reserve(in_bytes, in_bytes + in_bytes / 2) != hipSuccess || h->d_px_out.reserve(out_bytes, out_bytes + out_bytes / 2) != hipSuccess)
    return sc_fail(GORIO_ERR_ALLOC, "device allocation failed (" + std::to_string(in_bytes + out_bytes) + " bytes)");
  return GORIO_OK;
}

// rows / cols of the matrix calls: null means 0 .. n_scans - 1, so the extent must be n_scans; entries must have been added.
int scx_check_indices(const gorio_sc* h, const char* fn, const char* what, const int* idx, int n) {
  if (!idx) {
    if (n != h->n)
      return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": null " + what + " means all " + std::to_string(h->n) + " scans, but the extent is " + std::to_string(n));
    return GORIO_OK;
  }
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= h->n)
      return sc_fail(GORIO_ERR_INVALID, std::string(fn) + ": " + what + "[" + std::to_string(i) + "] = " + std::to_string(idx[i]) + " has not been added (" + std::to_string(h->n) + " scans)");
  return GORIO_OK;
}

void scx_count(gorio_sc* h, long long pairs, int launches) {
  h->px_calls += 1;
  h->px_pairs += pairs;
  h->px_launches += launches;
  h->px_syncs += 1;
}

size_t scx_align16(size_t b) { return (b + 15) / 16 * 16; }

}  // namespace

extern "C" {

int gorio_sc_distance_pairs(gorio_sc_t* h, const int* q, const int* c, int count, double* dist, int* shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "distance_pairs: null handle");
  if (count < 0) return sc_fail(GORIO_ERR_INVALID, "distance_pairs: count < 0");
  if (count == 0) return GORIO_OK;
  if (!q || !c || !dist || !shift) return sc_fail(GORIO_ERR_INVALID, "distance_pairs: null argument");
  for (int k = 0; k < count; ++k)
    if (q[k] < 0 || q[k] >= h->n || c[k] < 0 || c[k] >= h->n)
      return sc_fail(GORIO_ERR_INVALID, "distance_pairs: pair " + std::to_string(k) + " = (" + std::to_string(q[k]) + ", " + std::to_string(c[k]) + ") has not been added (" +
                                            std::to_string(h->n) + " scans)");
  std::vector<gorio::ScPairRef> tab(count);
  for (int k = 0; k < count; ++k) tab[k] = gorio::ScPairRef{q[k], c[k]};
  std::vector<gorio::ScBest> res(count);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (scx_reserve(h, sizeof(gorio::ScPairRef) * tab.size(), sizeof(gorio::ScBest) * res.size())) return GORIO_ERR_ALLOC;
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, tab.data(), sizeof(gorio::ScPairRef) * tab.size(), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gorio::sc_pairs_kernel, dim3((unsigned)(((long long)count + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScPairRef*)h->d_px_in.get(), count, h->db(),
                     (gorio::ScBest*)h->d_px_out.get());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), h->d_px_out, sizeof(gorio::ScBest) * res.size(), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  scx_count(h, count, 1);
  for (int k = 0; k < count; ++k) {
    dist[k] = res[k].d;
    shift[k] = res[k].s;
  }
  return GORIO_OK;
}

int gorio_sc_distance_matrix(gorio_sc_t* h, const int* rows, int n_rows, const int* cols, int n_cols, double* dist, int* shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "distance_matrix: null handle");
  if (n_rows < 0 || n_cols < 0) return sc_fail(GORIO_ERR_INVALID, "distance_matrix: negative extent");
  if (n_rows == 0 || n_cols == 0) return GORIO_OK;
  if (!dist && !shift) return sc_fail(GORIO_ERR_INVALID, "distance_matrix: both outputs are null");
  if (scx_check_indices(h, "distance_matrix", "rows", rows, n_rows) || scx_check_indices(h, "distance_matrix", "cols", cols, n_cols)) return GORIO_ERR_INVALID;
  const long long total = (long long)n_rows * n_cols;
  if (total > (long long)INT_MAX)
    return sc_fail(GORIO_ERR_UNSUPPORTED, "distance_matrix: " + std::to_string(n_rows) + " x " + std::to_string(n_cols) + " pairs exceed 2^31 - 1");
  const size_t b_rows = rows ? scx_align16(sizeof(int) * n_rows) : 0, b_cols = cols ? scx_align16(sizeof(int) * n_cols) : 0;
  const size_t b_dist = dist ? scx_align16(sizeof(double) * total) : 0, b_shift = shift ? sizeof(int) * total : 0;
  std::vector<char> blob(b_rows + b_cols);
  if (rows) std::memcpy(blob.data(), rows, sizeof(int) * n_rows);
  if (cols) std::memcpy(blob.data() + b_rows, cols, sizeof(int) * n_cols);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (scx_reserve(h, blob.size(), b_dist + b_shift)) return GORIO_ERR_ALLOC;
  if (!blob.empty()) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
  gorio::ScTileArgs A{};
  A.rows = rows ? (const int*)h->d_px_in.get() : nullptr;
  A.cols = cols ? (const int*)((const char*)h->d_px_in.get() + b_rows) : nullptr;
  A.n_rows = n_rows, A.n_cols = n_cols;
  A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
  A.run_tiles = 1, A.n_runs = A.n_ctiles;
  A.dist = dist ? (double*)h->d_px_out.get() : nullptr;
  A.shift = shift ? (int*)((char*)h->d_px_out.get() + b_dist) : nullptr;
  const long long n_groups = (long long)((n_rows + gorio::kScTileR - 1) / gorio::kScTileR) * A.n_ctiles;  // <= 2^31 / 8 + n_rows + n_cols
  hipLaunchKernelGGL(gorio::sc_tile_kernel<false>, dim3((unsigned)n_groups), dim3(gorio::kScTileThreads), 0, h->stream, A, h->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  if (dist) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(dist, A.dist, sizeof(double) * total, hipMemcpyDeviceToHost, h->stream));
  if (shift) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(shift, A.shift, sizeof(int) * total, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  scx_count(h, total, 1);
  return GORIO_OK;
}

int gorio_sc_best_matches(gorio_sc_t* h, const int* rows, int n_rows, int min_gap, int* best_index, double* best_dist, int* best_shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "best_matches: null handle");
  if (n_rows < 0) return sc_fail(GORIO_ERR_INVALID, "best_matches: negative extent");
  if (n_rows == 0) return GORIO_OK;
  if (!best_index || !best_dist) return sc_fail(GORIO_ERR_INVALID, "best_matches: null output");
  if (min_gap < 1) return sc_fail(GORIO_ERR_INVALID, "best_matches: min_gap = " + std::to_string(min_gap) + " must be >= 1");
  if (scx_check_indices(h, "best_matches", "rows", rows, n_rows)) return GORIO_ERR_INVALID;
  int limit = -1;  // the largest column any row accepts
  long long pairs = 0;
  for (int i = 0; i < n_rows; ++i) {
    const int l = (rows ? rows[i] : i) - min_gap;
    limit = std::max(limit, l);
    if (l >= 0) pairs += l + 1;
  }
  std::vector<gorio::ScBest> res(n_rows, gorio::ScBest{10000000.0, -1, 0});
  if (limit >= 0) {
    const int n_cols = limit + 1, n_rtiles = (n_rows + gorio::kScTileR - 1) / gorio::kScTileR;
    gorio::ScTileArgs A{};
    A.n_rows = n_rows, A.n_cols = n_cols;
    A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
    // enough column runs for about 2048 workgroups, so the partial results stay O(n_rows + 8 * 2048)
    const int want_runs = std::min(A.n_ctiles, std::max(1, 2048 / n_rtiles));
    A.run_tiles = (A.n_ctiles + want_runs - 1) / want_runs;
    A.n_runs = (A.n_ctiles + A.run_tiles - 1) / A.run_tiles;
    A.min_gap = min_gap;
    const size_t n_partial = (size_t)n_rows * A.n_runs;
    if (n_partial > (size_t)INT_MAX) return sc_fail(GORIO_ERR_UNSUPPORTED, "best_matches: too many rows");
    // upload: segment offsets of the row minimum | rows
    const size_t b_off = scx_align16(sizeof(int) * ((size_t)n_rows + 1)), b_rows = rows ? sizeof(int) * (size_t)n_rows : 0;
    std::vector<char> blob(b_off + b_rows);
    int* off = (int*)blob.data();
    for (int i = 0; i <= n_rows; ++i) off[i] = i * A.n_runs;
    if (rows) std::memcpy(blob.data() + b_off, rows, b_rows);
    const size_t b_partial = sizeof(gorio::ScBest) * n_partial;
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
    if (scx_reserve(h, blob.size(), b_partial + sizeof(gorio::ScBest) * n_rows)) return GORIO_ERR_ALLOC;
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    A.rows = rows ? (const int*)((const char*)h->d_px_in.get() + b_off) : nullptr;
    A.partial = (gorio::ScBest*)h->d_px_out.get();
    gorio::ScBest* d_res = A.partial + n_partial;
    hipLaunchKernelGGL(gorio::sc_tile_kernel<true>, dim3((unsigned)(n_rtiles * A.n_runs)), dim3(gorio::kScTileThreads), 0, h->stream, A, h->db());
    hipLaunchKernelGGL(gorio::sc_rowmin_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScBest*)A.partial,
                       (const int*)h->d_px_in.get(), n_rows, d_res);
    GORIO_HIP_CHECK(sc_fail, hipGetLastError());
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), d_res, sizeof(gorio::ScBest) * n_rows, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
    scx_count(h, pairs, 2);
  }
  for (int i = 0; i < n_rows; ++i) {
    best_index[i] = res[i].c;
    best_dist[i] = res[i].d;
    if (best_shift) best_shift[i] = res[i].s;
  }
  return GORIO_OK;
}

int gorio_sc_detect_exhaustive(gorio_sc_t* h, int count, const int* qidx, const int* const* cands, const int* ncand, int* loop_id, float* yaw_rad, double* min_dist) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: null handle");
  if (count < 0) return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: count < 0");
  if (count == 0) return GORIO_OK;
  if (!qidx || !cands || !ncand || !loop_id || !yaw_rad || !min_dist) return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: null argument");
  size_t total = 0;
  for (int i = 0; i < count; ++i) {
    const std::string at = " (query " + std::to_string(i) + ")";
    if (qidx[i] < 0 || qidx[i] >= h->n)
      return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: query index " + std::to_string(qidx[i]) + " has not been added (" + std::to_string(h->n) + " scans)" + at);
    if (ncand[i] <= 0 || !cands[i]) return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: empty candidate list" + at);
    for (int j = 0; j < ncand[i]; ++j)
      if (cands[i][j] < 0 || cands[i][j] >= h->n)
        return sc_fail(GORIO_ERR_INVALID, "detect_exhaustive: candidate " + std::to_string(j) + " = " + std::to_string(cands[i][j]) + " has not been added" + at);
    total += ncand[i];
  }
  if (total > (size_t)INT_MAX) return sc_fail(GORIO_ERR_UNSUPPORTED, "detect_exhaustive: more than 2^31 - 1 candidates in all");
  // CSR of the kept candidates: one segment per query that passes the early return (SC:284-288), the filter of SC:294-306 on its list
  std::vector<gorio::ScPairRef> tab;
  std::vector<int> off(1, 0), seg(count, -1);
  for (int i = 0; i < count; ++i) {
    if (qidx[i] < GORIO_SC_EXCLUDE_RECENT) continue;
    for (int j = 0; j < ncand[i]; ++j)  // size_t arithmetic (SC:300): a candidate after the query wraps and is kept
      if ((size_t)qidx[i] - (size_t)cands[i][j] >= (size_t)GORIO_SC_EXCLUDE_RECENT) tab.push_back(gorio::ScPairRef{qidx[i], cands[i][j]});
    seg[i] = (int)off.size() - 1;
    off.push_back((int)tab.size());
  }
  const int n_seg = (int)off.size() - 1, n_pairs = (int)tab.size();
  std::vector<gorio::ScBest> res(std::max(n_seg, 1), gorio::ScBest{10000000.0, -1, 0});
  if (n_pairs) {
    const size_t b_tab = scx_align16(sizeof(gorio::ScPairRef) * tab.size()), b_off = sizeof(int) * off.size();
    std::vector<char> blob(b_tab + b_off);
    std::memcpy(blob.data(), tab.data(), sizeof(gorio::ScPairRef) * tab.size());
    std::memcpy(blob.data() + b_tab, off.data(), b_off);
    const size_t b_items = sizeof(gorio::ScBest) * tab.size();
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
    if (scx_reserve(h, blob.size(), b_items + sizeof(gorio::ScBest) * n_seg)) return GORIO_ERR_ALLOC;
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    gorio::ScBest* items = (gorio::ScBest*)h->d_px_out.get();
    gorio::ScBest* d_res = items + tab.size();
    hipLaunchKernelGGL(gorio::sc_pairs_kernel, dim3((unsigned)(((long long)n_pairs + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScPairRef*)h->d_px_in.get(), n_pairs,
                       h->db(), items);
    hipLaunchKernelGGL(gorio::sc_rowmin_kernel, dim3((unsigned)((n_seg + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScBest*)items,
                       (const int*)((const char*)h->d_px_in.get() + b_tab), n_seg, d_res);
    GORIO_HIP_CHECK(sc_fail, hipGetLastError());
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), d_res, sizeof(gorio::ScBest) * n_seg, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
    scx_count(h, n_pairs, 2);
  }
  const double unit = (h->p.azimuth_range - (-h->p.azimuth_range)) / double(GORIO_SC_SECTORS);  // PC_UNIT_SECTOR_ANGLE (SC:72)
  for (int i = 0; i < count; ++i) {
    if (seg[i] < 0) {  // SC:284-288
      loop_id[i] = -1;
      yaw_rad[i] = 0.0f;
      min_dist[i] = 10000000.0;
      continue;
    }
    const gorio::ScBest& o = res[seg[i]];
    const int nn_idx = o.c < 0 ? 0 : o.c, nn_align = o.c < 0 ? 0 : o.s;  // SC:312-314: the values the loop starts from
    loop_id[i] = o.d < h->p.sc_dist_thresh ? nn_idx : -1;                // SC:354-356
    const float deg = (float)(nn_align * unit);                          // deg2rad(float degrees) (SC:18-21, 369)
    yaw_rad[i] = (float)((double)deg * M_PI / 180.0);
    min_dist[i] = o.d;
  }
  return GORIO_OK;
}

int gorio_sc_pairs_counters(const gorio_sc_t* h, long long* calls, long long* pairs, long long* launches, long long* synchronisations) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "pairs_counters: null handle");
  if (calls) *calls = h->px_calls;
  if (pairs) *pairs = h->px_pairs;
  if (launches) *launches = h->px_launches;
  if (synchronisations) *synchronisations = h->px_syncs;
  return GORIO_OK;
}

}  // extern "C"
