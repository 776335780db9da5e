// apd_sc_pairs.hip -- exhaustive Scan Context matching (include/gorio_sc_pairs.h): listed pairs, whole matrices, best matches per row and
// detectLoopClosureID without its tree stage -- and everything those calls share with their two-handle forms of
// include/gorio_sc_cross.h: the kernels read the query side and the database side through two ScDb views, the host paths take an
// ScSides, and a same-handle call is the two-handle call with the handle given twice.  Included by apd_api.hip after apd_sc.hip, whose
// handle, database and per-pair function (sc_pair_eval) it uses.  An extension: the Go-RIO sources have no such mode (they score 3 tree
// picks per query, SC:294-348).
//
//   listed pairs     sc_pairs_kernel    one wave per (q, c) of a pair table, records read from global memory: sc_pair_kernel's body over
//                                       a table (distance_pairs, detect_exhaustive, cross_distance_pairs, cross_detect; the detects
//                                       follow it with sc_rowmin_kernel)
//   matrix tiles     sc_matrix_kernel   a workgroup stages 8 row and 8 column records in LDS once and evaluates the 64 pairs from there
//                                       (distance_matrix, cross_distance_matrix)
//   folding tiles    sc_tile_kernel     the same tile shape walking a run of column tiles of one database, keeping a running
//                                       (dist, index) per row instead of writing the pairs (best_matches)
//   row minimum      sc_rowmin_kernel   one wave per segment of items: the lexicographic (dist, position) minimum on doubles, of the column
//                                       runs' partial results (best_matches) or of a query's kept candidates (the detects)
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

// sc_pair_kernel's body over a pair table, the query side in dq and the candidate side in dd.
__global__ __launch_bounds__(kScThreads) void sc_pairs_kernel(const ScPairRef* __restrict__ pairs, int n_pairs, ScDb dq, ScDb dd, ScBest* __restrict__ out) {
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

// The tile shape of the matrix, folding and K-best kernels: 8 row records + 8 column records per workgroup, 1024 threads = 16 waves,
// wave w evaluating row w / 2 against columns 4 (w % 2) .. + 3, one pair at a time through sc_pair_eval.  A workgroup above 80 KB of LDS
// has its CU to itself, so the shape is the one that still gives every SIMD 4 waves: 16 records = 107,520 B, + 16 x 920 B of per-wave
// scratch, + indices (and fold slots).  LDS traffic is ds_read / ds_write only (no flat access), staging is global_load_dwordx4 +
// ds_write_b128.  Per pair the records cost 16 * 6720 / 64 = 1680 B of global traffic instead of the listed-pairs kernel's 13,440 B.
// The descriptor stays ring-major in LDS: in the column walk lane j reads [r * 20 + j], so across lanes the addresses are contiguous
// doubles (20 of them, 40 banks of 64) and the three shift groups read the same 20 addresses, which broadcast; the stride of 20 is only
// a lane's own step from one ring to the next.  No padding or transposition is needed for a conflict-free read.
// Partial tiles stage and evaluate only the entries that exist; indices may repeat (each slot holds its own copy).
struct ScMatrixArgs {
  const int* rows;  // index of row i in dq, or null: i
  const int* cols;  // index of column j in dd, or null: j
  int n_rows, n_cols;
  int n_ctiles;  // column tiles in all
  double* dist;  // either may be null: [n_rows][n_cols]
  int* shift;
};

// The matrix kernel: one (row tile, column tile) per workgroup, row records staged from dq and column records from dd, so both index
// lists are filled before one barrier and both record sets staged before the next.
//   LDS 122,304 B static, 65 VGPRs, scratch 0, no spills, 4 waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage).
__global__ __launch_bounds__(kScTileThreads) void sc_matrix_kernel(ScMatrixArgs A, ScDb dq, ScDb dd) {
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

struct ScFoldArgs {
  const int* rows;  // database index of row i, or null: i
  const int* cols;  // the same for columns; gorio_sc_best_matches leaves it null, see the kernel's note
  int n_rows, n_cols;
  int n_ctiles;     // column tiles in all
  int run_tiles;    // column tiles one workgroup walks
  int n_runs;       // runs per row tile
  int min_gap;      // pair (r, c) counts iff c <= r - min_gap
  ScBest* partial;  // [n_rows][n_runs]
};

// The folding kernel: a workgroup stages its row records once, walks a run of column tiles of the same database and keeps, in lane 0 of
// each wave, the best of the wave's row over the columns it has seen.
//   LDS 122,560 B static, 102 VGPRs, scratch 0, no spills, 4 waves per SIMD.  The two outer loops are kept rolled: unrolled, it spilled.
//   The column list is a kept line: without the A.cols branch the same report came out but best_matches measured 1.5 - 2 % slower at
//   1024 and 4096 rows, with it the times are the earlier ones (profiles/r30/sc_unify.md, section 3).
__global__ __launch_bounds__(kScTileThreads) void sc_tile_kernel(ScFoldArgs A, ScDb db) {
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
  int limit = -1;  // the largest column any row of this tile accepts
  for (int i = 0; i < nr; ++i) limit = max(limit, ridx[i] - A.min_gap);
  const int ri = w >> 1, cbase = (w & 1) * kScPairsPerWave;
  const double* R = rec + ri * kScRecord;
  // lane 0 of each wave: the best of this wave's row over the columns it has seen, in ascending column order
  double best_d = 10000000.0;
  int best_c = -1, best_s = 0;
  const int tc_end = min(A.n_ctiles, (run + 1) * A.run_tiles);
#pragma unroll 1
  for (int tc = run * A.run_tiles; tc < tc_end; ++tc) {
    const int c0 = tc * kScTileC, nc = min(kScTileC, A.n_cols - c0);
    if (c0 > limit) break;  // uniform over the workgroup
    __syncthreads();        // the previous tile's records and indices are no longer read
    if (t < nc) cidx[t] = A.cols ? A.cols[c0 + t] : c0 + t;
    __syncthreads();
    sc_stage_records(rec + kScTileR * kScRecord, cidx, nc, db, t);
    __syncthreads();
#pragma unroll 1
    for (int i = 0; i < kScPairsPerWave; ++i) {
      const int ci = cbase + i;
      const bool live = ri < nr && ci < nc && cidx[ci] <= ridx[ri] - A.min_gap;
      const double* C = rec + (kScTileR + ci) * kScRecord;
      double m = 0.0;
      int arg = 0;
      sc_pair_eval(live, lane, scratch[w], R + kScBins, C + kScBins, R + kScBins + kScSectors, C + kScBins + kScSectors, R, C, m, arg);
      if (live && lane == 0 && m < best_d) {  // strict: the lower column stays on a tie
        best_d = m;
        best_c = cidx[ci];
        best_s = arg;
      }
    }
  }
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

// ============================================================== host (include/gorio_sc_pairs.h and what include/gorio_sc_cross.h shares)
namespace {

// The two sides of a call.  Work runs on q's stream and in q's scratch buffers; d is only read, which is safe because the calls that
// add to a database synchronise before they return.  A call of gorio_sc_pairs.h has its handle on both sides.
struct ScSides {
  gorio_sc* q;                   // query side: rows, q[], query indices
  gorio_sc* d;                   // database side: columns, c[], candidates
  const char* fn;                // the call's name in messages
  bool cross;                    // the two-handle wording: a refusal says which handle it is about
  gorio_sc::Counters* counters;  // the group the call is charged to
};

ScSides sc_one_handle(gorio_sc* h, const char* fn) { return ScSides{h, h, fn, false, &h->px}; }
ScSides sc_two_handles(gorio_sc* Q, gorio_sc* D, const char* fn) { return ScSides{Q, D, fn, true, &Q->cx}; }

int sc_refuse(const ScSides& S, int code, const std::string& m) { return sc_fail(code, std::string(S.fn) + ": " + m); }

// prep + "the query handle" / "the database handle" in the two-handle wording, nothing in the same-handle one.
std::string sc_which(const ScSides& S, bool query_side, const char* prep) {
  return S.cross ? std::string(prep) + (query_side ? "the query handle" : "the database handle") : std::string();
}

// `what` (an argument, its position and its value) is no scan of its side.
int sc_not_added(const ScSides& S, bool query_side, const std::string& what, const std::string& at = "") {
  return sc_refuse(S, GORIO_ERR_INVALID, what + " has not been added" + sc_which(S, query_side, " to ") + " (" + std::to_string((query_side ? S.q : S.d)->n) + " scans)" + at);
}

// rows / cols on one side: null means 0 .. n_scans - 1 of that side's handle, so the extent must be its scan count; entries must have
// been added.
int sc_check_indices(const ScSides& S, bool query_side, const char* what, const int* idx, int n) {
  const gorio_sc* h = query_side ? S.q : S.d;
  if (!idx) {
    if (n != h->n)
      return sc_refuse(S, GORIO_ERR_INVALID, std::string("null ") + what + " means all " + std::to_string(h->n) + " scans" + sc_which(S, query_side, " of ") + ", but the extent is " + std::to_string(n));
    return GORIO_OK;
  }
  for (int i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= h->n) return sc_not_added(S, query_side, std::string(what) + "[" + std::to_string(i) + "] = " + std::to_string(idx[i]));
  return GORIO_OK;
}

// One finished call: it synchronised once.
void sc_charge(const ScSides& S, long long pairs, int launches) {
  S.counters->calls += 1;
  S.counters->pairs += pairs;
  S.counters->launches += launches;
  S.counters->syncs += 1;
}

int sc_read_counters(const gorio_sc::Counters& c, long long* calls, long long* pairs, long long* launches, long long* synchronisations) {
  if (calls) *calls = c.calls;
  if (pairs) *pairs = c.pairs;
  if (launches) *launches = c.launches;
  if (synchronisations) *synchronisations = c.syncs;
  return GORIO_OK;
}

// Grows the two scratch buffers of both headers' calls (by half beyond the need).
int sc_reserve(gorio_sc* h, size_t in_bytes, size_t out_bytes) {
  in_bytes = std::max<size_t>(in_bytes, 16), out_bytes = std::max<size_t>(out_bytes, 16);
  if (h->d_px_in.reserve(in_bytes, in_bytes + in_bytes / 2) != hipSuccess || h->d_px_out.reserve(out_bytes, out_bytes + out_bytes / 2) != hipSuccess)
    return sc_fail(GORIO_ERR_ALLOC, "device allocation failed (" + std::to_string(in_bytes + out_bytes) + " bytes)");
  return GORIO_OK;
}

size_t sc_align16(size_t b) { return (b + 15) / 16 * 16; }

// Column runs of the folding and K-best kernels: enough for about 2048 workgroups, so the partial results stay O(n_rows + 8 * 2048)
// entries per kept match.
void sc_size_runs(int n_rtiles, int n_ctiles, int* run_tiles, int* n_runs) {
  const int want_runs = std::min(n_ctiles, std::max(1, 2048 / n_rtiles));
  *run_tiles = (n_ctiles + want_runs - 1) / want_runs;
  *n_runs = (n_ctiles + *run_tiles - 1) / *run_tiles;
}

// The listed-pairs pass.  Evaluates every pair of the table and, given the ascending offsets of segments of it (one more than there
// are segments), reduces each segment to its first minimum; res receives one ScBest per pair, or one per segment.  One upload, 1 or 2
// launches, one copy back, one synchronisation.  An empty table touches neither the device nor the counters (nor res).
int sc_run_pairs(const ScSides& S, const std::vector<gorio::ScPairRef>& tab, const std::vector<int>& seg_off, gorio::ScBest* res) {
  if (tab.empty()) return GORIO_OK;
  gorio_sc* h = S.q;
  const int n_pairs = (int)tab.size(), n_seg = seg_off.empty() ? 0 : (int)seg_off.size() - 1;
  const size_t b_tab = sizeof(gorio::ScPairRef) * tab.size(), b_off = sizeof(int) * seg_off.size();
  std::vector<char> blob;  // table | offsets, put together only when there are offsets: a table alone goes up from where it lies
  if (n_seg) {
    blob.resize(b_tab + b_off);
    std::memcpy(blob.data(), tab.data(), b_tab);
    std::memcpy(blob.data() + b_tab, seg_off.data(), b_off);
  }
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (sc_reserve(h, b_tab + b_off, sizeof(gorio::ScBest) * ((size_t)n_pairs + n_seg))) return GORIO_ERR_ALLOC;
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, n_seg ? (const void*)blob.data() : (const void*)tab.data(), b_tab + b_off, hipMemcpyHostToDevice, h->stream));
  gorio::ScBest* items = (gorio::ScBest*)h->d_px_out.get();
  gorio::ScBest* d_res = n_seg ? items + n_pairs : items;
  hipLaunchKernelGGL(gorio::sc_pairs_kernel, dim3((unsigned)(((long long)n_pairs + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScPairRef*)h->d_px_in.get(), n_pairs,
                     S.q->db(), S.d->db(), items);
  if (n_seg)
    hipLaunchKernelGGL(gorio::sc_rowmin_kernel, dim3((unsigned)((n_seg + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScBest*)items,
                       (const int*)((const char*)h->d_px_in.get() + b_tab), n_seg, d_res);
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res, d_res, sizeof(gorio::ScBest) * (n_seg ? n_seg : n_pairs), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  sc_charge(S, n_pairs, n_seg ? 2 : 1);
  return GORIO_OK;
}

// gorio_sc_distance_pairs and gorio_sc_cross_distance_pairs, the handles checked.
int sc_distance_pairs(const ScSides& S, const int* q, const int* c, int count, double* dist, int* shift) {
  if (count < 0) return sc_refuse(S, GORIO_ERR_INVALID, "count < 0");
  if (count == 0) return GORIO_OK;
  if (!q || !c || !dist || !shift) return sc_refuse(S, GORIO_ERR_INVALID, "null argument");
  for (int k = 0; k < count; ++k) {
    const bool bad_q = q[k] < 0 || q[k] >= S.q->n, bad_c = c[k] < 0 || c[k] >= S.d->n;
    if (!S.cross && (bad_q || bad_c)) return sc_not_added(S, true, "pair " + std::to_string(k) + " = (" + std::to_string(q[k]) + ", " + std::to_string(c[k]) + ")");
    if (bad_q) return sc_not_added(S, true, "q[" + std::to_string(k) + "] = " + std::to_string(q[k]));
    if (bad_c) return sc_not_added(S, false, "c[" + std::to_string(k) + "] = " + std::to_string(c[k]));
  }
  std::vector<gorio::ScPairRef> tab(count);
  for (int k = 0; k < count; ++k) tab[k] = gorio::ScPairRef{q[k], c[k]};
  std::vector<gorio::ScBest> res(count);
  if (const int rc = sc_run_pairs(S, tab, {}, res.data())) return rc;
  for (int k = 0; k < count; ++k) {
    dist[k] = res[k].d;
    shift[k] = res[k].s;
  }
  return GORIO_OK;
}

// gorio_sc_distance_matrix and gorio_sc_cross_distance_matrix, the handles checked: one upload of the index lists that are given, one
// launch, one copy back per output, one synchronisation.
int sc_distance_matrix(const ScSides& S, const int* rows, int n_rows, const int* cols, int n_cols, double* dist, int* shift) {
  if (n_rows < 0 || n_cols < 0) return sc_refuse(S, GORIO_ERR_INVALID, "negative extent");
  if (n_rows == 0 || n_cols == 0) return GORIO_OK;
  if (!dist && !shift) return sc_refuse(S, GORIO_ERR_INVALID, "both outputs are null");
  if (sc_check_indices(S, true, "rows", rows, n_rows) || sc_check_indices(S, false, "cols", cols, n_cols)) return GORIO_ERR_INVALID;
  const long long total = (long long)n_rows * n_cols;
  if (total > (long long)INT_MAX) return sc_refuse(S, GORIO_ERR_UNSUPPORTED, std::to_string(n_rows) + " x " + std::to_string(n_cols) + " pairs exceed 2^31 - 1");
  gorio_sc* h = S.q;
  const size_t b_rows = rows ? sc_align16(sizeof(int) * n_rows) : 0, b_cols = cols ? sc_align16(sizeof(int) * n_cols) : 0;
  const size_t b_dist = dist ? sc_align16(sizeof(double) * total) : 0, b_shift = shift ? sizeof(int) * total : 0;
  std::vector<char> blob(b_rows + b_cols);
  if (rows) std::memcpy(blob.data(), rows, sizeof(int) * n_rows);
  if (cols) std::memcpy(blob.data() + b_rows, cols, sizeof(int) * n_cols);
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (sc_reserve(h, blob.size(), b_dist + b_shift)) return GORIO_ERR_ALLOC;
  if (!blob.empty()) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
  gorio::ScMatrixArgs A{};
  A.rows = rows ? (const int*)h->d_px_in.get() : nullptr;
  A.cols = cols ? (const int*)((const char*)h->d_px_in.get() + b_rows) : nullptr;
  A.n_rows = n_rows, A.n_cols = n_cols;
  A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
  A.dist = dist ? (double*)h->d_px_out.get() : nullptr;
  A.shift = shift ? (int*)((char*)h->d_px_out.get() + b_dist) : nullptr;
  const long long n_groups = (long long)((n_rows + gorio::kScTileR - 1) / gorio::kScTileR) * A.n_ctiles;  // <= 2^31 / 8 + n_rows + n_cols
  hipLaunchKernelGGL(gorio::sc_matrix_kernel, dim3((unsigned)n_groups), dim3(gorio::kScTileThreads), 0, h->stream, A, S.q->db(), S.d->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  if (dist) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(dist, A.dist, sizeof(double) * total, hipMemcpyDeviceToHost, h->stream));
  if (shift) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(shift, A.shift, sizeof(int) * total, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  sc_charge(S, total, 1);
  return GORIO_OK;
}

// detectLoopClosureID's tail for one query, from the best of its candidates and the query handle's parameters.
void sc_loop_from_best(const gorio_sc_params& p, const gorio::ScBest& o, int* loop_id, float* yaw_rad, double* min_dist) {
  const double unit = (p.azimuth_range - (-p.azimuth_range)) / double(GORIO_SC_SECTORS);  // PC_UNIT_SECTOR_ANGLE (SC:72)
  const int nn_idx = o.c < 0 ? 0 : o.c, nn_align = o.c < 0 ? 0 : o.s;                      // SC:312-314: the values the loop starts from
  *loop_id = o.d < p.sc_dist_thresh ? nn_idx : -1;                                         // SC:354-356
  const float deg = (float)(nn_align * unit);                                              // deg2rad(float degrees) (SC:18-21, 369)
  *yaw_rad = (float)((double)deg * M_PI / 180.0);
  *min_dist = o.d;
}

// gorio_sc_detect_exhaustive (exclude_recent: the early return of SC:284-288 and the filter of SC:294-306, which compare indices of
// one database) and gorio_sc_cross_detect (the lists as they are), the handles checked: a CSR of the kept candidates, one segment per
// query that is scored, then the listed-pairs pass with the row minimum.
int sc_detect_lists(const ScSides& S, bool exclude_recent, int count, const int* qidx, const int* const* cands, const int* ncand, int* loop_id, float* yaw_rad, double* min_dist) {
  if (count < 0) return sc_refuse(S, GORIO_ERR_INVALID, "count < 0");
  if (count == 0) return GORIO_OK;
  if (!qidx || !cands || !ncand || !loop_id || !yaw_rad || !min_dist) return sc_refuse(S, GORIO_ERR_INVALID, "null argument");
  size_t total = 0;
  for (int i = 0; i < count; ++i) {
    const std::string at = " (query " + std::to_string(i) + ")";
    if (qidx[i] < 0 || qidx[i] >= S.q->n) return sc_not_added(S, true, "query index " + std::to_string(qidx[i]), at);
    if (ncand[i] <= 0 || !cands[i]) return sc_refuse(S, GORIO_ERR_INVALID, "empty candidate list" + at);
    for (int j = 0; j < ncand[i]; ++j)
      if (cands[i][j] < 0 || cands[i][j] >= S.d->n) return sc_not_added(S, false, "candidate " + std::to_string(j) + " = " + std::to_string(cands[i][j]), at);
    total += ncand[i];
  }
  if (total > (size_t)INT_MAX) return sc_refuse(S, GORIO_ERR_UNSUPPORTED, "more than 2^31 - 1 candidates in all");
  std::vector<gorio::ScPairRef> tab;
  tab.reserve(total);
  std::vector<int> off(1, 0), seg(count, -1);
  for (int i = 0; i < count; ++i) {
    if (exclude_recent && qidx[i] < GORIO_SC_EXCLUDE_RECENT) continue;
    for (int j = 0; j < ncand[i]; ++j)  // size_t arithmetic (SC:300): a candidate after the query wraps and is kept
      if (!exclude_recent || (size_t)qidx[i] - (size_t)cands[i][j] >= (size_t)GORIO_SC_EXCLUDE_RECENT) tab.push_back(gorio::ScPairRef{qidx[i], cands[i][j]});
    seg[i] = (int)off.size() - 1;
    off.push_back((int)tab.size());
  }
  std::vector<gorio::ScBest> res(off.size(), gorio::ScBest{10000000.0, -1, 0});
  if (const int rc = sc_run_pairs(S, tab, off, res.data())) return rc;
  for (int i = 0; i < count; ++i) {
    if (seg[i] < 0) {  // SC:284-288
      loop_id[i] = -1;
      yaw_rad[i] = 0.0f;
      min_dist[i] = 10000000.0;
    } else {
      sc_loop_from_best(S.q->p, res[seg[i]], &loop_id[i], &yaw_rad[i], &min_dist[i]);
    }
  }
  return GORIO_OK;
}

}  // namespace

extern "C" {

int gorio_sc_distance_pairs(gorio_sc_t* h, const int* q, const int* c, int count, double* dist, int* shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "distance_pairs: null handle");
  return sc_distance_pairs(sc_one_handle(h, "distance_pairs"), q, c, count, dist, shift);
}

int gorio_sc_distance_matrix(gorio_sc_t* h, const int* rows, int n_rows, const int* cols, int n_cols, double* dist, int* shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "distance_matrix: null handle");
  return sc_distance_matrix(sc_one_handle(h, "distance_matrix"), rows, n_rows, cols, n_cols, dist, shift);
}

int gorio_sc_best_matches(gorio_sc_t* h, const int* rows, int n_rows, int min_gap, int* best_index, double* best_dist, int* best_shift) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "best_matches: null handle");
  const ScSides S = sc_one_handle(h, "best_matches");
  if (n_rows < 0) return sc_refuse(S, GORIO_ERR_INVALID, "negative extent");
  if (n_rows == 0) return GORIO_OK;
  if (!best_index || !best_dist) return sc_refuse(S, GORIO_ERR_INVALID, "null output");
  if (min_gap < 1) return sc_refuse(S, GORIO_ERR_INVALID, "min_gap = " + std::to_string(min_gap) + " must be >= 1");
  if (sc_check_indices(S, true, "rows", rows, n_rows)) return GORIO_ERR_INVALID;
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
    gorio::ScFoldArgs A{};
    A.n_rows = n_rows, A.n_cols = n_cols;
    A.n_ctiles = (n_cols + gorio::kScTileC - 1) / gorio::kScTileC;
    sc_size_runs(n_rtiles, A.n_ctiles, &A.run_tiles, &A.n_runs);
    A.min_gap = min_gap;
    const size_t n_partial = (size_t)n_rows * A.n_runs;
    if (n_partial > (size_t)INT_MAX) return sc_refuse(S, GORIO_ERR_UNSUPPORTED, "too many rows");
    // upload: segment offsets of the row minimum | rows
    const size_t b_off = sc_align16(sizeof(int) * ((size_t)n_rows + 1)), b_rows = rows ? sizeof(int) * (size_t)n_rows : 0;
    std::vector<char> blob(b_off + b_rows);
    int* off = (int*)blob.data();
    for (int i = 0; i <= n_rows; ++i) off[i] = i * A.n_runs;
    if (rows) std::memcpy(blob.data() + b_off, rows, b_rows);
    const size_t b_partial = sizeof(gorio::ScBest) * n_partial;
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
    if (sc_reserve(h, blob.size(), b_partial + sizeof(gorio::ScBest) * n_rows)) return GORIO_ERR_ALLOC;
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_px_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    A.rows = rows ? (const int*)((const char*)h->d_px_in.get() + b_off) : nullptr;
    A.partial = (gorio::ScBest*)h->d_px_out.get();
    gorio::ScBest* d_res = A.partial + n_partial;
    hipLaunchKernelGGL(gorio::sc_tile_kernel, dim3((unsigned)(n_rtiles * A.n_runs)), dim3(gorio::kScTileThreads), 0, h->stream, A, h->db());
    hipLaunchKernelGGL(gorio::sc_rowmin_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(gorio::kScThreads), 0, h->stream, (const gorio::ScBest*)A.partial,
                       (const int*)h->d_px_in.get(), n_rows, d_res);
    GORIO_HIP_CHECK(sc_fail, hipGetLastError());
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), d_res, sizeof(gorio::ScBest) * n_rows, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
    sc_charge(S, pairs, 2);
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
  return sc_detect_lists(sc_one_handle(h, "detect_exhaustive"), true, count, qidx, cands, ncand, loop_id, yaw_rad, min_dist);
}

int gorio_sc_pairs_counters(const gorio_sc_t* h, long long* calls, long long* pairs, long long* launches, long long* synchronisations) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "pairs_counters: null handle");
  return sc_read_counters(h->px, calls, pairs, launches, synchronisations);
}

}  // extern "C"
