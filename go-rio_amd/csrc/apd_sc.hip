// apd_sc.hip -- Intensity Scan Context loop-candidate search (include/gorio_sc.h), SCManager of the Go-RIO back end.
// Included by apd_api.hip after apd_ground.hip.
//
// SC = src/radar_graph_slam/Scancontext.cpp, NF = include/scan_context/nanoflann.hpp (v1.3.2) of the Go-RIO sources.
//   descriptors + keys   sc_descriptor_kernel  one workgroup per scan: scatter-max of the intensities into a 40 x 20 LDS grid
//                                              (atomicMax on an order-preserving int encoding), the -1000 / 0 rule, ring key,
//                                              sector key and column norms (SC:162-247)
//   ring-key k-NN        sc_knn_kernel         one workgroup per chunk of a query's snapshot: float distances in NF's grouped
//                                              order (NF:383-406), per-lane top 3 on (distance, position), wave64 + LDS merge
//                        sc_knn_merge_kernel   one wave per query: merges the chunks' top 3s, maps the positions through the
//                                              query's CURRENT candidate list (SC:330-338)
//   SC distance          sc_pair_kernel        one wave per (query, candidate): 20-shift sector-key alignment, then 3 shifts x 20
//                                              columns of double cosines (SC:80-160); its body is sc_pair_eval, which the kernels of
//                                              apd_sc_pairs.hip (include/gorio_sc_pairs.h) call too
//   counter, snapshots   host                  which snapshot each query sees follows from the inputs alone (SC:284-306)
//   final decision       host                  strict minimum over <= 3 distances, threshold, yaw (SC:341-371)
// Every sum runs in index order (Eigen's reduction order is not pinned by the reference), un-fused (-ffp-contract=off), so the
// descriptors, keys and k-NN distances are bit-identical to tests/sc_restatement.py.
#include <hip/hip_runtime.h>

#include <algorithm>

namespace gorio {

constexpr int kScRings = 40, kScSectors = 20, kScBins = kScRings * kScSectors;
constexpr int kScThreads = 256;     // 4 waves
constexpr int kScKnnChunk = 2048;   // snapshot positions per k-NN workgroup (8 per lane)

struct ScDb {
  double* desc;     // [n][800], ring-major (desc[ring * 20 + sector])
  double* ring;     // [n][40]  ring key (row mean)
  double* sector;   // [n][20]  sector key (column mean)
  double* colnorm;  // [n][20]  column norms, for distDirectSC
  float* ringf;     // [n][40]  ring key cast to float, what the kd-tree holds (eig2stdvec, SC:73-77)
};

struct ScChunk {
  int qdb, snap_off, begin, end;  // query's database index, its snapshot in the index pool, positions [begin, end)
};

struct ScQuery {
  int qdb, chunk_off, n_chunks, cand_off, n_cand;
};

struct ScHit {
  float d;
  int p;
};

// Per query: the k-NN result (NF) and the <= 3 SC distances.  The pair kernel reads (qdb, kf[k]) and writes dist[k], shift[k].
struct ScOut {
  int qdb, n_found;
  int pos[3], kf[3], shift[3];
  float keyd[3];
  double dist[3];
};

// Order-preserving int encoding of a non-NaN float: signed comparison of the codes is float comparison, -0 < +0.
__device__ inline int sc_code(float f) {
  const int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ inline float sc_decode(int k) { return __int_as_float(k >= 0 ? k : k ^ 0x7fffffff); }

// ring or sector index: std::max(std::min(N, int(ceil(v))), 1) (SC:193-195).  int(NaN) is INT_MIN on x86, which clamps to 1;
// the conversion is undefined behaviour on the device, so NaN is mapped explicitly.
__device__ inline int sc_clamp_index(double v, int n) {
  if (v != v) return 1;
  const double c = ceil(v);
  return c >= n ? n : (c < 1 ? 1 : (int)c);
}

// makeScancontext + makeRingkeyFromScancontext + makeSectorkeyFromScancontext for one scan per workgroup.
// pts: (x, y, intensity, -) of all scans back to back; scan_off[count + 1].
__global__ __launch_bounds__(kScThreads) void sc_descriptor_kernel(const float4* __restrict__ pts, const int* __restrict__ scan_off, int first, double range, ScDb db) {
  __shared__ int bins[kScBins];
  __shared__ double d[kScBins];
  const int s = blockIdx.x, t = threadIdx.x;
  const int b = scan_off[s], e = scan_off[s + 1];
  const int start = sc_code(-1000.0f);  // NO_POINT (SC:170-171)
  for (int i = t; i < kScBins; i += kScThreads) bins[i] = start;
  __syncthreads();
  for (int i = b + t; i < e; i += kScThreads) {
    const float4 p = pts[i];
    const float x = p.x, y = p.y, inten = p.z;
    // desc < intensity (SC:201, strict, in double): NaN never updates, nor does anything <= the start value
    if (!(inten > -1000.0f)) continue;
    const float rr = sqrtf(x * x + y * y);  // SC:183, float
    // SC:185: atan2f (taken as correctly rounded), then double, stored as float
    const float az = (float)(((double)(float)atan2((double)x, (double)y) - M_PI_2) * 180.0 / M_PI);
    if ((double)fabsf(az) > range) continue;  // SC:187, the float abs
    if ((double)rr > 80.0) continue;          // SC:190; NaN passes, +inf is skipped
    const int ring = sc_clamp_index((double)rr / 80.0 * 40.0, kScRings);                  // SC:193
    const int sec = sc_clamp_index(((double)az - (-range)) / (range - (-range)) * 20.0, kScSectors);  // SC:195
    atomicMax(&bins[(ring - 1) * kScSectors + (sec - 1)], sc_code(inten));
  }
  __syncthreads();
  const size_t o = (size_t)(first + s);
  for (int i = t; i < kScBins; i += kScThreads) {
    const int k = bins[i];
    const double v = k == start ? 0.0 : (double)sc_decode(k);  // SC:205-209
    d[i] = v;
    db.desc[o * kScBins + i] = v;
  }
  __syncthreads();
  if (t < kScRings) {  // row mean (SC:219-229), index order
    double sum = 0.0;
    for (int c = 0; c < kScSectors; ++c) sum += d[t * kScSectors + c];
    const double m = sum / (double)kScSectors;
    db.ring[o * kScRings + t] = m;
    db.ringf[o * kScRings + t] = (float)m;
  } else if (t >= 64 && t < 64 + kScSectors) {  // column mean (SC:235-245) and column norm, index order
    const int c = t - 64;
    double sum = 0.0, sq = 0.0;
    for (int r = 0; r < kScRings; ++r) {
      const double v = d[r * kScSectors + c];
      sum += v;
      sq += v * v;
    }
    db.sector[o * kScSectors + c] = sum / (double)kScRings;
    db.colnorm[o * kScSectors + c] = sqrt(sq);
  }
}

// (d, p) < (d', p'): ascending distance, the lower snapshot position first on ties.
__device__ inline bool sc_less(float da, int pa, float db, int pb) { return da < db || (da == db && pa < pb); }

struct ScTop3 {
  float d[3];
  int p[3];
  __device__ void init() {
    for (int k = 0; k < 3; ++k) {
      d[k] = INFINITY;
      p[k] = INT_MAX;
    }
  }
  __device__ void insert(float dd, int pp) {
    if (!sc_less(dd, pp, d[2], p[2])) return;
    if (sc_less(dd, pp, d[1], p[1])) {
      d[2] = d[1];
      p[2] = p[1];
      if (sc_less(dd, pp, d[0], p[0])) {
        d[1] = d[0];
        p[1] = p[0];
        d[0] = dd;
        p[0] = pp;
      } else {
        d[1] = dd;
        p[1] = pp;
      }
    } else {
      d[2] = dd;
      p[2] = pp;
    }
  }
  // every lane of the wave ends with the top 3 of the union
  __device__ void wave_reduce() {
    for (int off = 32; off > 0; off >>= 1) {
      float od[3];
      int op[3];
      for (int k = 0; k < 3; ++k) {
        od[k] = __shfl_xor(d[k], off, 64);
        op[k] = __shfl_xor(p[k], off, 64);
      }
      for (int k = 0; k < 3; ++k) insert(od[k], op[k]);
    }
  }
};

// The ring-key k-NN over one chunk of a query's snapshot.  The kd-tree (NF) is exact with eps = 0, and its leaves evaluate the
// full distance (NF:1358-1361), so a brute force in the same float order finds the same entries.  A distance not below FLT_MAX
// never enters (dist < worstDist(), which is FLT_MAX until three entries are in).
__global__ __launch_bounds__(kScThreads) void sc_knn_kernel(const ScChunk* __restrict__ chunks, const int* __restrict__ pool, const float* __restrict__ ringf,
                                                            ScHit* __restrict__ partial) {
  __shared__ float q[kScRings];
  __shared__ ScHit wave_top[kScThreads / 64][3];
  const ScChunk c = chunks[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (t < kScRings) q[t] = ringf[(size_t)c.qdb * kScRings + t];
  __syncthreads();
  ScTop3 top;
  top.init();
  for (int p = c.begin + t; p < c.end; p += kScThreads) {
    const float4* k4 = reinterpret_cast<const float4*>(ringf + (size_t)pool[c.snap_off + p] * kScRings);
    float res = 0.0f;
    for (int g = 0; g < kScRings / 4; ++g) {  // L2_Adaptor::evalMetric (NF:383-406): four components per group
      const float4 k = k4[g];
      const float d0 = q[4 * g] - k.x, d1 = q[4 * g + 1] - k.y, d2 = q[4 * g + 2] - k.z, d3 = q[4 * g + 3] - k.w;
      res += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    if (res < FLT_MAX) top.insert(res, p);
  }
  top.wave_reduce();
  if (lane == 0)
    for (int k = 0; k < 3; ++k) wave_top[w][k] = ScHit{top.d[k], top.p[k]};
  __syncthreads();
  if (t == 0) {
    for (int ww = 1; ww < kScThreads / 64; ++ww)
      for (int k = 0; k < 3; ++k) top.insert(wave_top[ww][k].d, wave_top[ww][k].p);
    for (int k = 0; k < 3; ++k) partial[(size_t)blockIdx.x * 3 + k] = ScHit{top.d[k], top.p[k]};
  }
}

// One wave per query: the top 3 over the query's chunks, as KNNResultSet leaves them (NF:158-190): unfound positions 0 (the index
// vector is zero-initialised), unfound distances 0 except the last, which init sets to FLT_MAX.  Then SC:330-338: a position beyond
// the current candidate list is skipped, the others name candidate_keyframe_indices[position].
__global__ __launch_bounds__(64) void sc_knn_merge_kernel(const ScQuery* __restrict__ queries, const ScHit* __restrict__ partial, const int* __restrict__ pool,
                                                          ScOut* __restrict__ out) {
  const ScQuery Q = queries[blockIdx.x];
  const int lane = threadIdx.x;
  ScTop3 top;
  top.init();
  for (int i = Q.chunk_off + lane; i < Q.chunk_off + Q.n_chunks; i += 64)
    for (int k = 0; k < 3; ++k) top.insert(partial[(size_t)i * 3 + k].d, partial[(size_t)i * 3 + k].p);
  top.wave_reduce();
  if (lane == 0) {
    ScOut o;
    o.qdb = Q.qdb;
    o.n_found = 0;
    for (int k = 0; k < 3; ++k) {
      const bool found = top.p[k] != INT_MAX;
      o.n_found += found;
      o.pos[k] = found ? top.p[k] : 0;
      o.keyd[k] = found ? top.d[k] : (k == 2 ? FLT_MAX : 0.0f);
      o.kf[k] = o.pos[k] > Q.n_cand - 1 ? -1 : pool[Q.cand_off + o.pos[k]];
      o.shift[k] = -1;
      o.dist[k] = __longlong_as_double(0x7ff8000000000000LL);
    }
    out[blockIdx.x] = o;
  }
}

// Per-wave LDS scratch of sc_pair_eval.
struct ScPairScratch {
  double vnorm[kScSectors];
  double sim[3][kScSectors];
  double sdist[3];
  int eff[3][kScSectors];
  int shifts[3];
  int pad;
};

// distanceBtnScanContext(q, c) (SC:127-160) by one wave; every kernel that needs the distance calls this one function, which is what
// makes the batched forms (apd_sc_pairs.hip) bit-identical to gorio_sc_distance.  vq / vc: sector keys, nq / nc: column norms, dq / dc:
// descriptors, ring-major as in the database; global memory or LDS.  EVERY thread of the workgroup must call it
// (it synchronises the workgroup between its stages), waves without a pair with live = false.  Lane 0 of a live wave returns the result.
__device__ __forceinline__ void sc_pair_eval(bool live, int lane, ScPairScratch& S, const double* vq, const double* vc, const double* nq, const double* nc,
                                             const double* dq0, const double* dc0, double& dist, int& shift) {
  // fastAlignUsingVkey (SC:104-122): ||vkey_q - circshift(vkey_c, s)||, circshift moving column j to (j + s) mod 20 (SC:42-62)
  if (live && lane < kScSectors) {
    double sq = 0.0;
    for (int j = 0; j < kScSectors; ++j) {
      const double diff = vq[j] - vc[(j - lane + kScSectors) % kScSectors];
      sq += diff * diff;
    }
    S.vnorm[lane] = sqrt(sq);
  }
  __syncthreads();
  if (live && lane == 0) {
    int a = 0;
    double m = 10000000.0;
    for (int s = 0; s < kScSectors; ++s)
      if (S.vnorm[s] < m) {
        a = s;
        m = S.vnorm[s];
      }
    // SEARCH_RADIUS = round(0.5 * 0.1 * 20) = 1: {a, a + 1, a - 1} mod 20, sorted ascending (SC:134-141)
    int s0 = a, s1 = (a + 1) % kScSectors, s2 = (a - 1 + kScSectors) % kScSectors, tmp;
    if (s1 < s0) { tmp = s0; s0 = s1; s1 = tmp; }
    if (s2 < s1) { tmp = s1; s1 = s2; s2 = tmp; }
    if (s1 < s0) { tmp = s0; s0 = s1; s1 = tmp; }
    S.shifts[0] = s0;
    S.shifts[1] = s1;
    S.shifts[2] = s2;
  }
  __syncthreads();
  // distDirectSC (SC:80-101) column terms: lane = 20 k + j, column j of the query against column j of the shifted candidate
  if (live && lane < 3 * kScSectors) {
    const int k = lane / kScSectors, j = lane % kScSectors;
    const int cj = (j - S.shifts[k] + kScSectors) % kScSectors;
    const double n1 = nq[j], n2 = nc[cj];
    int ok = 0;
    double sv = 0.0;
    if (!((n1 == 0) | (n2 == 0))) {
      const double* dq = dq0 + j;
      const double* dc = dc0 + cj;
      double dot = 0.0;
      for (int r = 0; r < kScRings; ++r) dot += dq[r * kScSectors] * dc[r * kScSectors];
      sv = dot / (n1 * n2);
      ok = 1;
    }
    S.sim[k][j] = sv;
    S.eff[k][j] = ok;
  }
  __syncthreads();
  if (live && lane < 3) {
    double sum = 0.0;
    int n_eff = 0;
    for (int j = 0; j < kScSectors; ++j)
      if (S.eff[lane][j]) {
        sum = sum + S.sim[lane][j];
        n_eff = n_eff + 1;
      }
    S.sdist[lane] = 1.0 - sum / (double)n_eff;  // no effective column: 0 / 0 = NaN
  }
  __syncthreads();
  if (live && lane == 0) {
    int arg = 0;
    double m = 10000000.0;
    for (int k = 0; k < 3; ++k)
      if (S.sdist[k] < m) {  // strict, a NaN never wins (SC:144-157)
        arg = S.shifts[k];
        m = S.sdist[k];
      }
    dist = m;
    shift = arg;
  }
}

// distanceBtnScanContext(desc[qdb], desc[kf]) (SC:127-160) for pair k of out[i], pair index = 3 i + k; one wave per pair.
__global__ __launch_bounds__(kScThreads) void sc_pair_kernel(ScOut* __restrict__ out, int n_pairs, ScDb db) {
  __shared__ ScPairScratch scratch[kScThreads / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int pair = blockIdx.x * (kScThreads / 64) + w;
  const bool active = pair < n_pairs;
  int q = -1, c = -1;
  if (active) {
    q = out[pair / 3].qdb;
    c = out[pair / 3].kf[pair % 3];
  }
  const bool live = active && c >= 0;
  const size_t qq = live ? q : 0, cc = live ? c : 0;
  double m = 0.0;
  int arg = 0;
  sc_pair_eval(live, lane, scratch[w], db.sector + qq * kScSectors, db.sector + cc * kScSectors, db.colnorm + qq * kScSectors, db.colnorm + cc * kScSectors,
                           db.desc + qq * kScBins, db.desc + cc * kScBins, m, arg);
  if (live && lane == 0) {
    out[pair / 3].dist[pair % 3] = m;
    out[pair / 3].shift[pair % 3] = arg;
  }
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_sc.h)
struct gorio_sc {
  int device = 0;
  hipStream_t stream = nullptr;
  gorio_sc_params p;
  // SCManager state
  int n = 0;                  // scans added
  int counter = 0;            // tree_making_period_conter
  std::vector<int> snapshot;  // polarcontext_invkeys_to_search_ as database indices
  // database: five arrays of one capacity db_cap (scans); db() is the view the kernels take
  gorio::DevBuf<double> db_desc, db_ring, db_sector, db_colnorm;
  gorio::DevBuf<float> db_ringf;
  size_t db_cap = 0;
  gorio::ScDb db() const { return gorio::ScDb{db_desc, db_ring, db_sector, db_colnorm, db_ringf}; }
  // scratch
  gorio::DevBuf<void> d_in;
  gorio::DevBuf<gorio::ScHit> d_partial;
  gorio::DevBuf<gorio::ScOut> d_out;
  gorio::DevBuf<void> d_kfjobs;  // gorio_sc_add_keyframes (apd_keyframes.hip): the pack kernel's job table
  // include/gorio_sc_pairs.h and include/gorio_sc_cross.h (apd_sc_pairs.hip, apd_sc_cross.hip): the upload and the device results of
  // either header's calls, and one group of cumulative counters each (cx: the calls this handle made as the query handle)
  gorio::DevBuf<void> d_px_in, d_px_out;
  struct Counters {
    long long calls = 0, pairs = 0, launches = 0, syncs = 0;
  } px, cx;
};

namespace {
thread_local std::string g_sc_err;
int sc_fail(int code, const std::string& m) {
  g_sc_err = m;
  return code;
}

// Grows the database to hold `need` scans, keeping what is there.
int sc_grow_db(gorio_sc* h, size_t need) {
  if (need <= h->db_cap) return GORIO_OK;
  const size_t cap = std::max(need + need / 2, (size_t)64);
  // new buffers, copy, then move-assign: the old database stays whole until the new one is (an early return frees the new buffers)
  gorio::DevBuf<double> desc, ring, sector, colnorm;
  gorio::DevBuf<float> ringf;
  size_t new_cap = 0;
  if (gorio::reserve_group(new_cap, cap, cap, desc, gorio::kScBins * cap, ring, gorio::kScRings * cap, sector, gorio::kScSectors * cap, colnorm, gorio::kScSectors * cap,
                           ringf, gorio::kScRings * cap) != hipSuccess)
    return sc_fail(GORIO_ERR_NO_DEVICE, "add_scans: device allocation failed");
  if (h->n) {
    const size_t n = h->n;
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(desc, h->db_desc, sizeof(double) * gorio::kScBins * n, hipMemcpyDeviceToDevice, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(ring, h->db_ring, sizeof(double) * gorio::kScRings * n, hipMemcpyDeviceToDevice, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(sector, h->db_sector, sizeof(double) * gorio::kScSectors * n, hipMemcpyDeviceToDevice, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(colnorm, h->db_colnorm, sizeof(double) * gorio::kScSectors * n, hipMemcpyDeviceToDevice, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(ringf, h->db_ringf, sizeof(float) * gorio::kScRings * n, hipMemcpyDeviceToDevice, h->stream));
  }
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  h->db_desc = std::move(desc), h->db_ring = std::move(ring), h->db_sector = std::move(sector), h->db_colnorm = std::move(colnorm), h->db_ringf = std::move(ringf);
  h->db_cap = cap;
  return GORIO_OK;
}

void sc_diag_early(gorio_sc_diag* d, int counter) {
  *d = gorio_sc_diag{};
  d->early_return = 1;
  d->counter = counter;
  for (int k = 0; k < 3; ++k) {
    d->keyframe[k] = -1;
    d->sc_dist[k] = NAN;
    d->sc_shift[k] = -1;
  }
}

// One device pass over the non-early queries: upload, k-NN chunks, merge + mapping, pair distances, one copy back.
int sc_detect_run(gorio_sc* h, int count, const int* qidx, const int* const* cands, const int* ncand, int* loop_id, float* yaw_rad, double* min_dist, gorio_sc_diag* diag) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "detect: null handle");
  if (count <= 0 || !qidx || !cands || !ncand || !loop_id || !yaw_rad || !min_dist) return sc_fail(GORIO_ERR_INVALID, "detect: null argument or count <= 0");
  for (int i = 0; i < count; ++i) {
    const std::string at = count > 1 ? " (query " + std::to_string(i) + ")" : "";
    if (qidx[i] < 0 || qidx[i] >= h->n)
      return sc_fail(GORIO_ERR_INVALID, "detect: query index " + std::to_string(qidx[i]) + " has not been added (" + std::to_string(h->n) + " scans)" + at);
    if (ncand[i] <= 0 || !cands[i]) return sc_fail(GORIO_ERR_INVALID, "detect: empty candidate list" + at);
    for (int j = 0; j < ncand[i]; ++j)
      if (cands[i][j] < 0 || cands[i][j] >= h->n)
        return sc_fail(GORIO_ERR_INVALID, "detect: candidate " + std::to_string(j) + " = " + std::to_string(cands[i][j]) + " has not been added" + at);
  }
  // SC:284-306 on the host: early returns, rebuilds, and the snapshot every query sees
  std::vector<std::vector<int>> snaps;  // snaps[0] = the handle's current snapshot
  snaps.push_back(h->snapshot);
  std::vector<int> snap_of(count, -1), rebuilt(count, 0), counter_after(count, 0);
  int counter = h->counter, cur = 0;
  for (int i = 0; i < count; ++i) {
    if (qidx[i] < GORIO_SC_EXCLUDE_RECENT) {
      counter_after[i] = counter;
      continue;
    }
    if (counter % GORIO_SC_TREE_PERIOD == 0) {
      std::vector<int> s;
      for (int j = 0; j < ncand[i]; ++j)  // size_t arithmetic (SC:300): a candidate after the query wraps and is kept
        if ((size_t)qidx[i] - (size_t)cands[i][j] >= (size_t)GORIO_SC_EXCLUDE_RECENT) s.push_back(cands[i][j]);
      snaps.push_back(std::move(s));
      cur = (int)snaps.size() - 1;
      rebuilt[i] = 1;
    }
    counter = counter + 1;
    counter_after[i] = counter;
    snap_of[i] = cur;
  }
  // pack: chunks | queries | index pool (snapshots in use, then candidate lists)
  std::vector<gorio::ScChunk> chunks;
  std::vector<gorio::ScQuery> queries;
  std::vector<int> pool, snap_off(snaps.size(), -1), slot(count, -1);
  for (int i = 0; i < count; ++i) {
    if (snap_of[i] < 0) continue;
    const int sid = snap_of[i];
    if (snap_off[sid] < 0) {
      snap_off[sid] = (int)pool.size();
      pool.insert(pool.end(), snaps[sid].begin(), snaps[sid].end());
    }
  }
  for (int i = 0; i < count; ++i) {
    if (snap_of[i] < 0) continue;
    const int m = (int)snaps[snap_of[i]].size();
    gorio::ScQuery Q;
    Q.qdb = qidx[i];
    Q.chunk_off = (int)chunks.size();
    for (int b = 0; b < m; b += gorio::kScKnnChunk) chunks.push_back(gorio::ScChunk{qidx[i], snap_off[snap_of[i]], b, std::min(m, b + gorio::kScKnnChunk)});
    Q.n_chunks = (int)chunks.size() - Q.chunk_off;
    Q.cand_off = (int)pool.size();
    Q.n_cand = ncand[i];
    pool.insert(pool.end(), cands[i], cands[i] + ncand[i]);
    slot[i] = (int)queries.size();
    queries.push_back(Q);
  }
  const int nq = (int)queries.size();
  std::vector<gorio::ScOut> res(nq);
  if (nq) {
    const size_t b_chunks = sizeof(gorio::ScChunk) * chunks.size(), b_queries = sizeof(gorio::ScQuery) * queries.size(), b_pool = sizeof(int) * pool.size();
    std::vector<char> blob(b_chunks + b_queries + b_pool);
    if (b_chunks) std::memcpy(blob.data(), chunks.data(), b_chunks);
    std::memcpy(blob.data() + b_chunks, queries.data(), b_queries);
    if (b_pool) std::memcpy(blob.data() + b_chunks + b_queries, pool.data(), b_pool);
    GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
    const size_t n_partial = std::max<size_t>(3 * chunks.size(), 3);  // the scratch buffers grow by half beyond the need
    GORIO_HIP_CHECK(sc_fail, h->d_in.reserve(blob.size(), blob.size() + blob.size() / 2));
    GORIO_HIP_CHECK(sc_fail, h->d_partial.reserve(n_partial, n_partial + n_partial / 2));
    GORIO_HIP_CHECK(sc_fail, h->d_out.reserve(nq, nq + nq / 2));
    char* base = (char*)h->d_in.get();
    const gorio::ScChunk* d_chunks = (const gorio::ScChunk*)base;
    const gorio::ScQuery* d_queries = (const gorio::ScQuery*)(base + b_chunks);
    const int* d_pool = (const int*)(base + b_chunks + b_queries);
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
    if (!chunks.empty()) hipLaunchKernelGGL(gorio::sc_knn_kernel, dim3((unsigned)chunks.size()), dim3(gorio::kScThreads), 0, h->stream, d_chunks, d_pool, h->db_ringf, h->d_partial);
    hipLaunchKernelGGL(gorio::sc_knn_merge_kernel, dim3(nq), dim3(64), 0, h->stream, d_queries, h->d_partial, d_pool, h->d_out);
    const int n_pairs = 3 * nq;
    hipLaunchKernelGGL(gorio::sc_pair_kernel, dim3((n_pairs + 3) / 4), dim3(gorio::kScThreads), 0, h->stream, h->d_out, n_pairs, h->db());
    GORIO_HIP_CHECK(sc_fail, hipGetLastError());
    GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(res.data(), h->d_out, sizeof(gorio::ScOut) * nq, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  }
  const double unit = (h->p.azimuth_range - (-h->p.azimuth_range)) / double(GORIO_SC_SECTORS);  // PC_UNIT_SECTOR_ANGLE (SC:72)
  for (int i = 0; i < count; ++i) {
    if (slot[i] < 0) {  // SC:284-288
      loop_id[i] = -1;
      yaw_rad[i] = 0.0f;
      min_dist[i] = 10000000.0;
      if (diag) sc_diag_early(&diag[i], counter_after[i]);
      continue;
    }
    const gorio::ScOut& o = res[slot[i]];
    double md = 10000000.0;  // SC:312-314, 330-348
    int nn_align = 0, nn_idx = 0;
    for (int k = 0; k < 3; ++k) {
      if (o.kf[k] < 0) continue;
      if (o.dist[k] < md) {
        md = o.dist[k];
        nn_align = o.shift[k];
        nn_idx = o.kf[k];
      }
    }
    loop_id[i] = md < h->p.sc_dist_thresh ? nn_idx : -1;                      // SC:354-356
    const float deg = (float)(nn_align * unit);                              // deg2rad(float degrees) (SC:18-21, 369)
    yaw_rad[i] = (float)((double)deg * M_PI / 180.0);
    min_dist[i] = md;
    if (diag) {
      gorio_sc_diag& d = diag[i];
      d = gorio_sc_diag{};
      d.rebuilt = rebuilt[i];
      d.counter = counter_after[i];
      d.snapshot_size = (int)snaps[snap_of[i]].size();
      d.n_found = o.n_found;
      for (int k = 0; k < 3; ++k) {
        d.position[k] = o.pos[k];
        d.key_dist[k] = o.keyd[k];
        d.keyframe[k] = o.kf[k];
        d.sc_dist[k] = o.dist[k];
        d.sc_shift[k] = o.shift[k];
      }
    }
  }
  h->counter = counter;
  if (cur != 0) h->snapshot = std::move(snaps[cur]);
  return GORIO_OK;
}
}  // namespace

extern "C" {

const char* gorio_sc_last_error(void) { return g_sc_err.c_str(); }

void gorio_sc_default_params(gorio_sc_params* p) {  // every launch file (e.g. launch/ntu_loop3.launch:137-138)
  if (!p) return;
  p->sc_dist_thresh = 0.5;
  p->azimuth_range = 56.5;
}

int gorio_sc_create(gorio_sc_t** out, int device, const gorio_sc_params* p) {
  if (!out || !p) return sc_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  if (!(std::isfinite(p->azimuth_range) && p->azimuth_range > 0)) return sc_fail(GORIO_ERR_INVALID, "create: azimuth_range must be finite and > 0");
  if (std::isnan(p->sc_dist_thresh)) return sc_fail(GORIO_ERR_INVALID, "create: sc_dist_thresh is NaN");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sc_fail(GORIO_ERR_NO_DEVICE, "create: no usable HIP device (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return sc_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(device));
  gorio_sc* h = new (std::nothrow) gorio_sc();
  if (!h) return sc_fail(GORIO_ERR_ALLOC, "create: out of memory");
  h->device = device;
  h->p = *p;
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return sc_fail(GORIO_ERR_NO_DEVICE, "create: no stream");
  }
  *out = h;
  return GORIO_OK;
}

void gorio_sc_destroy(gorio_sc_t* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamDestroy(h->stream);
  delete h;
}

int gorio_sc_add_scans(gorio_sc_t* h, int count, const float* const* xyz, const float* const* intensity, const int* n, const int* stride_bytes, int* first_index_out) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "add_scans: null handle");
  if (count <= 0 || !xyz || !intensity || !n || !stride_bytes) return sc_fail(GORIO_ERR_INVALID, "add_scans: null argument or count <= 0");
  size_t ntot = 0;
  for (int s = 0; s < count; ++s) {
    const std::string at = count > 1 ? " (scan " + std::to_string(s) + ")" : "";
    if (n[s] < 0) return sc_fail(GORIO_ERR_INVALID, "add_scans: negative point count" + at);
    if (n[s] > 0 && (!xyz[s] || !intensity[s] || stride_bytes[s] < 12 || stride_bytes[s] % 4)) return sc_fail(GORIO_ERR_INVALID, "add_scans: bad cloud arguments" + at);
    ntot += n[s];
  }
  if (ntot > (size_t)INT_MAX / 2 || (size_t)h->n + count > (size_t)INT_MAX / 2) return sc_fail(GORIO_ERR_INVALID, "add_scans: too many points or scans");
  // pack (x, y, intensity) -- z is never used (SC:182) -- then the scan offsets, for one upload
  const size_t b_pts = sizeof(float4) * ntot, b_off = sizeof(int) * (count + 1);
  std::vector<char> blob(b_pts + b_off);
  float4* pts = (float4*)blob.data();
  int* off = (int*)(blob.data() + b_pts);
  size_t o = 0;
  for (int s = 0; s < count; ++s) {
    off[s] = (int)o;
    const size_t st = n[s] > 0 ? stride_bytes[s] / 4 : 0;
    for (int i = 0; i < n[s]; ++i, ++o) {
      const float* pt = xyz[s] + st * i;
      pts[o] = make_float4(pt[0], pt[1], intensity[s][st * i], 0.0f);
    }
  }
  off[count] = (int)o;
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (sc_grow_db(h, (size_t)h->n + count)) return GORIO_ERR_NO_DEVICE;
  GORIO_HIP_CHECK(sc_fail, h->d_in.reserve(blob.size(), blob.size() + blob.size() / 2));
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_in, blob.data(), blob.size(), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gorio::sc_descriptor_kernel, dim3(count), dim3(gorio::kScThreads), 0, h->stream, (const float4*)h->d_in.get(), (const int*)((char*)h->d_in.get() + b_pts), h->n,
                     h->p.azimuth_range, h->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  if (first_index_out) *first_index_out = h->n;
  h->n += count;
  return GORIO_OK;
}

int gorio_sc_get_state(const gorio_sc_t* h, int* n_scans, int* counter, int* snapshot_size, int* snapshot, int capacity) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "get_state: null handle");
  if (n_scans) *n_scans = h->n;
  if (counter) *counter = h->counter;
  if (snapshot_size) *snapshot_size = (int)h->snapshot.size();
  if (snapshot) {
    if (capacity < (int)h->snapshot.size()) return sc_fail(GORIO_ERR_INVALID, "get_state: capacity below the snapshot size");
    std::copy(h->snapshot.begin(), h->snapshot.end(), snapshot);
  }
  return GORIO_OK;
}

int gorio_sc_get_descriptor(const gorio_sc_t* h, int index, double* desc, double* ring_key, double* sector_key) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "get_descriptor: null handle");
  if (index < 0 || index >= h->n) return sc_fail(GORIO_ERR_INVALID, "get_descriptor: index " + std::to_string(index) + " has not been added");
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  const size_t i = index;
  if (desc) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(desc, h->db_desc + i * gorio::kScBins, sizeof(double) * gorio::kScBins, hipMemcpyDeviceToHost, h->stream));
  if (ring_key) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(ring_key, h->db_ring + i * gorio::kScRings, sizeof(double) * gorio::kScRings, hipMemcpyDeviceToHost, h->stream));
  if (sector_key) GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(sector_key, h->db_sector + i * gorio::kScSectors, sizeof(double) * gorio::kScSectors, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_sc_distance(gorio_sc_t* h, int i, int j, double* dist, int* shift) {
  if (!h || !dist || !shift) return sc_fail(GORIO_ERR_INVALID, "distance: null argument");
  if (i < 0 || i >= h->n || j < 0 || j >= h->n) return sc_fail(GORIO_ERR_INVALID, "distance: index has not been added");
  gorio::ScOut o{};
  o.qdb = i;
  o.kf[0] = j;
  o.kf[1] = o.kf[2] = -1;
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  GORIO_HIP_CHECK(sc_fail, h->d_out.reserve(1));
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_out, &o, sizeof(o), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(gorio::sc_pair_kernel, dim3(1), dim3(gorio::kScThreads), 0, h->stream, h->d_out, 1, h->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(&o, h->d_out, sizeof(o), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));
  *dist = o.dist[0];
  *shift = o.shift[0];
  return GORIO_OK;
}

int gorio_sc_detect(gorio_sc_t* h, int query_index, const int* candidates, int n_candidates, int* loop_id, float* yaw_rad, double* min_dist, gorio_sc_diag* diag) {
  return sc_detect_run(h, 1, &query_index, &candidates, &n_candidates, loop_id, yaw_rad, min_dist, diag);
}

int gorio_sc_detect_batch(gorio_sc_t* h, int count, const int* query_index, const int* const* candidates, const int* n_candidates, int* loop_id, float* yaw_rad,
                          double* min_dist, gorio_sc_diag* diag) {
  return sc_detect_run(h, count, query_index, candidates, n_candidates, loop_id, yaw_rad, min_dist, diag);
}

}  // extern "C"
