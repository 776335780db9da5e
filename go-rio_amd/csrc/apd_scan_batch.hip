// apd_scan_batch.hip -- N raw scans through the scan pipeline in lock-step rounds: include/gorio_scan_batch.h.  Included at the end of
// apd_scan.hip.  Kernels first, the host side below them.
//
// Every kernel here is the JOB-TABLE form of a single kernel of apd_scan.hip / apd_prep.hip: workgroup b reads its (job, block) entry,
// loads that job's arguments and runs the single kernel's per-workgroup body over the same 256-point block (64 clusters for the cluster
// sums).  No arithmetic is restated, so every member's result is bit for bit its single call's.  No workgroup waits for another and
// there are no floating-point atomics.  The ordered compaction stays three launches: counts per (job, block) into ONE array, ONE scan over
// all of it (block_scan_kernel, apd_voxel_group.hip), scatter; a job's offsets are the scanned counts minus the scanned count of its own
// first block.
#include <hip/hip_runtime.h>

#include <deque>

#pragma clang fp contract(off)

namespace gorio {

struct ScanJob {  // one member's arguments of the elementwise kernels and the compaction; a launch fills what its body reads
  ScanColumns c;
  float *x, *y, *z;  // gate: the uploaded columns, rotated in place
  const float* power;
  unsigned char* keep;
  const int* order;  // permute
  const float* lab;  // set_labels
  float* label;
  float4* p4;
  int n;
  int first_block;  // compaction: the job's first entry in the block table
  GateArgs gate;
  DistanceArgs dist;
  double scan_period;
  float wx, wy, wz;
};

__global__ __launch_bounds__(256) void scan_gate_rotate_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  scan_gate_rotate_body(J.x, J.y, J.z, J.power, J.n, J.gate, J.keep, jb.y);
}
__global__ __launch_bounds__(256) void scan_deskew_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  scan_deskew_body(J.c, J.n, J.scan_period, J.wx, J.wy, J.wz, jb.y);
}
__global__ __launch_bounds__(256) void scan_distance_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  scan_distance_body(J.c.s[0], J.c.s[1], J.c.s[2], J.n, J.dist, J.keep, jb.y);
}
__global__ __launch_bounds__(256) void compact_count_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk, int* __restrict__ bcnt) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  compact_count_body(J.keep, J.n, bcnt + blockIdx.x, jb.y);
}
__global__ __launch_bounds__(256) void compact_scatter_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk, const int* __restrict__ boffs) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  compact_scatter_body(J.c, J.keep, J.n, boffs[blockIdx.x] - boffs[J.first_block], jb.y);
}
__global__ __launch_bounds__(256) void scan_permute_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  scan_permute_body(J.c, J.order, J.n, jb.y);
}
__global__ __launch_bounds__(256) void scan_set_labels_jobs_kernel(const ScanJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanJob& J = jobs[jb.x];
  scan_set_labels_body(J.lab, J.n, J.label, J.p4, jb.y);
}

struct ScanSearchJob {  // one member's arguments of the search kernels on its indexed cloud
  CloudView cloud;
  RadiusArgs ra;   // radius_neighbours
  float r2;        // radius_count
  int k;           // sor_mean_distance: mean_k + 1
  int* cnt_out;    // radius_count
  float* mean_out; // sor_mean_distance
};
__global__ __launch_bounds__(256) void radius_count_jobs_kernel(const ScanSearchJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanSearchJob& J = jobs[jb.x];
  radius_count_body(J.cloud, J.r2, J.cnt_out, jb.y);
}
__global__ __launch_bounds__(256) void sor_mean_distance_jobs_kernel(const ScanSearchJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanSearchJob& J = jobs[jb.x];
  sor_mean_distance_body(J.cloud, J.k, J.mean_out, jb.y);
}
template <int MODE>
__global__ __launch_bounds__(256) void radius_neighbours_jobs_kernel(const ScanSearchJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanSearchJob& J = jobs[jb.x];
  radius_neighbours_body<MODE>(J.cloud, J.ra, jb.y);
}

struct ScanReveJob {  // one member's arguments of the REVE kernels
  const float *px, *py, *pz, *inten, *dop;  // features: the gated columns (stride 1)
  double* f;
  unsigned char* valid;
  int n;
  ReveCfg cfg;
  const double* fv;  // eval, sums: the valid rows
  int m;
  const double* v;   // eval: [K][3]; sums: the estimate (pass 1) or nullptr
  double thresh;
  unsigned char* flags;
  int K;
  const unsigned char* sel;
  double* out;
};
__global__ __launch_bounds__(256) void reve_features_jobs_kernel(const ScanReveJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanReveJob& J = jobs[jb.x];
  reve_features_body(J.px, J.py, J.pz, J.inten, J.dop, 1, J.n, J.cfg, J.f, J.valid, jb.y);
}
// grid (entries, most hypotheses of a job)
__global__ __launch_bounds__(256) void reve_eval_jobs_kernel(const ScanReveJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanReveJob& J = jobs[jb.x];
  if ((int)blockIdx.y >= J.K) return;
  reve_eval_body(J.fv, J.m, J.v, J.thresh, J.flags, jb.y, blockIdx.y);
}
__global__ __launch_bounds__(256) void reve_sums_jobs_kernel(const ScanReveJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanReveJob& J = jobs[jb.x];
  reve_sums_body(J.fv, J.m, J.sel, J.v, J.out, jb.y);
}

struct ScanClusterJob {
  const float *x, *y, *z;
  const int *members, *offs;
  int nc;
  float* sums;
};
__global__ __launch_bounds__(64) void cluster_sums_jobs_kernel(const ScanClusterJob* __restrict__ jobs, const int2* __restrict__ blk) {
  const int2 jb = blk[blockIdx.x];
  const ScanClusterJob& J = jobs[jb.x];
  cluster_sums_body(J.x, J.y, J.z, J.members, J.offs, J.nc, J.sums, jb.y);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_scan_batch.h)
namespace {

// what the lead handle of a batch holds for it: grows, never shrinks
struct ScanBatchLead {
  DevBuf<void> d_jobs;  // the job table of the launch being enqueued (the stream orders the next upload behind the kernel that reads this one)
  DevBuf<int2> d_blk;   // its (job, block) entries
  DevBuf<int> d_bcnt;   // the compaction's counts of all blocks of all jobs, scanned in place
  std::vector<int> bcnt;                             // their host copy
  std::deque<std::vector<unsigned char>> staged;     // host arrays with an upload in flight; dropped at the round's synchronisation
  int rounds = 0, launches = 0, syncs = 0;
};

struct BatchMember {
  gorio_scan* h = nullptr;
  int i = 0;  // position in the call
  bool live = true;
  const ScanCloud* cur = nullptr;
  gorio_scan_result* r = nullptr;
  int* code = nullptr;
  const double* ang_vel = nullptr;
  ReveSolve solve;
  std::vector<unsigned char> inlier, keep;
  std::vector<double> f;               // load: feature rows
  std::vector<unsigned char> valid;
  std::vector<int> cnt, order, adj, cmembers, coffs;
  std::vector<float> dist, sums, lab;
  std::vector<long long> offs;
  std::vector<std::vector<int>> clusters;
  int first_block = 0, n_ground = 0, n_full = 0;
};

struct ScanBatch {
  ScanBatchLead& L;
  hipStream_t stream;
  std::vector<BatchMember> ms;
  bool round_used = false;
};

int batch_sync(ScanBatch& B) {
  GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(B.stream));
  ++B.L.syncs;
  if (B.round_used) ++B.L.rounds;
  B.round_used = false;
  B.L.staged.clear();
  return GORIO_OK;
}

// jobs and their (job, block) entries go up; nblocks[q] entries for job q.  The tables are copied into staging that lives until the
// round's synchronisation.
template <typename Job>
int batch_tables(ScanBatch& B, const std::vector<Job>& jobs, const std::vector<int>& nblocks, const Job*& d_jobs, const int2*& d_blk, int& total) {
  ScanBatchLead& L = B.L;
  total = 0;
  for (int nb : nblocks) total += nb;
  L.staged.emplace_back(sizeof(Job) * jobs.size());
  std::vector<unsigned char>& hj = L.staged.back();
  std::memcpy(hj.data(), jobs.data(), hj.size());
  L.staged.emplace_back(sizeof(int2) * (size_t)std::max(total, 1));
  int2* hb = reinterpret_cast<int2*>(L.staged.back().data());
  int e = 0;
  for (int q = 0; q < (int)nblocks.size(); ++q)
    for (int b = 0; b < nblocks[q]; ++b) hb[e++] = make_int2(q, b);
  GORIO_HIP_CHECK(scan_fail, L.d_jobs.reserve(hj.size(), hj.size() + hj.size() / 2 + 1024));
  GORIO_HIP_CHECK(scan_fail, L.d_blk.reserve((size_t)total, (size_t)total + (size_t)total / 4 + 256));
  GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(L.d_jobs, hj.data(), hj.size(), hipMemcpyHostToDevice, B.stream));
  if (total > 0) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(L.d_blk, hb, sizeof(int2) * (size_t)total, hipMemcpyHostToDevice, B.stream));
  d_jobs = static_cast<const Job*>(L.d_jobs.get());
  d_blk = L.d_blk;
  B.round_used = true;
  return GORIO_OK;
}

int batch_launched(ScanBatch& B, int launches = 1) {
  GORIO_HIP_CHECK(scan_fail, hipGetLastError());
  B.L.launches += launches;
  return GORIO_OK;
}

struct CompactItem {
  BatchMember* m;
  const ScanCloud* src;
  ScanCloud* dst;
};

// scan_compact for every item: dst = the points of src whose keep byte (the member's own d_keep) is set, in order.  Three launches and the
// download of the scanned counts; batch_compact_finish after the round's synchronisation sets every dst.n.
int batch_compact(ScanBatch& B, std::vector<CompactItem>& items) {
  if (items.empty()) return GORIO_OK;
  ScanBatchLead& L = B.L;
  std::vector<gorio::ScanJob> jobs(items.size());
  std::vector<int> nblocks(items.size());
  int first = 0;
  for (size_t q = 0; q < items.size(); ++q) {
    gorio::ScanJob& J = jobs[q];
    std::memset(&J, 0, sizeof(J));
    J.c = scan_columns(*items[q].src, *items[q].dst);
    J.keep = items[q].m->h->d_keep;
    J.n = items[q].src->n;
    J.first_block = first;
    items[q].m->first_block = first;
    nblocks[q] = (J.n + 255) / 256;
    first += nblocks[q];
  }
  const gorio::ScanJob* dj = nullptr;
  const int2* db = nullptr;
  int total = 0;
  int rc = batch_tables(B, jobs, nblocks, dj, db, total);
  if (rc) return rc;
  GORIO_HIP_CHECK(scan_fail, L.d_bcnt.reserve((size_t)total + 1, (size_t)total + (size_t)total / 4 + 260));
  gorio::compact_count_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db, L.d_bcnt);
  gorio::block_scan_kernel<<<1, 1024, 0, B.stream>>>(L.d_bcnt, total);
  gorio::compact_scatter_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db, L.d_bcnt);
  rc = batch_launched(B, 3);
  if (rc) return rc;
  L.bcnt.assign((size_t)total + 1, 0);
  GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(L.bcnt.data(), L.d_bcnt, sizeof(int) * ((size_t)total + 1), hipMemcpyDeviceToHost, B.stream));
  return GORIO_OK;
}
void batch_compact_finish(ScanBatch& B, std::vector<CompactItem>& items) {
  const std::vector<int>& bc = B.L.bcnt;
  for (size_t q = 0; q < items.size(); ++q) {
    const int lo = items[q].m->first_block, hi = q + 1 < items.size() ? items[q + 1].m->first_block : (int)bc.size() - 1;
    items[q].dst->n = bc[hi] - bc[lo];
    items[q].dst->identity = false;
  }
}

// a launch of an elementwise job-table kernel over `sel` members; fill(J, member) sets what the body reads and returns the point count
template <typename Fill, typename Launch>
int batch_elementwise(ScanBatch& B, std::vector<BatchMember*>& sel, Fill fill, Launch launch) {
  if (sel.empty()) return GORIO_OK;
  std::vector<gorio::ScanJob> jobs(sel.size());
  std::vector<int> nblocks(sel.size());
  for (size_t q = 0; q < sel.size(); ++q) {
    std::memset(&jobs[q], 0, sizeof(gorio::ScanJob));
    fill(jobs[q], *sel[q]);
    nblocks[q] = (jobs[q].n + 255) / 256;
  }
  const gorio::ScanJob* dj = nullptr;
  const int2* db = nullptr;
  int total = 0;
  int rc = batch_tables(B, jobs, nblocks, dj, db, total);
  if (rc) return rc;
  launch(total, dj, db);
  return batch_launched(B);
}

// a launch of a search job-table kernel over `sel` members, each on the indexed source of its registration handle
template <typename Fill, typename Launch>
int batch_search(ScanBatch& B, std::vector<BatchMember*>& sel, Fill fill, Launch launch) {
  if (sel.empty()) return GORIO_OK;
  std::vector<gorio::ScanSearchJob> jobs(sel.size());
  std::vector<int> nblocks(sel.size());
  for (size_t q = 0; q < sel.size(); ++q) {
    std::memset(&jobs[q], 0, sizeof(gorio::ScanSearchJob));
    jobs[q].cloud = sel[q]->h->prep.h->src->view();
    fill(jobs[q], *sel[q]);
    nblocks[q] = (roundup(sel[q]->cur->n, 512) + 255) / 256;
  }
  const gorio::ScanSearchJob* dj = nullptr;
  const int2* db = nullptr;
  int total = 0;
  int rc = batch_tables(B, jobs, nblocks, dj, db, total);
  if (rc) return rc;
  launch(total, dj, db);
  return batch_launched(B);
}

// prep_index_cloud_device for every member of `sel`: its current cloud becomes the source of its registration handle (one copy launch),
// the search indices are built by one run_index_build over the list, and every context gets its per-point slots
int batch_index(ScanBatch& B, std::vector<BatchMember*>& sel) {
  if (sel.empty()) return GORIO_OK;
  std::vector<gorio_apd*> hs;
  std::vector<gorio_apd_device_cloud> src;
  for (BatchMember* m : sel) {
    gorio_apd* a = m->h->prep.h;
    a->params.search = GORIO_SEARCH_PRUNED;
    hs.push_back(a);
    src.push_back(gorio_apd_device_cloud{m->cur->col(0), m->cur->col(1), m->cur->col(2), nullptr, m->cur->n});
  }
  int rc = gorio_apd_set_clouds_device_batch(hs.data(), (int)hs.size(), src.data(), nullptr);
  if (rc) return scan_fail(rc, hs[0]->err);
  ++B.L.launches;
  std::vector<std::pair<gorio_apd*, DevCloud*>> list;
  for (gorio_apd* a : hs) list.push_back({a, a->src.get()});
  rc = run_index_build(hs[0], list);
  if (rc) return scan_fail(rc, hs[0]->err);
  B.L.launches += g_index_build_launches;
  for (BatchMember* m : sel) {
    PrepCtx& c = m->h->prep;
    const int n = m->cur->n;
    const size_t cap = (size_t)n + n / 8;
    GORIO_HIP_CHECK(scan_fail, reserve_group(c.pts_cap, n, cap, c.d_cnt, cap, c.d_offs, cap));
    ++m->h->index_builds;
  }
  B.round_used = true;
  return GORIO_OK;
}

// the member's run ends here; REFUSED keeps its text in the handle
void batch_end(BatchMember& m, int status, int stage, int rc, const std::string& text = std::string()) {
  m.r->status = status;
  m.r->stage = stage;
  *m.code = rc;
  if (status == GORIO_SCAN_REFUSED) m.h->run_err = text;
  m.live = false;
}

std::vector<BatchMember*> batch_live(ScanBatch& B) {
  std::vector<BatchMember*> v;
  for (BatchMember& m : B.ms)
    if (m.live) v.push_back(&m);
  return v;
}

// the checks both calls share; `what` = "load_batch" / "run_batch"
int batch_check_handles(const char* what, gorio_scan_t* const* handles, int count) {
  const std::string w = what;
  if (count < 0) return scan_fail(GORIO_ERR_INVALID, w + ": count < 0");
  if (count > GORIO_SCAN_BATCH_MAX) return scan_fail(GORIO_ERR_UNSUPPORTED, w + ": more than " + std::to_string(GORIO_SCAN_BATCH_MAX) + " members");
  std::unordered_set<const gorio_scan*> seen;
  for (int i = 0; i < count; ++i) {
    const std::string at = "handles[" + std::to_string(i) + "]";
    if (!handles[i]) return scan_fail(GORIO_ERR_INVALID, w + ": " + at + " is null");
    if (!seen.insert(handles[i]).second) return scan_fail(GORIO_ERR_INVALID, w + ": " + at + " is listed twice");
    if (handles[i]->device != handles[0]->device) return scan_fail(GORIO_ERR_INVALID, w + ": " + at + " lives on another device than handles[0]");
  }
  return GORIO_OK;
}

ScanBatchLead& batch_lead(gorio_scan* lead) {
  if (!lead->batch) lead->batch = std::make_shared<ScanBatchLead>();
  ScanBatchLead& L = *lead->batch;
  L.rounds = L.launches = L.syncs = 0;
  L.staged.clear();
  return L;
}

// ---- the rounds of gorio_scan_run_batch, in the order of scan_run_stages (apd_scan.hip); each leaves the stream synchronised

// 1. REVE (PREP:421-449): up to three sub-rounds -- the hypotheses' inlier flags, the sums of the selected rows, the same with the residual
int batch_round_reve(ScanBatch& B) {
  for (BatchMember& m : B.ms) {
    if (!m.live) continue;
    m.inlier.assign((size_t)m.cur->n, 0);
    m.solve.inlier_mask = m.inlier.data();
    const int rc = reve_solve_begin(m.solve);
    if (rc) batch_end(m, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GATE, rc, gorio_prep_last_error());
  }
  for (;;) {
    std::vector<BatchMember*> ev, su;
    for (BatchMember& m : B.ms) {
      if (!m.live) continue;
      if (m.solve.want == ReveSolve::EVAL) ev.push_back(&m);
      if (m.solve.want == ReveSolve::SUMS) su.push_back(&m);
    }
    if (ev.empty() && su.empty()) break;
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<BatchMember*>& sel = kind == 0 ? ev : su;
      if (sel.empty()) continue;
      std::vector<gorio::ScanReveJob> jobs(sel.size());
      std::vector<int> nblocks(sel.size());
      int max_k = 1;
      for (size_t q = 0; q < sel.size(); ++q) {
        gorio::ScanReveJob& J = jobs[q];
        std::memset(&J, 0, sizeof(J));
        BatchMember& m = *sel[q];
        ReveCtx& c = m.h->reve;
        J.fv = c.d_fv;
        J.m = m.h->frame.m;
        if (kind == 0) {
          J.v = c.d_v;
          J.thresh = (double)m.h->p.reve.inlier_thresh;
          J.flags = c.d_flags;
          J.K = m.solve.K;
          max_k = std::max(max_k, J.K);
        } else {
          J.sel = c.d_valid;
          J.v = m.solve.pass == 1 ? c.d_v.get() : nullptr;
          J.out = c.d_out;
        }
        nblocks[q] = (J.m + 255) / 256;
      }
      const gorio::ScanReveJob* dj = nullptr;
      const int2* db = nullptr;
      int total = 0;
      int rc = batch_tables(B, jobs, nblocks, dj, db, total);
      if (rc) return rc;
      if (kind == 0) gorio::reve_eval_jobs_kernel<<<dim3(total, max_k), 256, 0, B.stream>>>(dj, db);
      else gorio::reve_sums_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db);
      rc = batch_launched(B);
      if (rc) return rc;
      for (BatchMember* m : sel) {
        rc = reve_solve_download(m->solve);
        if (rc) return scan_fail(rc, gorio_prep_last_error());
      }
    }
    int rc = batch_sync(B);
    if (rc) return rc;
    for (int kind = 0; kind < 2; ++kind)
      for (BatchMember* m : kind == 0 ? ev : su) {
        rc = reve_solve_advance(m->solve);
        if (rc) batch_end(*m, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GATE, rc, gorio_prep_last_error());
      }
  }
  for (BatchMember& m : B.ms) {
    if (!m.live) continue;
    gorio_scan_result* r = m.r;
    const int ok = m.solve.ok;
    r->reve_success = ok;
    if (ok) {
      const double* v = r->v_r;
      if (std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) < 0.05) batch_end(m, GORIO_SCAN_ZERO_VELOCITY, -1, GORIO_OK);  // PREP:427-430
    } else {
      for (int q = 0; q < 3; ++q) r->v_r[q] = r->sigma_v_r[q] = 0.0;
    }
  }
  return GORIO_OK;
}

// the keep bytes of `sel` go up to each member's d_keep, the compaction of cur into the stage's cloud follows, and the round ends
int batch_round_mask_compact(ScanBatch& B, std::vector<BatchMember*>& sel, int stage, bool upload) {
  if (sel.empty()) return GORIO_OK;
  std::vector<CompactItem> items;
  for (BatchMember* m : sel) {
    if (upload) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->h->d_keep, m->keep.data(), m->keep.size(), hipMemcpyHostToDevice, B.stream));
    items.push_back(CompactItem{m, m->cur, &m->h->cl[1 + stage]});
  }
  int rc = batch_compact(B, items);
  if (!rc) rc = batch_sync(B);
  if (rc) return rc;
  batch_compact_finish(B, items);
  for (BatchMember* m : sel) m->cur = &m->h->cl[1 + stage];
  return GORIO_OK;
}

int batch_run_rounds(ScanBatch& B) {
  int rc = GORIO_OK;
  // ---- the gated cloud; empty: REVE fails on no targets, src_cloud is empty (PREP:480)
  for (BatchMember& m : B.ms) {
    m.cur = &m.h->cl[1 + GORIO_SCAN_STAGE_GATE];
    if (m.cur->n == 0) batch_end(m, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_GATE, GORIO_OK);
  }
  // ---- 1. REVE
  rc = batch_round_reve(B);
  if (rc) return rc;
  // ---- 2. dynamic-object removal (PREP:464-478)
  {
    std::vector<BatchMember*> sel;
    for (BatchMember* m : batch_live(B))
      if (m->h->p.enable_dynamic_object_removal) {
        if (!m->solve.ok) std::fill(m->inlier.begin(), m->inlier.end(), 0);
        m->keep = m->inlier;
        sel.push_back(m);
      }
    rc = batch_round_mask_compact(B, sel, GORIO_SCAN_STAGE_DYNAMIC, true);
    if (rc) return rc;
    for (BatchMember* m : batch_live(B)) {
      m->h->stage_cloud[GORIO_SCAN_STAGE_DYNAMIC] = m->cur;
      if (m->cur->n == 0) batch_end(*m, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_DYNAMIC, GORIO_OK);  // PREP:480-482
    }
  }
  // ---- 3. deskew (PREP:484, 658-719) and 4. distance filter (PREP:502, 639-656): one round
  {
    std::vector<BatchMember*> live = batch_live(B), sel;
    for (BatchMember* m : live)
      if (m->h->p.deskew && m->ang_vel) sel.push_back(m);
    rc = batch_elementwise(
        B, sel,
        [](gorio::ScanJob& J, BatchMember& m) {
          ScanCloud& dst = m.h->cl[1 + GORIO_SCAN_STAGE_DESKEW];
          J.c = scan_columns(*m.cur, dst);
          J.n = m.cur->n;
          J.scan_period = m.h->p.scan_period;
          J.wx = -(float)m.ang_vel[0], J.wy = -(float)m.ang_vel[1], J.wz = -(float)m.ang_vel[2];  // PREP:695-696
          dst.n = m.cur->n;
          dst.identity = false;
          m.cur = &dst;
        },
        [&](int total, const gorio::ScanJob* dj, const int2* db) { gorio::scan_deskew_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
    if (rc) return rc;
    for (BatchMember* m : live) m->h->stage_cloud[GORIO_SCAN_STAGE_DESKEW] = m->cur;
    rc = batch_elementwise(
        B, live,
        [](gorio::ScanJob& J, BatchMember& m) {
          const gorio_scan_params& P = m.h->p;
          for (int q = 0; q < 3; ++q) J.c.s[q] = m.cur->col(q);
          J.n = m.cur->n;
          J.dist = gorio::DistanceArgs{P.distance_near, P.distance_far, P.z_low, P.z_high};
          J.keep = m.h->d_keep;
        },
        [&](int total, const gorio::ScanJob* dj, const int2* db) { gorio::scan_distance_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
    if (rc) return rc;
    rc = batch_round_mask_compact(B, live, GORIO_SCAN_STAGE_DISTANCE, false);
    if (rc) return rc;
    for (BatchMember* m : live) {
      m->h->stage_cloud[GORIO_SCAN_STAGE_DISTANCE] = m->cur;
      if (m->cur->n == 0) batch_end(*m, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_DISTANCE, GORIO_OK);
    }
  }
  // ---- 5. outlier removal (PREP:503, 626-637): the searches, then the masks' compaction
  {
    std::vector<BatchMember*> sel, rad, sor;
    for (BatchMember* m : batch_live(B)) {
      const gorio_scan_params& P = m->h->p;
      if (P.outlier_method == GORIO_SCAN_OUTLIER_NONE) continue;
      if (P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL && m->cur->n < P.mean_k + 1) {
        batch_end(*m, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_OUTLIER, GORIO_ERR_INVALID, kSorTooFew);
        continue;
      }
      sel.push_back(m);
      (P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL ? sor : rad).push_back(m);
    }
    if (!sel.empty()) {
      rc = batch_index(B, sel);
      if (rc) return rc;
      rc = batch_search(
          B, rad,
          [](gorio::ScanSearchJob& J, BatchMember& m) {
            J.r2 = prep_radius_r2(m.h->p.radius);
            J.cnt_out = m.h->prep.d_cnt;
          },
          [&](int total, const gorio::ScanSearchJob* dj, const int2* db) { gorio::radius_count_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
      if (rc) return rc;
      rc = batch_search(
          B, sor,
          [](gorio::ScanSearchJob& J, BatchMember& m) {
            J.k = m.h->p.mean_k + 1;
            J.mean_out = reinterpret_cast<float*>(m.h->prep.d_cnt.get());  // one 4-byte word per point, like the neighbour counts
          },
          [&](int total, const gorio::ScanSearchJob* dj, const int2* db) { gorio::sor_mean_distance_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
      if (rc) return rc;
      for (BatchMember* m : rad) {
        m->cnt.assign((size_t)m->cur->n, 0);
        GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->cnt.data(), m->h->prep.d_cnt, sizeof(int) * (size_t)m->cur->n, hipMemcpyDeviceToHost, B.stream));
      }
      for (BatchMember* m : sor) {
        m->dist.assign((size_t)m->cur->n, 0.0f);
        GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->dist.data(), m->h->prep.d_cnt, sizeof(float) * (size_t)m->cur->n, hipMemcpyDeviceToHost, B.stream));
      }
      rc = batch_sync(B);
      if (rc) return rc;
      for (BatchMember* m : sel) {
        const gorio_scan_params& P = m->h->p;
        const int n = m->cur->n;
        m->keep.assign((size_t)n, 0);
        if (P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL) prep_sor_keep_from_distances(m->dist.data(), n, P.stddev_mul, m->keep.data(), nullptr, nullptr);
        else prep_radius_keep_from_counts(m->cnt.data(), n, P.min_neighbors, m->keep.data(), nullptr);
      }
      rc = batch_round_mask_compact(B, sel, GORIO_SCAN_STAGE_OUTLIER, true);
      if (rc) return rc;
    }
    for (BatchMember* m : batch_live(B)) {
      m->h->stage_cloud[GORIO_SCAN_STAGE_OUTLIER] = m->cur;
      if (m->cur->n == 0) batch_end(*m, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_OUTLIER, GORIO_OK);
    }
  }
  // ---- 6. Patchwork++ and full_scan = ground + nonground (PREP:505-518): ground_run over the members' segmenters, then the permutation
  {
    std::vector<BatchMember*> sel;
    for (BatchMember* m : batch_live(B))
      if (m->h->ground) sel.push_back(m);
    if (!sel.empty()) {
      const int cnt = (int)sel.size();
      std::vector<gorio_ground*> hs(cnt);
      std::vector<int> n(cnt), n_ground(cnt, 0), n_full(cnt, 0);
      std::vector<int*> order_ptr(cnt);
      std::vector<GroundDeviceScan> dev(cnt);
      for (int q = 0; q < cnt; ++q) {
        BatchMember& m = *sel[q];
        hs[q] = m.h->ground;
        n[q] = m.cur->n;
        m.order.assign((size_t)n[q], -1);
        order_ptr[q] = m.order.data();
        dev[q] = GroundDeviceScan{m.cur->col(0), m.cur->col(1), m.cur->col(2), m.cur->col(3)};
      }
      // the stream is synchronised (every round ends so): the segmenters launch on a stream of their own
      rc = ground_run(hs.data(), cnt, nullptr, nullptr, n.data(), nullptr, 1, order_ptr.data(), n_ground.data(), n_full.data(), dev.data());
      B.L.launches += 6;  // ground_run with device scans: pack, classify, segment, patch, final fit, below; it synchronises twice
      B.L.syncs += 2;
      ++B.L.rounds;
      std::vector<BatchMember*> perm;
      for (int q = 0; q < cnt; ++q) {
        BatchMember& m = *sel[q];
        if (rc) {
          batch_end(m, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GROUND, rc, gorio_ground_last_error());
          continue;
        }
        bool inside = true;
        for (int j = 0; j < n_full[q]; ++j)
          if (m.order[j] < 0 || m.order[j] >= n[q]) inside = false;
        if (!inside) {
          batch_end(m, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GROUND, GORIO_ERR_STATE, "run: ground order outside the cloud");
          continue;
        }
        m.n_ground = n_ground[q];
        m.n_full = n_full[q];
        if (n_full[q] > 0) perm.push_back(&m);
      }
      for (BatchMember* m : perm) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->h->d_order, m->order.data(), sizeof(int) * (size_t)m->n_full, hipMemcpyHostToDevice, B.stream));
      rc = batch_elementwise(
          B, perm,
          [](gorio::ScanJob& J, BatchMember& m) {
            J.c = scan_columns(*m.cur, m.h->cl[1 + GORIO_SCAN_STAGE_GROUND]);
            J.order = m.h->d_order;
            J.n = m.n_full;
          },
          [&](int total, const gorio::ScanJob* dj, const int2* db) { gorio::scan_permute_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
      if (rc) return rc;
      if (!perm.empty()) {
        rc = batch_sync(B);
        if (rc) return rc;
      }
      for (BatchMember* m : sel) {
        if (!m->live) continue;
        ScanCloud& dst = m->h->cl[1 + GORIO_SCAN_STAGE_GROUND];
        dst.n = m->n_full;
        dst.identity = false;
        m->r->n_ground = m->n_ground;
        m->cur = &dst;
      }
    }
    for (BatchMember* m : batch_live(B)) {
      m->h->stage_cloud[GORIO_SCAN_STAGE_GROUND] = m->cur;
      if (m->cur->n == 0) batch_end(*m, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_GROUND, GORIO_OK);
    }
  }
  // ---- 7. DBSCAN labels (PREP:520-568): index, the two radius passes, the queue replay, the cluster sums, the labels
  {
    std::vector<BatchMember*> live = batch_live(B);
    if (live.empty()) return GORIO_OK;
    rc = batch_index(B, live);
    if (rc) return rc;
    auto radius_args = [](gorio::ScanSearchJob& J, BatchMember& m) {
      PrepCtx& c = m.h->prep;
      J.ra = gorio::RadiusArgs{m.h->p.dbscan_eps, c.d_cnt, c.d_offs, c.d_adj};
    };
    rc = batch_search(B, live, radius_args,
                      [&](int total, const gorio::ScanSearchJob* dj, const int2* db) { gorio::radius_neighbours_jobs_kernel<0><<<total, 256, 0, B.stream>>>(dj, db); });
    if (rc) return rc;
    for (BatchMember* m : live) {
      m->cnt.assign((size_t)m->cur->n, 0);
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->cnt.data(), m->h->prep.d_cnt, sizeof(int) * (size_t)m->cur->n, hipMemcpyDeviceToHost, B.stream));
    }
    rc = batch_sync(B);
    if (rc) return rc;
    for (BatchMember* m : live) {  // the per-member offsets: prefix sums on the host between the two passes, as in the single call
      PrepCtx& c = m->h->prep;
      const int n = m->cur->n;
      m->offs.assign((size_t)n + 1, 0);
      for (int i = 0; i < n; ++i) m->offs[i + 1] = m->offs[i] + m->cnt[i];
      const long long E = m->offs[n];
      GORIO_HIP_CHECK(scan_fail, c.d_adj.reserve((size_t)E, (size_t)E + (size_t)E / 8 + 16));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(c.d_offs, m->offs.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, B.stream));
    }
    rc = batch_search(B, live, radius_args,
                      [&](int total, const gorio::ScanSearchJob* dj, const int2* db) { gorio::radius_neighbours_jobs_kernel<1><<<total, 256, 0, B.stream>>>(dj, db); });
    if (rc) return rc;
    for (BatchMember* m : live) {
      const long long E = m->offs[(size_t)m->cur->n];
      m->adj.assign((size_t)E, 0);
      if (E > 0) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->adj.data(), m->h->prep.d_adj, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost, B.stream));
    }
    rc = batch_sync(B);
    if (rc) return rc;
    std::vector<BatchMember*> with;
    for (BatchMember* m : live) {
      gorio_scan* h = m->h;
      const gorio_scan_params& P = h->p;
      const int n = m->cur->n;
      prep_dbscan_replay(m->cnt, m->offs, m->adj, n, P.dbscan_core_min_pts, P.dbscan_min_cluster_size, P.dbscan_max_cluster_size, m->clusters);
      m->lab.assign((size_t)n, 0.0f);
      const int nc = (int)m->clusters.size();
      if (nc == 0) continue;
      m->cmembers.clear();
      m->coffs.assign(1, 0);
      for (const std::vector<int>& cl : m->clusters) {
        m->cmembers.insert(m->cmembers.end(), cl.begin(), cl.end());
        m->coffs.push_back((int)m->cmembers.size());
      }
      GORIO_HIP_CHECK(scan_fail, h->d_members.reserve(m->cmembers.size(), m->cmembers.size() + m->cmembers.size() / 8));
      GORIO_HIP_CHECK(scan_fail, h->d_coffs.reserve(m->coffs.size(), m->coffs.size() + 64));
      GORIO_HIP_CHECK(scan_fail, h->d_sums.reserve(3 * (size_t)nc, 3 * (size_t)nc + 192));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_members, m->cmembers.data(), sizeof(int) * m->cmembers.size(), hipMemcpyHostToDevice, B.stream));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_coffs, m->coffs.data(), sizeof(int) * m->coffs.size(), hipMemcpyHostToDevice, B.stream));
      with.push_back(m);
    }
    if (!with.empty()) {  // PREP:537-568: the coordinate sums on the device, ranking and label values on the host
      std::vector<gorio::ScanClusterJob> jobs(with.size());
      std::vector<int> nblocks(with.size());
      for (size_t q = 0; q < with.size(); ++q) {
        BatchMember& m = *with[q];
        const int nc = (int)m.clusters.size();
        jobs[q] = gorio::ScanClusterJob{m.cur->col(0), m.cur->col(1), m.cur->col(2), m.h->d_members, m.h->d_coffs, nc, m.h->d_sums};
        nblocks[q] = (nc + 63) / 64;
      }
      const gorio::ScanClusterJob* dj = nullptr;
      const int2* db = nullptr;
      int total = 0;
      rc = batch_tables(B, jobs, nblocks, dj, db, total);
      if (rc) return rc;
      gorio::cluster_sums_jobs_kernel<<<total, 64, 0, B.stream>>>(dj, db);
      rc = batch_launched(B);
      if (rc) return rc;
      for (BatchMember* m : with) {
        m->sums.assign(3 * m->clusters.size(), 0.0f);
        GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->sums.data(), m->h->d_sums, sizeof(float) * m->sums.size(), hipMemcpyDeviceToHost, B.stream));
      }
      rc = batch_sync(B);
      if (rc) return rc;
      for (BatchMember* m : with) {
        std::vector<int> order;
        prep_rank_clusters(m->clusters, m->sums.data(), order);
        const int nc = (int)m->clusters.size();
        for (int r = 0; r < nc; ++r)
          for (int idx : m->clusters[order[r]]) m->lab[idx] = (float)(r + 1);
      }
    }
    for (BatchMember* m : live) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->h->d_lab, m->lab.data(), sizeof(float) * (size_t)m->cur->n, hipMemcpyHostToDevice, B.stream));
    rc = batch_elementwise(
        B, live,
        [](gorio::ScanJob& J, BatchMember& m) {
          DevCloud& out = *m.h->prep.h->src;
          J.lab = m.h->d_lab;
          J.n = m.cur->n;
          J.label = out.label;
          J.p4 = out.p4;
        },
        [&](int total, const gorio::ScanJob* dj, const int2* db) { gorio::scan_set_labels_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
    if (rc) return rc;
    rc = batch_sync(B);
    if (rc) return rc;
    for (BatchMember* m : live) {
      const int n = m->cur->n;
      m->r->n_clusters = (int)m->clusters.size();
      m->r->n_out = n;
      m->h->n_out = n;
      m->h->have_output = true;
      m->r->status = GORIO_SCAN_OK;
      *m->code = GORIO_OK;
      m->live = false;
    }
  }
  return GORIO_OK;
}

}  // namespace

extern "C" {

const char* gorio_scan_handle_error(const gorio_scan_t* h) { return h ? h->run_err.c_str() : ""; }

int gorio_scan_batch_diag(const gorio_scan_t* lead, int* rounds, int* launches, int* synchronisations) {
  if (!lead) return scan_fail(GORIO_ERR_INVALID, "batch_diag: null handle");
  const ScanBatchLead* L = lead->batch.get();
  if (rounds) *rounds = L ? L->rounds : 0;
  if (launches) *launches = L ? L->launches : 0;
  if (synchronisations) *synchronisations = L ? L->syncs : 0;
  return GORIO_OK;
}

int gorio_scan_load_batch(gorio_scan_t* const* handles, int count, const float* const* xyz, const float* const* power, const float* const* doppler, const int* n,
                          const int* stride_bytes, int* n_gated, int* n_valid) {
  if (count == 0) return GORIO_OK;
  if (count > 0 && (!handles || !xyz || !power || !doppler || !n || !stride_bytes || !n_gated || !n_valid)) return scan_fail(GORIO_ERR_INVALID, "load_batch: null argument");
  int rc = batch_check_handles("load_batch", handles, count);
  if (rc) return rc;
  long long total_pts = 0;
  for (int i = 0; i < count; ++i) {
    const std::string at = "load_batch: handles[" + std::to_string(i) + "]: ";
    if (n[i] < 0 || (n[i] > 0 && (!xyz[i] || !power[i] || !doppler[i]))) return scan_fail(GORIO_ERR_INVALID, at + "bad cloud arguments");
    if (stride_bytes[i] < 4 || (stride_bytes[i] % 4)) return scan_fail(GORIO_ERR_INVALID, at + "bad stride");
    total_pts += n[i];
  }
  if (total_pts > (long long)INT_MAX) return scan_fail(GORIO_ERR_UNSUPPORTED, "load_batch: more than 2^31 - 1 raw points in all");
  // ---- as gorio_scan_load from here: the state of every member is reset, its device side made, its buffers sized
  for (int i = 0; i < count; ++i) {
    gorio_scan* h = handles[i];
    h->loaded = false;
    h->have_output = false;
    for (auto& s : h->stage_cloud) s = nullptr;
    n_gated[i] = n_valid[i] = 0;
  }
  for (int i = 0; i < count; ++i) {
    gorio_scan* h = handles[i];
    rc = scan_ensure_device(h);
    if (rc) return rc;
    GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
    rc = scan_reserve(h, n[i]);
    if (rc) return rc;
  }
  gorio_scan* lead = handles[0];
  ScanBatch B{batch_lead(lead), lead->stream, {}, false};
  B.ms.resize(count);
  // ---- round 1: the uploads, gate + rotate, the compaction into the gated clouds
  std::vector<BatchMember*> up;
  for (int i = 0; i < count; ++i) {
    BatchMember& m = B.ms[i];
    gorio_scan* h = handles[i];
    m.h = h;
    m.i = i;
    ScanCloud &raw = h->cl[kScanRaw], &gated = h->cl[1 + GORIO_SCAN_STAGE_GATE];
    h->n_raw = n[i];
    raw.n = n[i];
    gated.n = 0;
    h->frame = ReveFrame();
    if (n[i] == 0) continue;
    const size_t st = stride_bytes[i] / 4, cap = raw.cap;
    B.L.staged.emplace_back(sizeof(float) * (4 * cap + (size_t)n[i]));  // the one upload of the frame: the five message columns in one copy
    float* cols = reinterpret_cast<float*>(B.L.staged.back().data());
    for (int k = 0; k < n[i]; ++k) {
      const float* pt = xyz[i] + st * k;
      cols[k] = pt[0];
      cols[cap + k] = pt[1];
      cols[2 * cap + k] = pt[2];
      cols[3 * cap + k] = power[i][st * k];
      cols[4 * cap + k] = doppler[i][st * k];
    }
    GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(raw.f, cols, B.L.staged.back().size(), hipMemcpyHostToDevice, B.stream));
    ++h->point_uploads;
    m.cur = &raw;
    up.push_back(&m);
  }
  rc = batch_elementwise(
      B, up,
      [](gorio::ScanJob& J, BatchMember& m) {
        const ScanCloud& raw = m.h->cl[kScanRaw];
        J.x = raw.col(0), J.y = raw.col(1), J.z = raw.col(2);
        J.power = raw.col(3);
        J.n = raw.n;
        std::memcpy(J.gate.R, m.h->p.rotation, sizeof(J.gate.R));
        J.gate.power_threshold = m.h->p.power_threshold;
        J.keep = m.h->d_keep;
      },
      [&](int total, const gorio::ScanJob* dj, const int2* db) { gorio::scan_gate_rotate_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db); });
  if (rc) return rc;
  rc = batch_round_mask_compact(B, up, GORIO_SCAN_STAGE_GATE, false);
  if (rc) return rc;
  // ---- round 2: REVE:75-90 on the gated clouds (radarcloud_raw, PREP:397-409)
  std::vector<BatchMember*> fe;
  for (int i = 0; i < count; ++i) {
    gorio_scan* h = handles[i];
    const ScanCloud& gated = h->cl[1 + GORIO_SCAN_STAGE_GATE];
    h->stage_cloud[GORIO_SCAN_STAGE_GATE] = &gated;
    n_gated[i] = gated.n;
    if (gated.n == 0) continue;
    rc = reve_prepare(h->reve, h->device, gated.n);
    if (rc) return scan_fail(rc, gorio_prep_last_error());
    fe.push_back(&B.ms[i]);
  }
  if (!fe.empty()) {
    std::vector<gorio::ScanReveJob> jobs(fe.size());
    std::vector<int> nblocks(fe.size());
    for (size_t q = 0; q < fe.size(); ++q) {
      gorio_scan* h = fe[q]->h;
      const ScanCloud& g = h->cl[1 + GORIO_SCAN_STAGE_GATE];
      gorio::ScanReveJob& J = jobs[q];
      std::memset(&J, 0, sizeof(J));
      J.px = g.col(0), J.py = g.col(1), J.pz = g.col(2), J.inten = g.col(3), J.dop = g.col(4);
      J.f = h->reve.d_f;
      J.valid = h->reve.d_valid;
      J.n = g.n;
      J.cfg = reve_device_cfg(&h->p.reve);
      nblocks[q] = (g.n + 255) / 256;
    }
    const gorio::ScanReveJob* dj = nullptr;
    const int2* db = nullptr;
    int total = 0;
    rc = batch_tables(B, jobs, nblocks, dj, db, total);
    if (rc) return rc;
    gorio::reve_features_jobs_kernel<<<total, 256, 0, B.stream>>>(dj, db);
    rc = batch_launched(B);
    if (rc) return rc;
    for (BatchMember* m : fe) {
      gorio_scan* h = m->h;
      const int gn = h->cl[1 + GORIO_SCAN_STAGE_GATE].n;
      m->f.assign((size_t)gn * 4, 0.0);
      m->valid.assign((size_t)gn, 0);
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->f.data(), h->reve.d_f, sizeof(double) * m->f.size(), hipMemcpyDeviceToHost, B.stream));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(m->valid.data(), h->reve.d_valid, (size_t)gn, hipMemcpyDeviceToHost, B.stream));
    }
    rc = batch_sync(B);
    if (rc) return rc;
    for (BatchMember* m : fe) reve_collect(m->h->frame, m->f, m->valid, m->h->cl[1 + GORIO_SCAN_STAGE_GATE].n);
  }
  for (int i = 0; i < count; ++i) {
    n_valid[i] = handles[i]->frame.m;
    handles[i]->loaded = true;
  }
  return GORIO_OK;
}

int gorio_scan_run_batch(gorio_scan_t* const* handles, int count, const unsigned int* const* sample_idx, const int* n_iter, const double* const* ang_vel,
                         gorio_scan_result* results, int* codes) {
  if (count == 0) return GORIO_OK;
  if (count > 0 && (!handles || !sample_idx || !n_iter || !results || !codes)) return scan_fail(GORIO_ERR_INVALID, "run_batch: null argument");
  int rc = batch_check_handles("run_batch", handles, count);
  if (rc) return rc;
  for (int i = 0; i < count; ++i) {
    const std::string at = "run_batch: handles[" + std::to_string(i) + "]: ";
    if (n_iter[i] < 0 || (n_iter[i] > 0 && !sample_idx[i])) return scan_fail(GORIO_ERR_INVALID, at + "bad sample arguments");
  }
  for (int i = 0; i < count; ++i)
    if (!handles[i]->loaded)
      return scan_fail(GORIO_ERR_STATE, "run_batch: handles[" + std::to_string(i) + "]: no scan loaded (gorio_scan_load or gorio_scan_load_batch comes first, once per run)");
  gorio_scan* lead = handles[0];
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(lead->device));
  ScanBatch B{batch_lead(lead), lead->stream, {}, false};
  B.ms.resize(count);
  for (int i = 0; i < count; ++i) {
    BatchMember& m = B.ms[i];
    gorio_scan* h = handles[i];
    m.h = h;
    m.i = i;
    m.r = &results[i];
    m.code = &codes[i];
    m.ang_vel = ang_vel ? ang_vel[i] : nullptr;
    std::memset(m.r, 0, sizeof(*m.r));
    m.r->stage = -1;
    codes[i] = GORIO_OK;
    h->run_err.clear();
    h->loaded = false;
    h->have_output = false;
    ReveSolve& S = m.solve;
    S.c = &h->reve;
    S.cfg = &h->p.reve;
    S.fr = &h->frame;
    S.sample_idx = sample_idx[i];
    S.n_iter = n_iter[i];
    S.v_r = m.r->v_r;
    S.sigma_v_r = m.r->sigma_v_r;
  }
  for (BatchMember& m : B.ms) m.solve.inlier_mask = nullptr;  // set per round: the mask is sized there
  return batch_run_rounds(B);
}

}  // extern "C"
