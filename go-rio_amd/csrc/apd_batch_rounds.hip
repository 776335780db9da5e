// apd_batch_rounds.hip -- what the lock-step batched aligns share (gorio_apd_gicp_omp_align_batch, gorio_apd_icp_align_batch with the single
// ICP align and gorio_apd_icp_step, gorio_apd_gicp_mp_align_batch).  Included by apd_api.hip ahead of the three methods' files.
//   batch_front_door     the validation of N handles before anything is built, allocated or launched
//   batch_prepare_search, batch_arm_handles, fill_moved_search   the search-side set-up of the methods that search from a moved copy
//   fold_wave            lane q of one wave adds a job's block partials of term q in block order
//   run_rounds           the round loop: order, round table (batch_rounds.h), upload, the method's launches, fold, copy back, one
//                        synchronisation, the method's machines -- on the stream and in the scratch (gorio_apd::RoundScratch) of hs[0]
#include "batch_rounds.h"

namespace gorio {

using batch_rounds::BlockRef;

// out[q] = the nblk partials of term q added in ascending block order, lane q of one wave
template <int NV>
__device__ __forceinline__ void fold_wave(const double* __restrict__ partials, int nblk, double* __restrict__ out) {
  const int t = threadIdx.x;
  if (t >= NV) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partials[(size_t)b * NV + t];
  out[t] = s;
}

}  // namespace gorio

namespace {

// "<name>: handle <q>: <why>" on handles[0].  Checks, in this order: arguments, null handles; per handle one device, no duplicate, the
// method, (same_params) the parameters of handles[0] but for cl_weight_points; then per handle ready(), whose message moves to handles[0]
// while the refused handle keeps the error text it had.
int batch_front_door(const std::string& name, gorio_apd** handles, int count, const float* guesses, float* T_out, bool same_params, bool (*is_method)(const gorio_apd*),
                     const char* method_msg, int (*ready)(gorio_apd*)) {
  if (count < 0 || !handles || !guesses || !T_out) return GORIO_ERR_INVALID;
  for (int q = 0; q < count; ++q)
    if (!handles[q]) return handles[0] ? fail(handles[0], GORIO_ERR_INVALID, name + ": handle " + std::to_string(q) + " is null") : GORIO_ERR_INVALID;
  gorio_apd* lead = handles[0];
  auto refuse = [&](int q, int code, const std::string& why) { return fail(lead, code, name + ": handle " + std::to_string(q) + ": " + why); };
  std::unordered_set<gorio_apd*> distinct;
  for (int q = 0; q < count; ++q) {
    gorio_apd* h = handles[q];
    if (h->device != lead->device) return refuse(q, GORIO_ERR_INVALID, "all handles of a batch must live on one device");
    if (!distinct.insert(h).second) return refuse(q, GORIO_ERR_INVALID, "the same handle appears twice in a batch (its buffers would be raced on)");
    if (!is_method(h)) return refuse(q, GORIO_ERR_STATE, method_msg);
    if (!same_params) continue;
    gorio_apd_params a = h->params, b = lead->params;
    a.cl_weight_points = b.cl_weight_points = 0;
    if (std::memcmp(&a, &b, sizeof(a)) != 0) return refuse(q, GORIO_ERR_INVALID, "all handles of a batch must carry the same parameters (cl_weight_points excepted)");
  }
  for (int q = 0; q < count; ++q) {
    gorio_apd* h = handles[q];
    const std::string kept = h->err;
    const int rc = ready(h);
    if (rc) {
      const std::string why = h->err;
      if (h != lead) h->err = kept;
      return refuse(q, rc, why);
    }
  }
  return GORIO_OK;
}

// The per-source-point buffers of every handle, and in pruned mode the search indices of ALL clouds of the batch in one call, as
// LsqBatch::prepare builds them.
int batch_prepare_search(gorio_apd** hs, int count) {
  gorio_apd* lead = hs[0];
  for (int q = 0; q < count; ++q)
    if (int rc = hand_over(lead, hs[q], ensure_points(hs[q], hs[q]->src->n))) return rc;
  if (lead->params.search != GORIO_SEARCH_PRUNED) return GORIO_OK;
  std::vector<std::pair<gorio_apd*, DevCloud*>> all;
  for (int q = 0; q < count; ++q) {
    all.emplace_back(hs[q], hs[q]->src.get());
    all.emplace_back(hs[q], hs[q]->tgt.get());
  }
  return run_index_build(lead, all);
}

// Per handle, in batch order: the method's own preparation prepare(q), then best_key armed on the lead's stream (the kernels that consume a key re-arm it)
template <typename Prepare>
int batch_arm_handles(gorio_apd** hs, int count, Prepare prepare) {
  gorio_apd* lead = hs[0];
  for (int q = 0; q < count; ++q) {
    if (int rc = hand_over(lead, hs[q], prepare(q))) return rc;
    HIP_TRY(lead, hipMemsetAsync(hs[q]->best_key, 0xff, sizeof(unsigned long long) * hs[q]->src->n, lead->stream));
  }
  return GORIO_OK;
}

// Descriptor and state of a 1-NN search of h whose queries are a moved copy of the source (x, y, z; s4 in search-index order or null),
// still to be moved by Tr: the search kernels read coordinates and nothing else of a source, and transform their queries by Tf
void fill_moved_search(gorio_apd* h, PairDesc& d, PairState& s, PairState* d_state, long total_src_waves, const float* x, const float* y, const float* z, const float4* s4,
                       const float* Tr) {
  fill_desc(h, d, d_state, total_src_waves);
  d.src.x = const_cast<float*>(x); d.src.y = const_cast<float*>(y); d.src.z = const_cast<float*>(z);
  d.src.idx.s4 = const_cast<float4*>(s4);
  double Td[16];
  for (int i = 0; i < 16; ++i) Td[i] = (double)Tr[i];
  init_state(s, Td);
  for (int i = 0; i < 12; ++i) s.Tf[i] = Tr[i];
}

// One round as the method's launch hook sees it: job k belongs to handle order[k]; jobs is the host copy of the records already
// uploaded to d_jobs, d_refs the round table behind them (plan: batch_rounds.h).
template <typename Job>
struct RoundView {
  const std::vector<int>& order;
  batch_rounds::Round plan;
  Job* jobs;
  const Job* d_jobs;
  const BlockRef* d_refs;
};

struct RoundCounters { int rounds = 0, launches = 0; };

// The lock-step rounds.  M describes the method's table: Job (with int members first and nblk, which this loop sets), kSums doubles per
// job, kCounts (an int per job behind the sums, from an int per block), kSecondList, and fold(), the launch of its fold kernel.
//   pending(q)                  -1: handle q is finished; 0 / 1: it has a job in this round, of the leading / trailing class
//   fill(k, q, job)             the zeroed record of job k, handle q; returns its JobShape
//   launch(view, launches)      the round's kernels between the upload of the table and the fold; adds its launches
//   consume(k, q, sums, count)  job k's folded sums
// total_wg: the workgroups of a round with every handle pending.  The counters go to the caller, never into a handle.
template <typename M, typename Pending, typename Fill, typename Launch, typename Consume>
int run_rounds(gorio_apd* lead, int count, size_t total_wg, RoundCounters& ctr, Pending pending, Fill fill, Launch launch, Consume consume) {
  using Job = typename M::Job;
  static_assert(sizeof(Job) % alignof(BlockRef) == 0, "the refs follow the job records");
  gorio_apd::RoundScratch& s = lead->round;
  const size_t tab_bytes = batch_rounds::table_bytes(sizeof(Job), count, total_wg, M::kSecondList);
  const size_t job_out = sizeof(double) * M::kSums + (M::kCounts ? sizeof(int) : 0), out_bytes = job_out * (size_t)count;
  HIP_TRY(lead, s.tab.reserve(tab_bytes, batch_rounds::grown(tab_bytes)));
  HIP_TRY(lead, s.part.reserve(M::kSums * total_wg, M::kSums * batch_rounds::grown(total_wg)));
  if (M::kCounts) HIP_TRY(lead, s.cnt.reserve(total_wg, batch_rounds::grown(total_wg)));
  HIP_TRY(lead, s.out.reserve(out_bytes, batch_rounds::grown(out_bytes)));
  HIP_TRY(lead, s.h_out.reserve(out_bytes, batch_rounds::grown(out_bytes)));
  std::vector<unsigned char> table(tab_bytes);
  std::vector<batch_rounds::JobShape> shape(count);
  std::vector<int> first(count), order;
  order.reserve(count);
  for (;;) {
    order.clear();
    for (int q = 0; q < count; ++q)
      if (pending(q) == 0) order.push_back(q);
    const int n_leading = (int)order.size();
    for (int q = 0; q < count; ++q)
      if (pending(q) == 1) order.push_back(q);
    const int njobs = (int)order.size();
    if (njobs == 0) break;
    Job* const jobs = reinterpret_cast<Job*>(table.data());
    for (int k = 0; k < njobs; ++k) {
      std::memset(&jobs[k], 0, sizeof(Job));
      shape[k] = fill(k, order[k], jobs[k]);
    }
    const batch_rounds::Round plan = batch_rounds::plan_round(shape.data(), njobs, n_leading, first.data(), reinterpret_cast<BlockRef*>(jobs + njobs));
    for (int k = 0; k < njobs; ++k) {
      jobs[k].first = first[k];
      jobs[k].nblk = shape[k].nblk;
    }
    if (int rc = upload_staged(lead, s.pin, s.tab, table.data(), plan.bytes(sizeof(Job)))) return rc;  // <= tab_bytes
    const Job* d_jobs = reinterpret_cast<const Job*>(s.tab.get());
    RoundView<Job> view{order, plan, jobs, d_jobs, reinterpret_cast<const BlockRef*>(d_jobs + njobs)};
    int launches = 1;  // the fold
    if (int rc = launch(view, launches)) return rc;
    double* d_out = static_cast<double*>(s.out.get());
    M::fold(njobs, lead->stream, d_jobs, s.part, s.cnt, d_out, reinterpret_cast<int*>(d_out + (size_t)M::kSums * njobs));
    HIP_TRY(lead, hipGetLastError());
    HIP_TRY(lead, hipMemcpyAsync(s.h_out.get(), d_out, job_out * (size_t)njobs, hipMemcpyDeviceToHost, lead->stream));
    HIP_TRY(lead, hipStreamSynchronize(lead->stream));
    ++ctr.rounds;
    ctr.launches += launches;
    const double* sums = static_cast<const double*>(s.h_out.get());
    const int* counts = reinterpret_cast<const int*>(sums + (size_t)M::kSums * njobs);
    for (int k = 0; k < njobs; ++k) consume(k, order[k], sums + (size_t)M::kSums * k, M::kCounts ? counts[k] : 0);
  }
  return GORIO_OK;
}

}  // namespace
