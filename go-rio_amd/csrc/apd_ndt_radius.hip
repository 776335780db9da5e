// apd_ndt_radius.hip -- the search half of NDT's radius mode (gorio_ndt_set_radius_search, apd_ndt.hip): host code only, included by
// apd_api.hip behind apd_search.hip, where the search handle's type is complete.  apd_ndt.hip declares these functions and holds every
// kernel of the mode; here a per-NDT-handle search state is pointed at the centroid cloud of the target state and handed to
// search_radius_core / search_radius_batch_core, the way apd_gicp_mp.hip drives the search state inside a registration handle.
namespace {

// a search state without a cloud of its own: `up` and `cloud` are set before every use (ndt_rs_bind)
gorio_search_handle* ndt_rs_new(int device) {
  gorio_search_handle* s = new (std::nothrow) gorio_search_handle();
  if (s) s->device = device;
  return s;
}

void ndt_rs_free(gorio_search_handle* s) {
  if (!s) return;
  hipSetDevice(s->device);
  delete s;  // the buffers, with the device current
}

hipStream_t ndt_rs_stream(gorio_search_handle* cloud) { return cloud->up->stream; }

// s searches the cloud `cloud` holds, through cloud's registration handle (its stream and launch scratch)
void ndt_rs_bind(gorio_search_handle* s, gorio_search_handle* cloud) {
  s->up = cloud->up;
  s->cloud = cloud->up->src.get();
}

void ndt_rs_csr(NdtRadiusJob* job) {
  const gorio_search_handle* s = job->s;
  job->csr.offs = s->d_kept_offs;
  job->csr.idx = s->d_ridx;
  job->csr.sqd = s->d_rsqd;
  job->csr.total = s->r_offs.empty() ? 0 : s->r_offs.back();
}

int ndt_rs_radius(NdtRadiusJob* job) {
  ndt_rs_bind(job->s, job->cloud);
  long long total = 0;
  if (const int rc = search_radius_core(job->s, reinterpret_cast<const float*>(job->q), job->n, 16, job->radius, 0, nullptr, &total)) return ndt_fail(rc, "radius search: " + g_search_err);
  ndt_rs_csr(job);
  return GORIO_OK;
}

int ndt_rs_radius_batch(NdtRadiusJob* jobs, int count, int* launches, int* syncs) {
  std::vector<SearchBatchJob> sj((size_t)count);
  for (int j = 0; j < count; ++j) {
    ndt_rs_bind(jobs[j].s, jobs[j].cloud);
    sj[j] = SearchBatchJob{jobs[j].s, reinterpret_cast<const float*>(jobs[j].q), jobs[j].n, 16, jobs[j].radius, 0, nullptr, 0};
  }
  SearchBatchStats st;
  if (const int rc = search_radius_batch_core(sj.data(), count, &st)) return ndt_fail(rc, "radius search: " + g_search_err);
  for (int j = 0; j < count; ++j) ndt_rs_csr(&jobs[j]);
  *launches += st.launches;
  *syncs += st.syncs;
  return GORIO_OK;
}

const std::vector<long long>& ndt_rs_host_offsets(const gorio_search_handle* s) { return s->r_offs; }

}  // namespace
