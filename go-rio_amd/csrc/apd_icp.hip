// apd_icp.hip -- ICP (pcl::IterativeClosestPoint, REG:72-79) as method GORIO_METHOD_ICP of the registration handle.  Included at the end of
// apd_api.hip: upload, search index, the exact 1-NN search, fitness score and hand-offs are the handle's.  The algorithm is the one fixed
// in include/gorio_apd.h ("GORIO_METHOD_ICP"): no k-NN lists, no covariances.
//
//   icp_recip_batch_kernel   reciprocal mode only: the exact 1-NN of every matched target point among the points of the moved copy
//   icp_pairs_batch_kernel   per 256-point block: q = transformation * p with the float arithmetic the search used, committed as the new
//                            working copy in both orders the searches read; gate, reciprocal flag, corr / sqd; 17 doubles per block
//                            (count, sum d^2, sum q, sum t, sum t q^T) reduced wave -> block, one partial per block, no atomics
//   icp_fold_batch_kernel    the block partials of every job added in block order
// The working copy is moved lazily: the search of iteration k + 1 runs on the stored copy with Tf = transformation of iteration k (the
// search kernels transform their queries), and the pairs kernel of iteration k + 1 re-derives the same q and stores it.  The first
// iteration reads the source itself with Tf = guess, so no launch prepares the copy.
// The loop of computeTransformation and DefaultConvergenceCriteria runs on the host as one resumable machine per handle (IcpMachine).
// gorio_apd_align drives one through the batched path with count = 1, so single and batched aligns share every kernel body and every sum.

namespace gorio {

// One handle's correspondence pass of a round.  Workgroups [first, first + nwg) of the launch belong to it; blocks b < nblk cover source
// points and write the partial slot first + b, the blocks behind them only move padding of the index-ordered copy.
struct IcpJob {
  const float *ix, *iy, *iz;  // the copy the search read (the source itself in the first iteration)
  float *ox, *oy, *oz;        // the working copy
  const float4* s4_in;        // the same in search-index order (x, y, z, original index bits), or null (exhaustive search)
  float4* s4_out;
  const float4* tgt;
  unsigned long long* best_key;
  int* corr;
  float* sqd;
  int* rflag;                 // reciprocal mode: 1 = the matched target point's nearest point of the moved copy is this one
  TfArg tf;                   // transformation of the previous iteration (the guess in the first)
  double thr2;                // corr_dist_threshold^2
  int n, n_tgt, n_spad;
  int recip;
  int first, nblk, nwg;
  int pad0_;
};

constexpr int kIcpSums = 17;

// grid: the reciprocal jobs' source blocks, block 256.  Lane = source point i with search winner j: the lowest-index nearest point of
// target j among q_k = tf * p_k, k < n (the distances are those of the forward search: sqdist3 is even in its difference).
__global__ __launch_bounds__(256) void icp_recip_batch_kernel(const IcpJob* __restrict__ jobs, const BlockRef* __restrict__ wg) {
  __shared__ float s_x[256], s_y[256], s_z[256];
  const BlockRef w = wg[blockIdx.x];
  const IcpJob& j = jobs[w.job];
  const int n = j.n;
  const int i = w.blk * 256 + threadIdx.x;
  bool live = false;
  float tx = 0.f, ty = 0.f, tz = 0.f;
  if (i < n) {
    const unsigned long long key = j.best_key[i];
    const int t = (int)(unsigned int)(key & 0xffffffffu);
    if (key != ~0ull && t >= 0 && t < j.n_tgt) {
      const float4 p = j.tgt[t];
      tx = p.x; ty = p.y; tz = p.z;
      live = true;
    }
  }
  float best = INFINITY;
  int bk = -1;
  for (int base = 0; base < n; base += 256) {
    const int k = base + threadIdx.x;
    __syncthreads();
    if (k < n) {
      float a, b, c;
      transform_f(j.tf.m, j.ix[k], j.iy[k], j.iz[k], a, b, c);
      s_x[threadIdx.x] = a; s_y[threadIdx.x] = b; s_z[threadIdx.x] = c;
    }
    __syncthreads();
    const int m = n - base < 256 ? n - base : 256;
    if (live)
      for (int u = 0; u < m; ++u) {
        const float d = sqdist3(tx, ty, tz, s_x[u], s_y[u], s_z[u]);
        if (d < best) { best = d; bk = base + u; }  // ascending k, strict: ties stay on the lowest index
      }
  }
  if (i < n) j.rflag[i] = (live && bk == i) ? 1 : 0;
}

// The work of ONE workgroup of 256 lanes on block `block` of job j.  s_red: 4 * kIcpSums doubles of LDS.
__device__ __forceinline__ void icp_pairs_block(const IcpJob& j, int block, double* s_red, double* __restrict__ out) {
  const int i = block * 256 + threadIdx.x;
  if (j.s4_in && i < j.n_spad) {  // the index-ordered copy, by sorted position; positions >= n are padding
    float4 v = j.s4_in[i];
    if (i < j.n) {
      float a, b, c;
      transform_f(j.tf.m, v.x, v.y, v.z, a, b, c);
      v.x = a; v.y = b; v.z = c;
    }
    j.s4_out[i] = v;
  }
  if (block >= j.nblk) return;  // uniform over the workgroup
  double v[kIcpSums];
#pragma unroll
  for (int q = 0; q < kIcpSums; ++q) v[q] = 0.0;
  if (i < j.n) {
    float qx, qy, qz;
    transform_f(j.tf.m, j.ix[i], j.iy[i], j.iz[i], qx, qy, qz);
    j.ox[i] = qx; j.oy[i] = qy; j.oz[i] = qz;
    const unsigned long long key = j.best_key[i];
    j.best_key[i] = ~0ull;  // re-armed for the next search
    const float d = __uint_as_float((unsigned int)(key >> 32));
    const int t = (int)(unsigned int)(key & 0xffffffffu);
    const bool found = key != ~0ull && t >= 0 && t < j.n_tgt;
    bool pair = found && !((double)d > j.thr2);
    if (j.recip) pair = pair && j.rflag[i] != 0;
    j.corr[i] = pair ? t : -1;
    j.sqd[i] = pair ? d : INFINITY;
    if (pair) {
      const float4 p = j.tgt[t];
      const double q0 = (double)qx, q1 = (double)qy, q2 = (double)qz, t0 = (double)p.x, t1 = (double)p.y, t2 = (double)p.z;
      v[0] = 1.0;
      v[1] = (double)d;
      v[2] = q0; v[3] = q1; v[4] = q2;
      v[5] = t0; v[6] = t1; v[7] = t2;
      v[8] = t0 * q0; v[9] = t0 * q1; v[10] = t0 * q2;  // products of two floats: exact in double
      v[11] = t1 * q0; v[12] = t1 * q1; v[13] = t1 * q2;
      v[14] = t2 * q0; v[15] = t2 * q1; v[16] = t2 * q2;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < kIcpSums; ++q) {
    const double s = wave_sum(v[q]);
    if (lane == 0) s_red[wave * kIcpSums + q] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < kIcpSums) {
    const int q = threadIdx.x;
    out[q] = ((s_red[q] + s_red[kIcpSums + q]) + s_red[2 * kIcpSums + q]) + s_red[3 * kIcpSums + q];
  }
}

// grid: the sum over the round's jobs of nwg, block 256.  wg[blockIdx.x] = (job, job-local block) of the round table (batch_rounds.h):
// job < number of jobs, blk < jobs[job].nwg; the partial buffer holds a slot for every workgroup of the launch.
__global__ __launch_bounds__(256) void icp_pairs_batch_kernel(const IcpJob* __restrict__ jobs, const BlockRef* __restrict__ wg, double* __restrict__ partials) {
  __shared__ double s_red[4 * kIcpSums];
  const BlockRef w = wg[blockIdx.x];
  const IcpJob& j = jobs[w.job];
  icp_pairs_block(j, w.blk, s_red, partials + (size_t)(j.first + w.blk) * kIcpSums);
}

// grid: the round's jobs, block 64.  Lane q adds the job's partials of value q in block order into out[17 job + q].
__global__ __launch_bounds__(64) void icp_fold_batch_kernel(const IcpJob* __restrict__ jobs, const double* __restrict__ partials, double* __restrict__ out) {
  const IcpJob& j = jobs[blockIdx.x];
  fold_wave<kIcpSums>(partials + (size_t)j.first * kIcpSums, j.nblk, out + (size_t)blockIdx.x * kIcpSums);
}

}  // namespace gorio

namespace {

void icp_mul4f(const float* a, const float* b, float* c) {  // row-major 4x4 float product, sums left to right
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      float s = a[r * 4] * b[q];
      for (int k = 1; k < 4; ++k) s = s + a[r * 4 + k] * b[k * 4 + q];
      c[r * 4 + q] = s;
    }
}

// Singular pairs of a 3x3 (row-major) by one-sided fp64 Jacobi: the columns of A V are rotated until they are orthogonal; their norms
// are the singular values.  On return sv[] is descending, u / v hold the matching columns u_k, v_k as rows; u_k is valid where sv[k] > 0.
void icp_svd3(const double* A, double* sv, double u[3][3], double v[3][3]) {
  double a[3][3], w[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // a[c] / w[c]: column c of A V / of V
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) a[c][r] = A[r * 3 + c];
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double alpha = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2];
        const double beta = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + a[q][2] * a[q][2];
        const double gamma = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + a[p][2] * a[q][2];
        if (gamma == 0.0 || std::fabs(gamma) <= 1e-16 * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        double t = 1.0 / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
        if (zeta < 0.0) t = -t;
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double x = a[p][r], y = a[q][r];
          a[p][r] = c * x - s * y;
          a[q][r] = s * x + c * y;
          const double vx = w[p][r], vy = w[q][r];
          w[p][r] = c * vx - s * vy;
          w[q][r] = s * vx + c * vy;
        }
      }
    if (!rotated) break;
  }
  double nrm[3];
  int ord[3] = {0, 1, 2};
  for (int c = 0; c < 3; ++c) nrm[c] = std::sqrt((a[c][0] * a[c][0] + a[c][1] * a[c][1]) + a[c][2] * a[c][2]);
  std::stable_sort(ord, ord + 3, [&](int x, int y) { return nrm[x] > nrm[y]; });
  for (int k = 0; k < 3; ++k) {
    const int c = ord[k];
    sv[k] = nrm[c];
    for (int r = 0; r < 3; ++r) {
      v[k][r] = w[c][r];
      u[k][r] = nrm[c] > 0.0 ? a[c][r] / nrm[c] : 0.0;
    }
  }
}

void icp_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The rigid transform of the 17 sums (Umeyama without scale, evaluated in double, rounded once to float): T row-major 4x4.
// R = U S V^T with S = diag(1, 1, det(U) det(V)): that is sign(det Sigma) at full rank and Umeyama's rank-2 rule otherwise, and it needs
// only the two leading singular pairs -- u_3 s_33 v_3^T = (u_1 x u_2)(v_1 x v_2)^T.
void icp_estimate(const double* s, float* T) {
  const double n = s[0];
  const double qm[3] = {s[2] / n, s[3] / n, s[4] / n}, tm[3] = {s[5] / n, s[6] / n, s[7] / n};
  double sig[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) sig[r * 3 + c] = s[8 + r * 3 + c] / n - tm[r] * qm[c];
  double sv[3], u[3][3], v[3][3];
  icp_svd3(sig, sv, u, v);
  {  // u_2 orthogonal to u_1 to the last bit that matters, then the third pair by cross products
    const double d = (u[0][0] * u[1][0] + u[0][1] * u[1][1]) + u[0][2] * u[1][2];
    double nn = 0.0;
    for (int r = 0; r < 3; ++r) { u[1][r] -= d * u[0][r]; nn += u[1][r] * u[1][r]; }
    nn = std::sqrt(nn);
    for (int r = 0; r < 3; ++r) u[1][r] = nn > 0.0 ? u[1][r] / nn : 0.0;
  }
  icp_cross(u[0], u[1], u[2]);
  icp_cross(v[0], v[1], v[2]);
  double R[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r * 3 + c] = (u[0][r] * v[0][c] + u[1][r] * v[1][c]) + u[2][r] * v[2][c];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T[r * 4 + c] = (float)R[r * 3 + c];
    T[r * 4 + 3] = (float)(tm[r] - ((R[r * 3] * qm[0] + R[r * 3 + 1] * qm[1]) + R[r * 3 + 2] * qm[2]));
  }
  T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// computeTransformation with DefaultConvergenceCriteria as a machine that stops wherever it needs the device: for one correspondence
// pass on the copy moved by Tr.  The caller answers with pass_done().
struct IcpMachine {
  gorio_apd* h = nullptr;
  bool finished = true;
  float Tr[16];     // what the next pass moves the stored copy by: the guess first, then `transformation`
  float fin[16];    // final_transformation_
  bool conv = false;
  int nr = 0, similar = 0;
  double prev_mse = DBL_MAX;

  void begin(gorio_apd* handle, const float* g) {
    h = handle;
    for (int i = 0; i < 16; ++i) Tr[i] = fin[i] = g[i];
    conv = false;
    nr = 0;
    similar = 0;
    prev_mse = DBL_MAX;
    finished = false;
    h->icp_iterations = 0; h->icp_state = 0; h->icp_mse = 0.0; h->icp_pairs = -1; h->icp_passes = 0;
  }
  bool done() const { return finished; }
  void finish(int state, bool converged) {
    h->icp_state = state;
    conv = converged;
    finished = true;
  }
  // s: the 17 sums of the pass
  void pass_done(const double* s) {
    const gorio_apd_params& p = h->params;
    const int pairs = (int)s[0];
    ++h->icp_passes;
    h->icp_pairs = pairs;
    h->corr_valid = true;
    h->omega_valid = false;
    if (pairs < 3) {
      h->err = "ICP: fewer than 3 correspondences";
      finish(5, false);
      return;
    }
    icp_estimate(s, Tr);
    float nf[16];
    icp_mul4f(Tr, fin, nf);
    for (int i = 0; i < 16; ++i) fin[i] = nf[i];
    ++nr;
    h->icp_iterations = nr;
    const double mse = s[1] / s[0];
    h->icp_mse = mse;
    const double rot_thr = h->icp_rot_eps > 0.0 ? h->icp_rot_eps : 1.0 - p.transformation_epsilon;
    const double trans_thr = p.transformation_epsilon, rel_thr = h->icp_fit_eps, abs_thr = 1e-12;
    const int max_similar = 0;
    if (nr >= p.max_iterations) return finish(1, true);
    bool is_similar = false;
    const double cos_angle = 0.5 * ((((double)Tr[0] + (double)Tr[5]) + (double)Tr[10]) - 1.0);
    const double t2 = ((double)Tr[3] * (double)Tr[3] + (double)Tr[7] * (double)Tr[7]) + (double)Tr[11] * (double)Tr[11];
    if (cos_angle >= rot_thr && t2 <= trans_thr) {
      if (similar >= max_similar) return finish(2, true);
      is_similar = true;
    }
    if (std::fabs(mse - prev_mse) < abs_thr) {
      if (similar >= max_similar) return finish(3, true);
      is_similar = true;
    }
    if (std::fabs(mse - prev_mse) / prev_mse < rel_thr) {
      if (similar >= max_similar) return finish(4, true);
      is_similar = true;
    }
    similar = is_similar ? similar + 1 : 0;
    prev_mse = mse;
  }
  void results(float* T_out, int* converged, int* nr_iterations, int* n_linearize) const {
    for (int i = 0; i < 16; ++i) T_out[i] = fin[i];
    if (converged) *converged = conv ? 1 : 0;
    if (nr_iterations) *nr_iterations = nr;
    if (n_linearize) *n_linearize = h->icp_passes;
  }
};

int icp_check_ready(gorio_apd* h) {
  if (!h->src->present) return fail(h, GORIO_ERR_STATE, "no input source set (setInputSource)");
  if (!h->tgt->present) return fail(h, GORIO_ERR_STATE, "no input target set (setInputTarget)");
  if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "ICP has no sharded-source mode");
  return GORIO_OK;
}

int icp_reserve(gorio_apd* h) {
  const int n = h->src->n;
  const size_t cap = n + n / 8 + 256;
  HIP_TRY(h, reserve_group(h->icp_cap, n, cap, h->icp_w, 3 * cap, h->icp_s4, cap + 1024, h->icp_rflag, cap));
  return GORIO_OK;
}

struct IcpRounds {  // the round table of run_rounds
  using Job = IcpJob;
  static constexpr int kSums = kIcpSums;
  static constexpr bool kCounts = false, kSecondList = true;  // the second list: the source blocks of the reciprocal jobs
  static void fold(int njobs, hipStream_t stream, const IcpJob* jobs, const double* part, const int*, double* out, int*) { icp_fold_batch_kernel<<<njobs, 64, 0, stream>>>(jobs, part, out); }
};

// The lock-step rounds behind gorio_apd_align (count 1), gorio_apd_icp_align_batch and gorio_apd_icp_step (step_T != null: one pass of
// hs[0] on step_T * source, no machine).  Per round: one search launch, one reciprocal launch when a pending handle asks for it, one pairs
// launch, one fold launch, one copy back, one synchronisation -- on the stream and with the tables of hs[0].  ctr: the rounds and launches.
int icp_run(gorio_apd** hs, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations, int* n_linearize, const float* step_T, double* step_sums,
            RoundCounters& ctr) {
  gorio_apd* lead = hs[0];
  const bool pruned = lead->params.search == GORIO_SEARCH_PRUNED;
  if (int rc = batch_prepare_search(hs, count)) return rc;
  size_t max_wg = 0;
  const int armed = batch_arm_handles(hs, count, [&](int q) {
    const int cover = std::max(hs[q]->src->n, pruned ? hs[q]->src->idx_spad : 0);
    max_wg += (size_t)(cover + 255) / 256;
    return icp_reserve(hs[q]);
  });
  if (armed) return armed;
  if (batch_rounds::too_many_wg(max_wg, 32)) return fail(lead, GORIO_ERR_INVALID, "icp_align_batch: too many source points in one batch");
  if (int rc = ensure_batch(lead, count)) return rc;
  std::vector<IcpMachine> mc(count);
  if (!step_T)
    for (int q = 0; q < count; ++q) mc[q].begin(hs[q], guesses + (size_t)16 * q);
  std::vector<char> first_pass(count, 1);
  std::vector<PairDesc> descs(count);
  std::vector<PairState> states(count);
  bool stepped = false;
  auto tr_of = [&](int q) { return step_T ? step_T : mc[q].Tr; };
  auto pending = [&](int q) { return (step_T ? !stepped : !mc[q].done()) ? 0 : -1; };
  auto fill = [&](int, int q, IcpJob& j) {
    gorio_apd* h = hs[q];
    const DevCloud& s = *h->src;
    const int n = s.n;
    float* o = h->icp_w;
    const size_t st = h->icp_w.cap() / 3;
    const bool first = first_pass[q] != 0;
    first_pass[q] = 0;
    j.ix = first ? s.x.get() : o; j.iy = first ? s.y.get() : o + st; j.iz = first ? s.z.get() : o + 2 * st;
    j.ox = o; j.oy = o + st; j.oz = o + 2 * st;
    j.s4_in = pruned ? (first ? s.idx_s4.get() : h->icp_s4.get()) : nullptr;
    j.s4_out = h->icp_s4;
    j.tgt = h->tgt->p4;
    j.best_key = h->best_key;
    j.corr = h->corr;
    j.sqd = h->sqd;
    j.rflag = h->icp_rflag;
    for (int i = 0; i < 12; ++i) j.tf.m[i] = tr_of(q)[i];
    j.thr2 = h->params.corr_dist_threshold * h->params.corr_dist_threshold;
    j.n = n;
    j.n_tgt = h->tgt->n;
    j.n_spad = pruned ? s.idx_spad : 0;
    j.recip = h->icp_reciprocal;
    j.nwg = (std::max(n, j.n_spad) + 255) / 256;
    return batch_rounds::JobShape{(n + 255) / 256, j.nwg, j.recip != 0};
  };
  auto launch = [&](const RoundView<IcpJob>& v, int& launches) {
    const int njobs = v.plan.njobs;
    long waves = 0;
    int max_n = 0, max_m = 0, max_splits = 1;
    for (int q : v.order) {
      waves += (hs[q]->src->n + 63) / 64;
      max_n = std::max(max_n, hs[q]->src->n);
      max_m = std::max(max_m, hs[q]->tgt->n);
    }
    for (int k = 0; k < njobs; ++k) {  // the searches read the copy the job reads
      const IcpJob& j = v.jobs[k];
      fill_moved_search(hs[v.order[k]], descs[k], states[k], lead->d_states_batch + k, waves, j.ix, j.iy, j.iz, j.s4_in, tr_of(v.order[k]));
      max_splits = std::max(max_splits, descs[k].nn_splits);
    }
    if (int rc2 = upload_staged(lead, lead->pin_desc, lead->d_desc, descs.data(), sizeof(PairDesc) * njobs)) return rc2;
    if (int rc2 = upload_staged(lead, lead->pin_states, lead->d_states_batch, states.data(), sizeof(PairState) * njobs)) return rc2;
    launch_nn(lead, lead->d_desc, dim3((max_n + 255) / 256, max_splits, njobs), roundup(max_n, 512), njobs, max_m, -1, true);
    if (v.plan.second > 0) icp_recip_batch_kernel<<<v.plan.second, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs + v.plan.wg);
    icp_pairs_batch_kernel<<<v.plan.wg, 256, 0, lead->stream>>>(v.d_jobs, v.d_refs, lead->round.part);
    launches += v.plan.second > 0 ? 3 : 2;
    return (int)GORIO_OK;
  };
  auto consume = [&](int, int q, const double* sums, int) {
    if (!step_T) return mc[q].pass_done(sums);
    std::memcpy(step_sums, sums, sizeof(double) * kIcpSums);
    lead->icp_pairs = (int)sums[0];
    lead->corr_valid = true;
    lead->omega_valid = false;
    stepped = true;
  };
  if (int rc = run_rounds<IcpRounds>(lead, count, max_wg, ctr, pending, fill, launch, consume)) return rc;
  if (!step_T)
    for (int q = 0; q < count; ++q)
      mc[q].results(T_out + (size_t)16 * q, converged ? converged + q : nullptr, nr_iterations ? nr_iterations + q : nullptr, n_linearize ? n_linearize + q : nullptr);
  resolve_stage_events(lead);
  return GORIO_OK;
}

int icp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!guess || !T_out) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = icp_check_ready(h);
  if (rc) return rc;
  gorio_apd* hs[1] = {h};
  RoundCounters ctr;  // dropped: gorio_apd_icp_batch_diag speaks of batches only
  rc = icp_run(hs, 1, guess, T_out, converged, nr_iterations, n_linearize, nullptr, nullptr, ctr);
  if (rc) return rc;
  if (H_out) std::memset(H_out, 0, sizeof(double) * 36);
  return GORIO_OK;
}

}  // namespace

extern "C" {

int gorio_apd_set_icp_params(gorio_apd_t* h, int use_reciprocal, double euclidean_fitness_epsilon, double transformation_rotation_epsilon) {
  if (!h) return GORIO_ERR_INVALID;
  if (use_reciprocal != 0 && use_reciprocal != 1) return fail(h, GORIO_ERR_INVALID, "set_icp_params: use_reciprocal must be 0 or 1");
  if (std::isnan(euclidean_fitness_epsilon) || std::isnan(transformation_rotation_epsilon)) return fail(h, GORIO_ERR_INVALID, "set_icp_params: an epsilon is not a number");
  h->icp_reciprocal = use_reciprocal;
  h->icp_fit_eps = euclidean_fitness_epsilon;
  h->icp_rot_eps = transformation_rotation_epsilon;
  return GORIO_OK;
}

int gorio_apd_get_icp_params(const gorio_apd_t* h, int* use_reciprocal, double* euclidean_fitness_epsilon, double* transformation_rotation_epsilon) {
  if (!h) return GORIO_ERR_INVALID;
  if (use_reciprocal) *use_reciprocal = h->icp_reciprocal;
  if (euclidean_fitness_epsilon) *euclidean_fitness_epsilon = h->icp_fit_eps;
  if (transformation_rotation_epsilon) *transformation_rotation_epsilon = h->icp_rot_eps;
  return GORIO_OK;
}

int gorio_apd_icp_diag(const gorio_apd_t* h, int* iterations, int* state, double* mse, int* pairs) {
  if (!h) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_ICP) return fail(const_cast<gorio_apd_t*>(h), GORIO_ERR_STATE, "icp_diag: the handle's method is not GORIO_METHOD_ICP");
  if (iterations) *iterations = h->icp_iterations;
  if (state) *state = h->icp_state;
  if (mse) *mse = h->icp_mse;
  if (pairs) *pairs = h->icp_pairs;
  return GORIO_OK;
}

int gorio_apd_icp_step(gorio_apd_t* h, const float T16[16], int* pairs, double sums17[17], float T_est16[16]) {
  if (!h || !T16) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_ICP) return fail(h, GORIO_ERR_STATE, "icp_step: the handle's method is not GORIO_METHOD_ICP");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = icp_check_ready(h);
  if (rc) return rc;
  gorio_apd* hs[1] = {h};
  double s[kIcpSums];
  RoundCounters ctr;
  rc = icp_run(hs, 1, nullptr, nullptr, nullptr, nullptr, nullptr, T16, s, ctr);
  if (rc) return rc;
  if (pairs) *pairs = (int)s[0];
  if (sums17) std::memcpy(sums17, s, sizeof(s));
  if (T_est16) {
    if (s[0] >= 3.0) icp_estimate(s, T_est16);
    else
      for (int i = 0; i < 16; ++i) T_est16[i] = (i % 5 == 0) ? 1.f : 0.f;  // fewer than 3 pairs: no estimate
  }
  return GORIO_OK;
}

int gorio_apd_icp_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations) {
  if (count == 0) return GORIO_OK;
  if (int rc = batch_front_door("icp_align_batch", handles, count, guesses, T_out, true, [](const gorio_apd* h) { return h->method == GORIO_METHOD_ICP; }, "the handle's method is not GORIO_METHOD_ICP", icp_check_ready)) return rc;
  gorio_apd* lead = handles[0];
  HIP_TRY(lead, hipSetDevice(lead->device));
  RoundCounters ctr;
  const int rc = icp_run(handles, count, guesses, T_out, converged, nr_iterations, nullptr, nullptr, nullptr, ctr);
  if (rc) return rc;
  lead->icp_b_rounds = ctr.rounds;
  lead->icp_b_launches = ctr.launches;
  return GORIO_OK;
}

int gorio_apd_icp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches) {
  if (!lead) return GORIO_ERR_INVALID;
  if (lead->method != GORIO_METHOD_ICP) return fail(const_cast<gorio_apd_t*>(lead), GORIO_ERR_STATE, "icp_batch_diag: the handle's method is not GORIO_METHOD_ICP");
  if (rounds) *rounds = lead->icp_b_rounds;
  if (launches) *launches = lead->icp_b_launches;
  return GORIO_OK;
}

}  // extern "C"
