// Host pipeline of the Gauss-Newton / LM family (included by apd_api.hip, inside its anonymous namespace): the five methods that run on
// the device shell lm_solve_body<METHOD> with PairDesc / PairState.  One call -- a single align, a batch, a parity hook -- is an LsqBatch
// and walks four stages: validate (ready checks), prepare (derived products), upload (descriptors, pair tables, states), then the
// launches search / linearize / solve.  Each stage switches on the family once.

enum class LsqFamily {
  PointPairs,   // APD-GICP, FastGICP: a nearest-neighbour search pairs source points with target points
  VoxelPairs,   // FastVGICP: (source point, offset) slots into the double voxel map, looked up by the linearisation (VG:73-116)
  FloatVoxels,  // NDTCuda, FastVGICPCuda: (item, offset) slots into a float voxel map; no per-point search state, no search index
};

LsqFamily lsq_family(const gorio_apd* h) {
  if (is_voxf(h)) return LsqFamily::FloatVoxels;
  return h->method == GORIO_METHOD_VGICP ? LsqFamily::VoxelPairs : LsqFamily::PointPairs;
}

// One call's view of `count` handles of one family, led by hs[0]: its stream, its batch arrays, its parameters.
struct LsqBatch {
  gorio_apd** hs;
  int count;
  gorio_apd* lead;
  LsqFamily family;
  std::vector<PairDesc> descs;
  std::vector<PairState> states;
  int max_n = 0, max_m = 0;
  ApdConsts cst;
  dim3 g_nn, g_lin, g_lm, g_slots;  // searches, per-point linearisations, one workgroup per pair, per-slot linearisations

  LsqBatch(gorio_apd** hs_, int count_) : hs(hs_), count(count_), lead(hs_[0]), family(lsq_family(hs_[0])) {}

  int validate() {
    for (int q = 0; q < count; ++q)
      if (hs[q] && hs[q]->comm && count != 1) return fail(lead, GORIO_ERR_INVALID, "a handle with a communicator (sharded source) cannot be part of a batch");
    for (int q = 0; q < count; ++q)
      if (hs[q] && hs[q]->method == GORIO_METHOD_GICP_OMP) return fail(lead, GORIO_ERR_UNSUPPORTED, "align_batch: GICP_OMP handles batch through gorio_apd_gicp_omp_align_batch (the BFGS shell is not the Gauss-Newton / LM one)");
    for (int q = 0; q < count; ++q)
      if (hs[q] && hs[q]->method == GORIO_METHOD_ICP) return fail(lead, GORIO_ERR_UNSUPPORTED, "align_batch: ICP handles batch through gorio_apd_icp_align_batch");
    for (int q = 0; q < count; ++q)
      if (hs[q] && is_mp(hs[q])) return fail(lead, GORIO_ERR_UNSUPPORTED, "align_batch: FastGICPMultiPoints handles are batched by gorio_apd_gicp_mp_align_batch (their rounds run a batched radius search, not this call's pair searches)");
    std::unordered_set<gorio_apd*> distinct;
    for (int q = 0; q < count; ++q) {
      gorio_apd* h = hs[q];
      if (!h) return fail(lead, GORIO_ERR_INVALID, "null handle in batch");
      if (h->device != lead->device) return fail(lead, GORIO_ERR_INVALID, "all handles of a batch must live on one device");
      if (!distinct.insert(h).second) return fail(lead, GORIO_ERR_INVALID, "the same handle appears twice in a batch (its buffers would be raced on)");
      // one launch set advances all pairs: everything but cl_weight_points (per handle) must agree with the first handle
      gorio_apd_params a = h->params, b = lead->params;
      a.cl_weight_points = b.cl_weight_points = 0;
      if (std::memcmp(&a, &b, sizeof(a)) != 0) return fail(lead, GORIO_ERR_INVALID, "all handles of a batch must carry the same parameters (cl_weight_points excepted)");
      if (h->method != lead->method) return fail(lead, GORIO_ERR_INVALID, "all handles of a batch must use the same registration method (gorio_apd_set_method)");
      int rc = GORIO_OK;
      switch (family) {
        case LsqFamily::PointPairs:
          rc = check_ready(h);
          break;
        case LsqFamily::VoxelPairs:
          if (h->voxel_resolution != lead->voxel_resolution || h->voxel_search != lead->voxel_search || h->voxel_mode != lead->voxel_mode)
            return fail(lead, GORIO_ERR_INVALID, "all FastVGICP handles of a batch must carry the same voxel_resolution / voxel_search / voxel_mode");
          rc = check_ready(h);
          break;
        case LsqFamily::FloatVoxels:
          if (is_ndtc(h) && !ndtc_same_settings(h, lead))
            return fail(lead, GORIO_ERR_INVALID, "all NDTCuda handles of a batch must carry the same resolution / neighbour offsets / distance mode");
          if (is_vgc(h) && !vgc_same_settings(h, lead))
            return fail(lead, GORIO_ERR_INVALID, "all FastVGICPCuda handles of a batch must carry the same resolution / neighbour offsets / neighbour method / kernel parameters");
          rc = is_vgc(h) ? vgc_ready(h) : ndtc_ready(h);
          break;
      }
      if (rc) return hand_over(lead, h, rc);
    }
    return GORIO_OK;
  }

  // Per-point search state, search indices and covariances of the two families that hold double covariances per point (APD:149-154).
  int points_and_covariances() {
    std::vector<std::pair<gorio_apd*, DevCloud*>> todo, all;
    std::unordered_set<DevCloud*> seen;  // a target shared by many handles of the batch is estimated once
    for (int q = 0; q < count; ++q) {
      gorio_apd* h = hs[q];
      if (int rc = ensure_points(h, h->src->n)) return rc;
      if (h->src->cov_count != h->src->n && seen.insert(h->src.get()).second) todo.emplace_back(h, h->src.get());
      if (h->tgt->cov_count != h->tgt->n && seen.insert(h->tgt.get()).second) todo.emplace_back(h, h->tgt.get());
      all.emplace_back(h, h->src.get());
      all.emplace_back(h, h->tgt.get());
    }
    if (lead->params.search == GORIO_SEARCH_PRUNED) {  // the search indices first, for ALL clouds of the call in one build: the kd chunk size is chosen by the whole set (run_index_build)
      // FastVGICP runs no nearest-neighbour search: only the k-NN covariance stage of the stale clouds reads an index
      if (int rc = run_index_build(lead, family == LsqFamily::VoxelPairs ? todo : all)) return rc;
    }
    return run_covariances(lead, todo);
  }

  int prepare() {
    if (family != LsqFamily::FloatVoxels)  // NDTCuda makes no covariances, FastVGICPCuda float ones of its own (ensure_vgc_pair)
      if (int rc = points_and_covariances()) return rc;
    for (int q = 0; q < count; ++q) {  // a shared cloud's map is built once: the second sharer finds it valid
      gorio_apd* h = hs[q];
      int rc = GORIO_OK;
      switch (family) {
        case LsqFamily::PointPairs:
          break;
        case LsqFamily::VoxelPairs:  // VG:120-123
          rc = build_voxelmap(h, *h->tgt, h->voxel_resolution, h->voxel_mode);
          if (!rc) rc = ensure_voxel_pair(h);
          break;
        case LsqFamily::FloatVoxels:  // create_voxelmaps (NI:76-79)
          rc = is_vgc(h) ? ensure_vgc_pair(h) : ensure_ndtc_pair(h);
          break;
      }
      if (rc) return hand_over(lead, h, rc);
    }
    return reserve_tables();
  }

  // the lead's batch arrays: the pair table of a slot family, then descriptors and states
  int reserve_tables() {
    if (family == LsqFamily::VoxelPairs) HIP_TRY(lead, lead->d_vox.reserve(count));
    if (family == LsqFamily::FloatVoxels) HIP_TRY(lead, lead->d_ndtc.reserve(count));
    return ensure_batch(lead, count);
  }

  // Descriptors and pair tables over what the handles HOLD (compute_error reads the stale pairs of the last linearise), through the
  // lead's pinned staging.  poses ([count][16], row-major): the states start there (LSQ:56), the search's key buffers are armed and the
  // handles' correspondences count as held.  poses == nullptr: the states stay as they are.
  int upload(const double* poses, int write_omega) {
    long total_src_waves = 0;
    for (int q = 0; q < count; ++q) {
      total_src_waves += (hs[q]->src->n + 63) / 64;
      max_n = std::max(max_n, hs[q]->src->n);
      max_m = std::max(max_m, hs[q]->tgt->n);
    }
    descs.resize(count);
    int max_splits = 1;
    size_t max_slots = 1;
    for (int q = 0; q < count; ++q) {
      const gorio_apd* h = hs[q];
      PairDesc& d = descs[q];
      fill_desc(hs[q], d, h->d_state, total_src_waves);
      size_t slots = 0;  // a slot family reduces one partial per 256 slots, not per 256 points
      switch (family) {
        case LsqFamily::PointPairs:
          break;
        case LsqFamily::VoxelPairs:
          slots = (size_t)h->src->n * h->v_n_off;
          d.partials = h->v_partials;
          break;
        case LsqFamily::FloatVoxels:
          slots = (size_t)h->ndtc_items * h->ndtc_slot_off;
          d.partials = h->ndtc_partials;
          break;
      }
      if (family != LsqFamily::PointPairs) d.nblk = (int)((slots + 255) / 256);
      max_slots = std::max(max_slots, slots);
      d.write_omega = write_omega;
      max_splits = std::max(max_splits, d.nn_splits);
    }
    if (int rc = upload_staged(lead, lead->pin_desc, lead->d_desc, descs.data(), sizeof(PairDesc) * count)) return rc;
    if (poses) {
      states.resize(count);
      for (int q = 0; q < count; ++q) {
        init_state(states[q], poses + (size_t)q * 16);
        hs[q]->corr_valid = true;
        hs[q]->omega_valid = write_omega != 0;  // never read in the FloatVoxels family
      }
      if (int rc = upload_staged(lead, lead->pin_states, lead->d_states_batch, states.data(), sizeof(PairState) * count)) return rc;
    }
    switch (family) {
      case LsqFamily::PointPairs:
        break;
      case LsqFamily::VoxelPairs: {
        std::vector<VoxPair> voxs(count);
        for (int q = 0; q < count; ++q) voxs[q] = make_vox_pair(hs[q], write_omega);
        if (int rc = upload_staged(lead, lead->pin_vox, lead->d_vox, voxs.data(), sizeof(VoxPair) * count)) return rc;
        break;
      }
      case LsqFamily::FloatVoxels: {
        std::vector<NdtcPair> prs(count);
        for (int q = 0; q < count; ++q) prs[q] = make_ndtc_pair(hs[q]);
        if (int rc = upload_staged(lead, lead->pin_ndtc, lead->d_ndtc, prs.data(), sizeof(NdtcPair) * count)) return rc;
        break;
      }
    }
    if (poses) {
      scatter_states_kernel<<<count, 64, 0, lead->stream>>>(lead->d_desc, lead->d_states_batch);
      if (family == LsqFamily::PointPairs) arm_keys_kernel<<<dim3(std::min(64, (max_n + 255) / 256), count), 256, 0, lead->stream>>>(lead->d_desc);
    }
    cst = make_consts(lead->params);
    g_nn = dim3((max_n + 255) / 256, max_splits, count);
    g_lin = dim3((max_n + 255) / 256, 1, count);
    g_lm = dim3(count);
    g_slots = dim3((unsigned int)((max_slots + 255) / 256), 1, count);
    return GORIO_OK;
  }

  // launch_index: position of the search inside its align, -1 outside an align loop (launch_nn).  False: this family runs no search.
  bool search(int launch_index) {
    if (family != LsqFamily::PointPairs) return false;
    launch_nn(lead, lead->d_desc, g_nn, roundup(max_n, 512), count, max_m, launch_index);
    return true;
  }

  // Gauss-Newton needs no error trials: its step can ride on the linearisation launch (the last workgroup of a pair runs it).
  // Levenberg-Marquardt keeps its own launch (an error trial wants the 1024 threads of lm_solve_kernel), and so do the slot families.
  bool fuse_gn() const { return family == LsqFamily::PointPairs && lead->fuse_step && lead->params.optimizer != GORIO_OPT_LEVENBERG_MARQUARDT; }

  // the compile-time variants behind one call (kMethodApd stays the instantiation every APD-GICP caller runs); the slot families look
  // their pairs up inside the linearisation, by the slot table HELD (ndtc_slot_d2d of the lead: the settings of a batch agree)
  void linearize(int fuse) {
    switch (family) {
      case LsqFamily::PointPairs:
        if (lead->method == GORIO_METHOD_GICP) linearize_kernel<kMethodGicp><<<g_lin, 256, 0, lead->stream>>>(lead->d_desc, cst, fuse);
        else linearize_kernel<kMethodApd><<<g_lin, 256, 0, lead->stream>>>(lead->d_desc, cst, fuse);
        break;
      case LsqFamily::VoxelPairs:
        vgicp_linearize_kernel<<<g_slots, 256, 0, lead->stream>>>(lead->d_desc, lead->d_vox);
        break;
      case LsqFamily::FloatVoxels:  // update_correspondences + compute_error (NI:82-85) in one launch
        if (lead->ndtc_slot_d2d == 2) vgc_linearize_kernel<<<g_slots, 256, 0, lead->stream>>>(lead->d_desc, lead->d_ndtc);
        else launch_ndtc_linearize(lead->ndtc_slot_d2d != 0, g_slots, lead->stream, lead->d_desc, lead->d_ndtc);
        break;
    }
  }

  // the shell: mode 0 = one optimiser iteration, 1 = fold the partials into H, b, y0 (linearize hook), 2 = the error at xi (compute_error hook)
  void solve(int mode) {
    switch (family) {
      case LsqFamily::PointPairs:
        if (lead->method == GORIO_METHOD_GICP) lm_solve_kernel<kMethodGicp><<<g_lm, 1024, 0, lead->stream>>>(lead->d_desc, cst, mode);
        else lm_solve_kernel<kMethodApd><<<g_lm, 1024, 0, lead->stream>>>(lead->d_desc, cst, mode);
        break;
      case LsqFamily::VoxelPairs:
        lm_solve_vgicp_kernel<<<g_lm, 1024, 0, lead->stream>>>(lead->d_desc, lead->d_vox, cst, mode);
        break;
      case LsqFamily::FloatVoxels:
        if (is_vgc(lead)) lm_solve_vgc_kernel<<<g_lm, 1024, 0, lead->stream>>>(lead->d_desc, lead->d_ndtc, cst, mode);
        else lm_solve_ndtc_kernel<<<g_lm, 1024, 0, lead->stream>>>(lead->d_desc, lead->d_ndtc, cst, mode);
        break;
    }
  }

  // Sharded source (PointPairs, count == 1; every rank makes the same calls): H, b and the error summed over the ranks, and this
  // rank's part of a trial error into d_red[28]
  int shard_sum(int mode) {
    shard_reduce_partials_kernel<<<1, 64, 0, lead->stream>>>(lead->d_desc, lead->d_red);
    NCCL_TRY(lead, rccl().AllReduce(lead->d_red, lead->d_red, 28, ncclDouble, ncclSum, lead->comm, lead->stream));  // THE collective: H, b, error
    shard_begin_kernel<<<1, 64, 0, lead->stream>>>(lead->d_desc, lead->d_red, cst, mode);
    return GORIO_OK;
  }
  int shard_trial_error(int mode) {
    if (lead->method == GORIO_METHOD_GICP) shard_trial_error_kernel<kMethodGicp><<<1, 1024, 0, lead->stream>>>(lead->d_desc, lead->d_red + 28, cst, mode);
    else shard_trial_error_kernel<kMethodApd><<<1, 1024, 0, lead->stream>>>(lead->d_desc, lead->d_red + 28, cst, mode);
    NCCL_TRY(lead, rccl().AllReduce(lead->d_red + 28, lead->d_red + 28, 1, ncclDouble, ncclSum, lead->comm, lead->stream));
    return GORIO_OK;
  }
};

void read_result(const PairState& s, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  for (int i = 0; i < 12; ++i) T_out[i] = (float)s.x0[i];  // LSQ:78
  T_out[12] = 0.f; T_out[13] = 0.f; T_out[14] = 0.f; T_out[15] = 1.f;
  if (H_out) std::memcpy(H_out, s.Hfin, sizeof(double) * 36);
  if (converged) *converged = s.converged;
  if (nr_iterations) *nr_iterations = s.nr_iterations;
  if (n_linearize) *n_linearize = s.n_linearize;
}

int align_impl(gorio_apd** hs, int count, const float* guesses, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!hs || count <= 0 || !guesses || !T_out) return GORIO_ERR_INVALID;
  gorio_apd* lead = hs[0];
  if (!lead) return GORIO_ERR_INVALID;
  HIP_TRY(lead, hipSetDevice(lead->device));
  LsqBatch B(hs, count);
  const bool lm = lead->params.optimizer == GORIO_OPT_LEVENBERG_MARQUARDT;
  const std::vector<double> poses(guesses, guesses + (size_t)count * 16);
  int rc = B.validate();
  if (!rc) rc = B.prepare();
  // Gauss-Newton never reads the Mahalanobis matrices back (only LM error trials and the parity hooks do): do not store them
  if (!rc) rc = B.upload(poses.data(), lm ? 1 : 0);
  if (rc) return rc;
  std::vector<PairState>& states = B.states;
  const int max_it = lead->params.max_iterations;
  if (lead->comm) {  // sharded source: the same loop, cut at the two all-reduces (count == 1, validate)
    for (int it = 0; it < max_it; ++it) {
      B.search(-1);
      B.linearize(0);
      if ((rc = B.shard_sum(0))) return rc;
      ++lead->allreduce_count;
      int trials = 0;
      bool active = lm;
      while (active) {
        // two trial slots per round trip: a Levenberg-Marquardt step is almost always decided by the first or second trial; every rank
        // reads the same flags, so every rank enqueues the same sequence of collectives
        for (int t = 0; t < 2 && trials < lead->params.lm_max_iterations; ++t, ++trials) {
          if ((rc = B.shard_trial_error(0))) return rc;
          ++lead->allreduce_count;
          shard_trial_decide_kernel<<<1, 64, 0, lead->stream>>>(lead->d_desc, lead->d_red + 28, B.cst, 0);
        }
        HIP_TRY(lead, hipMemcpyAsync(&states[0], lead->d_state, sizeof(PairState), hipMemcpyDeviceToHost, lead->stream));
        HIP_TRY(lead, hipStreamSynchronize(lead->stream));
        active = states[0].trial_active != 0 && trials < lead->params.lm_max_iterations;
      }
      if (lm) shard_trial_decide_kernel<<<1, 64, 0, lead->stream>>>(lead->d_desc, lead->d_red + 28, B.cst, 1);  // end-of-iteration bookkeeping
      HIP_TRY(lead, hipGetLastError());
      HIP_TRY(lead, hipMemcpyAsync(&states[0], lead->d_state, sizeof(PairState), hipMemcpyDeviceToHost, lead->stream));
      HIP_TRY(lead, hipStreamSynchronize(lead->stream));
      if (states[0].done) break;
    }
    read_result(states[0], T_out, H_out, converged, nr_iterations, n_linearize);
    if (states[0].lm_failed) lead->err = "lm not converged!!";
    resolve_stage_events(lead);
    return GORIO_OK;
  }
  int launched = 0;
  // Iterations between looks at the done flags (a look drains the stream): 4, 8, 16, 16, ... for the first batch of a handle; later
  // batches first enqueue as many iterations as the previous batch needed -- on like data that look is the only one.  A finished pair's
  // kernels return at once, so the schedule of the looks never changes a result.
  int chunk_iters = lead->align_budget > 0 ? lead->align_budget : 4;
  const bool fuse = B.fuse_gn();
  HIP_TRY(lead, lead->pin_looks.reserve(sizeof(PairState) * count, sizeof(PairState) * (count + count / 2)));
  while (launched < max_it) {
    const int todo_it = std::min(chunk_iters, max_it - launched);
    StageChain chain(lead);
    for (int it = 0; it < todo_it; ++it) {
      if (B.search(launched + it)) chain.mark(1);
      B.linearize(fuse ? 1 : 0);
      chain.mark(2);
      if (!fuse) {
        B.solve(0);
        chain.mark(3);
      }
    }
    launched += todo_it;
    chunk_iters = launched == todo_it && lead->align_budget > 0 ? 4 : std::min(16, chunk_iters * 2);  // after a budgeted first chunk: 4, 8, 16, ...
    HIP_TRY(lead, hipGetLastError());
    gather_states_kernel<<<count, 64, 0, lead->stream>>>(lead->d_desc, lead->d_states_batch);
    HIP_TRY(lead, hipMemcpyAsync(lead->pin_looks, lead->d_states_batch, sizeof(PairState) * count, hipMemcpyDeviceToHost, lead->stream));
    HIP_TRY(lead, hipStreamSynchronize(lead->stream));
    std::memcpy(states.data(), lead->pin_looks, sizeof(PairState) * count);
    bool all_done = true;
    for (int q = 0; q < count; ++q) all_done = all_done && states[q].done;
    if (all_done) break;
  }
  int need = 1;  // loop iterations the slowest pair used = its linearisations
  for (int q = 0; q < count; ++q) {
    need = std::max(need, states[q].n_linearize);
    read_result(states[q], T_out + (size_t)q * 16, H_out ? H_out + (size_t)q * 36 : nullptr, converged ? converged + q : nullptr, nr_iterations ? nr_iterations + q : nullptr,
                n_linearize ? n_linearize + q : nullptr);
    if (states[q].lm_failed) hs[q]->err = "lm not converged!!";  // LSQ:72 prints this to stderr
  }
  lead->align_budget = std::min(need, max_it);
  resolve_stage_events(lead);
  return GORIO_OK;
}

// gorio_apd_linearize behind its refusals.  NI:82-85, VI:170-173 for the slot families: update_correspondences(trans), then
// compute_error(trans, H, b) over the fresh pairs.
int lsq_linearize(gorio_apd* h, const double* T, double* H, double* b, double* error) {
  HIP_TRY(h, hipSetDevice(h->device));
  LsqBatch B(&h, 1);
  int rc = B.validate();
  if (!rc) rc = B.prepare();
  if (!rc) rc = B.upload(T, 1);
  if (rc) return rc;
  B.search(-1);
  B.linearize(0);
  if (h->comm) {  // every rank of the communicator makes this call; H, b and the error come back summed over all of them
    if ((rc = B.shard_sum(1))) return rc;
  } else {
    B.solve(1);
  }
  HIP_TRY(h, hipGetLastError());
  PairState& s = B.states[0];
  HIP_TRY(h, hipMemcpyAsync(&s, h->d_state, sizeof(s), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  resolve_stage_events(h);
  if (H && b) {
    std::memcpy(H, s.H, sizeof(double) * 36);
    std::memcpy(b, s.b, sizeof(double) * 6);
  }
  if (error) *error = s.y0;
  return GORIO_OK;
}

// gorio_apd_compute_error behind its refusals: the error at T over the pairs (and Mahalanobis matrices) HELD.  NC:162-177, VC:276-284
// for the slot families: the stale pairs and R_lin of the last linearise.
int lsq_compute_error(gorio_apd* h, const double* T, double* error) {
  HIP_TRY(h, hipSetDevice(h->device));
  LsqBatch B(&h, 1);
  if (!h->corr_valid || (B.family != LsqFamily::FloatVoxels && !h->omega_valid)) return fail(h, GORIO_ERR_STATE, "compute_error needs the correspondences and Mahalanobis matrices of a previous linearize (or LM align)");
  int rc = B.reserve_tables();  // a handle that has never led a call holds none
  if (!rc) rc = B.upload(nullptr, 1);
  if (rc) return rc;
  char* state = reinterpret_cast<char*>(h->d_state.get());
  HIP_TRY(h, hipMemcpyAsync(state + offsetof(PairState, xi), T, sizeof(double) * 16, hipMemcpyHostToDevice, h->stream));
  const void* yi = state + offsetof(PairState, yi);
  if (h->comm) {
    if ((rc = B.shard_trial_error(2))) return rc;
    yi = h->d_red + 28;
  } else {
    B.solve(2);
  }
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipMemcpyAsync(error, yi, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}
