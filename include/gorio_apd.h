/*
 * gorio_apd.h -- C ABI of the MI355X-native APD-GICP scan-matching back end (libgorio_amd.so).
 *
 * The reference has no FFI for this path: the seam is C++ virtual dispatch through
 * pcl::Registration<PointXYZINormal,PointXYZINormal>.  This header is the boundary a drop-in
 * fast_gicp::FastAPDGICP uses underneath that class surface (go-rio_amd/host/fast_gicp/gicp/fast_apdgicp.hpp in this
 * repository); every entry point cites the reference member it replaces.  Paths are relative to /root/reference:
 *   APDH = fast_apdgicp/include/fast_gicp/gicp/fast_apdgicp.hpp
 *   APD  = fast_apdgicp/include/fast_gicp/gicp/impl/fast_apdgicp_impl.hpp
 *   LSQH = fast_apdgicp/include/fast_gicp/gicp/lsq_registration.hpp
 *   LSQ  = fast_apdgicp/include/fast_gicp/gicp/impl/lsq_registration_impl.hpp
 *   REG  = 4DRadarSLAM/src/radar_graph_slam/registrations.cpp
 *
 * Conventions
 *  - plain pointers and sizes only; all host pointers are caller-owned and only read / written during the call.
 *  - 4x4 matrices are ROW-major (T[r*4+c]); pcl / Eigen matrices are column-major, the C++ shim transposes.
 *  - covariances cross the ABI as n * 16 doubles (Eigen::Matrix4d per point, symmetric, row/col 3 zero), exactly the
 *    element type of FastAPDGICP::source_covs_ / target_covs_ (APDH:109-110).
 *  - return 0 on success, negative gorio_status otherwise; gorio_apd_last_error() gives the text.
 *  - a handle is one FastAPDGICP object: not thread-safe, distinct handles are independent (SURVEY 8b "Threading").
 *  - there is no CPU fallback: every compute entry point fails with GORIO_ERR_NO_DEVICE when no HIP device is usable.
 */
#ifndef GORIO_APD_H
#define GORIO_APD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GORIO_OK = 0,
  GORIO_ERR_INVALID = -1,    /* bad argument (null pointer, n < k, ...) */
  GORIO_ERR_NO_DEVICE = -2,  /* no usable HIP device / HIP runtime error */
  GORIO_ERR_STATE = -3,      /* call order violated (align before setInputTarget, ...) */
  GORIO_ERR_ALLOC = -4,
  GORIO_ERR_UNSUPPORTED = -5 /* e.g. k_correspondences > 32, unknown regularisation (APD:389-391 aborts there) */
} gorio_status;

/* fast_gicp::RegularizationMethod, gicp_settings.hpp:6 (same order) */
typedef enum { GORIO_REG_NONE = 0, GORIO_REG_MIN_EIG = 1, GORIO_REG_NORMALIZED_MIN_EIG = 2, GORIO_REG_PLANE = 3, GORIO_REG_FROBENIUS = 4 } gorio_regularization;
/* fast_gicp::LSQ_OPTIMIZER_TYPE, lsq_registration.hpp:13 (same order) */
typedef enum { GORIO_OPT_GAUSS_NEWTON = 0, GORIO_OPT_LEVENBERG_MARQUARDT = 1 } gorio_optimizer;
/* correspondence search strategy; every mode returns the SAME indices (exact search, ties -> lowest index) */
typedef enum { GORIO_SEARCH_BRUTE_FORCE = 0, GORIO_SEARCH_PRUNED = 1 } gorio_search;

/* which fast_gicp registration a handle stands for: the three classes select_registration_method hands out through one pcl::Registration
 * pointer (REG:28-37 FAST_APDGICP, REG:63-67 FAST_GICP, REG:68-71 FAST_VGICP) */
typedef enum { GORIO_METHOD_APDGICP = 0, GORIO_METHOD_GICP = 1, GORIO_METHOD_VGICP = 2, GORIO_METHOD_GICP_OMP = 3 /* pclomp GICP, REG:91-100; below */ } gorio_method;
/* the methods that stand for classes of PCL itself, values of the same `method` argument of gorio_apd_set_method (gorio_method keeps the
 * GICP family: classes of the reference tree) */
typedef enum { GORIO_METHOD_ICP = 4 /* pcl::IterativeClosestPoint, REG:72-79; below */ } gorio_method_pcl;
/* a third enumeration feeding the same `method` argument: the algorithm of fast_gicp's CUDA back end (fast_gicp::NDTCuda; below) */
typedef enum { GORIO_METHOD_NDT_CUDA = 5 } gorio_method_fast_ndt;
/* fast_gicp::NDTDistanceMode in the order of ndt/ndt_settings.hpp:6 */
typedef enum { GORIO_NDT_CUDA_P2D = 0, GORIO_NDT_CUDA_D2D = 1 } gorio_ndt_cuda_distance;
/* a fourth enumeration feeding the same `method` argument: the other class of that back end (fast_gicp::FastVGICPCuda; below) */
typedef enum { GORIO_METHOD_VGICP_CUDA = 6 } gorio_method_fast_vgicp_cuda;
/* fast_gicp::NearestNeighborMethod in the order of gicp/fast_vgicp_cuda.hpp:21 */
typedef enum { GORIO_VGICP_CUDA_NN_CPU_PARALLEL_KDTREE = 0, GORIO_VGICP_CUDA_NN_GPU_BRUTEFORCE = 1, GORIO_VGICP_CUDA_NN_GPU_RBF_KERNEL = 2 } gorio_vgicp_cuda_nn;
/* a fifth enumeration feeding the same `method` argument: fast_gicp::FastGICPMultiPoints (below).  The value 7 stays unused and refused. */
typedef enum { GORIO_METHOD_GICP_MP = 8 } gorio_method_fast_gicp_mp;
/* fast_gicp::NeighborSearchMethod, gicp_settings.hpp:8 (same order) */
typedef enum { GORIO_VOXEL_DIRECT27 = 0, GORIO_VOXEL_DIRECT7 = 1, GORIO_VOXEL_DIRECT1 = 2, GORIO_VOXEL_DIRECT_RADIUS = 3 } gorio_voxel_search;
/* fast_gicp::VoxelAccumulationMode, gicp_settings.hpp:10 (same order) */
typedef enum { GORIO_VOXEL_ADDITIVE = 0, GORIO_VOXEL_ADDITIVE_WEIGHTED = 1, GORIO_VOXEL_MULTIPLICATIVE = 2 } gorio_voxel_mode;

typedef struct {
  int k_correspondences;         /* setCorrespondenceRandomness, APD:45; default 20 (APD:21); <= 32 */
  int regularization;            /* setRegularizationMethod, APD:50; default PLANE (APD:25) */
  double dist_var;               /* setDistVar APD:63; default 0.86 (APDH:118) */
  double azimuth_var;            /* setAzimuthVar APD:55; default 0.5 deg (APDH:116) */
  double elevation_var;          /* setElevationVar APD:59; default 1.0 deg (APDH:117) */
  double corr_dist_threshold;    /* pcl setMaxCorrespondenceDistance (REG:44); default FLT_MAX (APD:23) */
  int max_iterations;            /* pcl setMaximumIterations (REG:43); default 64 (LSQ:13) */
  double rotation_epsilon;       /* setRotationEpsilon LSQ:30; default 2e-3 (LSQ:14) */
  double transformation_epsilon; /* pcl setTransformationEpsilon (REG:42); default 5e-4 (LSQ:15) */
  int optimizer;                 /* lsq_optimizer_type_, default LM (LSQ:17) */
  int lm_max_iterations;         /* default 10 (LSQ:19) */
  double lm_init_lambda_factor;  /* setInitialLambdaFactor LSQ:35; default 1e-9 (LSQ:20) */
  int search;                    /* gorio_search; default brute force */
  int cl_weight_points;          /* N in cl_weight = 1/N (APD:273: correspondences_.size()); 0 = this handle's source size.  Set it to
                                    the global source size when the source cloud is sharded over several handles / GPUs */
  int keep_knn_indices;          /* parity hook: keep the k neighbour indices of every point for gorio_apd_get_knn_indices (80 B per point
                                    of extra stores in the covariance kernel); default 0 */
} gorio_apd_params;

typedef struct gorio_apd gorio_apd_t;

/* FastAPDGICP::FastAPDGICP() APD:14-28 / ~FastAPDGICP APD:31.  device = HIP device ordinal. */
int gorio_apd_create(gorio_apd_t** out, int device);
void gorio_apd_destroy(gorio_apd_t* h);
const char* gorio_apd_last_error(const gorio_apd_t* h);

/* library defaults == constructor defaults of the reference (APD:14-28, LSQ:10-24, APDH:116-118) */
void gorio_apd_default_params(gorio_apd_params* p);
/* all setters of APD:34-65, LSQ:30-42 and the pcl::Registration setters used at REG:42-44, in one call */
int gorio_apd_set_params(gorio_apd_t* h, const gorio_apd_params* p);
int gorio_apd_get_params(const gorio_apd_t* h, gorio_apd_params* p);

/*
 * Method selection.  GICPH / VGH = fast_gicp/gicp/fast_gicp.hpp / fast_vgicp.hpp, GICP / VG = their impl/ files, VOX = fast_vgicp_voxel.hpp.
 * A fresh handle is GORIO_METHOD_APDGICP and a caller that never calls the setter sees no change.
 *   GORIO_METHOD_GICP   FastGICP (GICP:126-257): FastAPDGICP without the sensor covariance in RCR (GICP:159) and without the (1 + geo + cl)
 *                       error weight (GICP:199, 253); dist_var / azimuth_var / elevation_var / cl_weight_points are not read.  Every entry
 *                       point of this header works as in APD-GICP mode, the sharded-source collective included.
 *   GORIO_METHOD_VGICP  FastVGICP (VG:66-204): the target becomes a Gaussian voxel map (GaussianVoxelMap, VOX:124-182; built on the device
 *                       from the target's covariances at the first linearise / align, reused while target, covariances, voxel_resolution and
 *                       voxel_mode stay as they are -- the reference rebuilds an equal map at every computeTransformation, VG:66-70), every
 *                       source point is paired with the occupied voxels among the 1 / 7 / 27 neighbours of voxel_coord(T * point)
 *                       (VG:83-94) and every pair enters H, b and the error with weight sqrt(num_points) (VG:149).  corr_dist_threshold is
 *                       not read (the reference has no gate there).  gorio_apd_get_correspondences / _get_mahalanobis (per-point
 *                       semantics) and the sharded-source calls return GORIO_ERR_STATE in this mode; fitness scores, transform_source,
 *                       align_batch and shared targets (sharers share the voxel map; a sharer whose voxel_resolution / voxel_mode differ
 *                       from the ones the shared map was built with gets GORIO_ERR_INVALID, like a differing k_correspondences) keep working.
 * voxel_resolution = setResolution VG:31, voxel_search = setNeighborSearchMethod VG:36 (gorio_voxel_search), voxel_mode =
 * setVoxelAccumulationMode VG:41 (gorio_voxel_mode); stored in every mode, read in VGICP mode (constructor defaults 1.0, DIRECT1, ADDITIVE,
 * VG:22-24).  GORIO_ERR_UNSUPPORTED for DIRECT_RADIUS (neighbor_offsets aborts there, VOX:13-15), voxel_resolution <= 0 and unknown values.
 * Target coordinates whose voxel grid does not fit the 33-bit voxel id of the map (bounding box of the occupied voxels >= 2^33 cells, or a
 * non-finite point) make the VGICP linearise / align return GORIO_ERR_UNSUPPORTED.  All handles of a gorio_apd_align_batch must carry the
 * same method and voxel settings (GORIO_ERR_INVALID otherwise).  Changing the method drops the correspondences held.
 */
int gorio_apd_set_method(gorio_apd_t* h, int method, double voxel_resolution, int voxel_search, int voxel_mode);
int gorio_apd_get_method(const gorio_apd_t* h, int* method, double* voxel_resolution, int* voxel_search, int* voxel_mode);
/*
 * GORIO_METHOD_GICP_OMP: pclomp::GeneralizedIterativeClosestPoint (REG:91-100; GOH = ndt_omp/include/pclomp/gicp_omp.h, GO = its
 * gicp_omp_impl.hpp).  gorio_apd_set_method(h, GORIO_METHOD_GICP_OMP, ...) ignores the voxel arguments.  In this mode
 *   - covariances are estimated by GO:50-122 from the handle's k-NN lists (float products summed in double, cov / k - mean mean^T, SVD
 *     rebuild with singular values 1, 1, gicp_epsilon); a cloud with fewer points than k_correspondences is refused (GORIO_ERR_INVALID; the
 *     reference prints an error and goes on without covariances).  The rule counts as one more regularization for shared clouds: sharing
 *     with a handle that estimates by another rule, k or gicp_epsilon gives GORIO_ERR_INVALID;
 *   - gorio_apd_align runs computeTransformation GO:375-520: the exact 1-NN of transformation_ * (guess * p) per outer iteration, float
 *     Mahalanobis matrices, the BFGS inner solve (GO:193-246) on the host with one device evaluation of the functor (GO:249-371) per round
 *     trip.  H_out is zero-filled; n_linearize = functor evaluations.  max_iterations, transformation_epsilon, rotation_epsilon,
 *     corr_dist_threshold, k_correspondences and search of gorio_apd_params are read, nothing else of it.  Fewer than 4 pairs, or a solver
 *     status other than Success / NoProgress before the inner cap, ends the align unconverged with previous_transformation_ * guess;
 *   - gorio_apd_linearize, gorio_apd_compute_error and gorio_apd_align_batch return GORIO_ERR_UNSUPPORTED (align_batch changes nothing;
 *     gorio_apd_gicp_omp_align_batch below is the batched form);
 *     the sharded-source calls return GORIO_ERR_STATE; everything else of this header works as in the other modes.
 * gicp_epsilon = gicp_epsilon_ (default 0.001, GOH:118), max_optimizer_iterations = setMaximumOptimizerIterations (default 20, GOH:121;
 * REG:99).  GORIO_ERR_INVALID for gicp_epsilon <= 0 and max_optimizer_iterations < 1.  Stored in every mode.
 */
int gorio_apd_set_gicp_omp_params(gorio_apd_t* h, double gicp_epsilon, int max_optimizer_iterations);
int gorio_apd_get_gicp_omp_params(const gorio_apd_t* h, double* gicp_epsilon, int* max_optimizer_iterations);
/* parity hooks (GICP_OMP mode).  _update: one pass of GO:411-476 with transformation_ = transformation16 and the given guess (both
 * row-major float 4x4): m receives the number of pairs; gorio_apd_get_correspondences then gives the target index per source point (-1:
 * none) and the float distances, gorio_apd_get_mahalanobis the stored float matrices widened to double (zero for unpaired points).
 * _evaluate: the functor at x = (tx, ty, tz, roll, pitch, yaw) over those pairs -- mode 0: operator() (f), 1: df (g6), 2: fdf (both).
 * _diag: outer iterations, minimizeOneStep calls and functor evaluations of the last align, and its last solver status (-1 running,
 * 0 success, 1 no progress, 2 failed). */
int gorio_apd_gicp_omp_update(gorio_apd_t* h, const float transformation16[16], const float guess16[16], int* m);
int gorio_apd_gicp_omp_evaluate(gorio_apd_t* h, const double x6[6], int mode, double* f, double* g6);
int gorio_apd_gicp_omp_diag(const gorio_apd_t* h, int* outer, int* inner_total, int* evaluations, int* last_status);
/*
 * Batched GICP_OMP aligns: the aligns of `count` handles in lock-step rounds.  Every handle runs the machine its own gorio_apd_align runs
 * (one pass of GO:411-476, then the BFGS inner solve, suspended at every functor evaluation); in every round each unfinished handle has
 * exactly one request pending, an update or an evaluation.  Per round: one search launch and one update launch when any update is pending,
 * one functor launch when any evaluation is pending, one launch that adds every request's block sums in block order, one copy back, one
 * synchronisation -- on the stream and with the tables of handles[0].  guesses / T_out: count x 16 row-major floats; converged,
 * nr_iterations, n_evaluations: count ints each, any may be NULL.
 *   - gorio_apd_align_batch is unchanged: it keeps returning GORIO_ERR_UNSUPPORTED for these handles.  The batched BFGS has an entry
 *     point of its own because its shell is not the Gauss-Newton / LM one.
 *   - count == 0 returns GORIO_OK.  count < 0, a null array or a null entry: GORIO_ERR_INVALID.  The same handle twice, handles on two
 *     devices, a handle with a communicator, gorio_apd_params that differ between handles (cl_weight_points excepted, as for
 *     gorio_apd_align_batch): GORIO_ERR_INVALID.  A handle whose method is not GORIO_METHOD_GICP_OMP: GORIO_ERR_STATE.  A handle that is
 *     not ready (no source or target, a cloud smaller than k_correspondences, a shared cloud estimated by another rule / k / epsilon):
 *     that handle's own code.  All of it is checked before anything is built or launched; the message on handles[0] names the offending
 *     index ("handle <q>: ..."), and no handle is changed.
 *   - gicp_epsilon and max_optimizer_iterations are per handle and may differ within a batch.
 *   - targets and sources may be shared between the handles (gorio_apd_set_target_shared, keyframe and scan hand-offs): a shared cloud's
 *     index and covariances are made once per batch.
 *   - an align that ends early is not a failed call: "fewer than 4 correspondences" and "BFGS solver didn't converge" end that handle alone
 *     with converged[q] = 0 and its own error string, as gorio_apd_align does; the call still returns GORIO_OK.
 *   - after the call every handle holds what its own gorio_apd_align would have left: correspondences, squared distances, Mahalanobis
 *     matrices, the pairs, and the four gorio_apd_gicp_omp_diag values; the parity hooks work on that state.
 *   - T_out, converged, nr_iterations and n_evaluations are bit for bit those of gorio_apd_align on the same handle, in both search modes:
 *     the per-workgroup bodies of the kernels and the order of every sum are the single align's.
 * gorio_apd_gicp_omp_batch_diag, of the last batch led by `lead` (its handles[0]): rounds = lock-step rounds (the longest member's updates
 * plus evaluations), launches = kernel launches of the batch (one `output` launch per handle, then at most four per round).
 */
int gorio_apd_gicp_omp_align_batch(gorio_apd_t** handles, int count, const float* guesses /* count x 16 */, float* T_out /* count x 16 */,
                                   int* converged, int* nr_iterations, int* n_evaluations /* each count, may be NULL */);
int gorio_apd_gicp_omp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches);

/*
 * GORIO_METHOD_ICP: pcl::IterativeClosestPoint (REG:72-79).  gorio_apd_set_method(h, GORIO_METHOD_ICP, ...) ignores the voxel arguments.
 * The algorithm below is PCL 1.10's IterativeClosestPoint::computeTransformation with CorrespondenceEstimation, TransformationEstimationSVD
 * and DefaultConvergenceCriteria, RECALLED from the published sources (they are not part of the reference tree) and FIXED HERE: this text
 * is the specification, tests/icp_restatement.py restates it.
 *   start   final = guess; the working copy W = guess * source in float by the ((m0 x + m1 y) + m2 z) + m3 rule; transformation = I,
 *           nr_iterations = 0, prev_mse = DBL_MAX, similar = 0.  translation_thr = transformation_epsilon, rotation_thr =
 *           transformation_rotation_epsilon > 0 ? that : 1 - transformation_epsilon, rel_mse_thr = euclidean_fitness_epsilon,
 *           abs_mse_thr = 1e-12, max_similar = 0.
 *   loop    1. the exact 1-NN of every point of W in the target (float L2_Simple, ties to the lowest index);
 *           2. the pair is kept unless (double)sqd > corr_dist_threshold^2;
 *           3. with use_reciprocal, only if the exact 1-NN of the matched target point among the points of W (ties to the lowest index) is
 *              that source point (a brute-force pass over W);
 *           4. fewer than 3 pairs: state 5, converged = false, stop;
 *           5. transformation = the rigid transform of the pairs: with n pairs (q in W, t in the target), means q_m, t_m and
 *              Sigma = sum(t q^T) / n - t_m q_m^T in double, Sigma = U D V^T by fp64 Jacobi, R = U diag(1, 1, det(U) det(V)) V^T (Umeyama's
 *              rule without scale: sign(det Sigma) at full rank, the rank-2 rule otherwise), t = t_m - R q_m, rounded ONCE to float.  PCL
 *              evaluates this in float with Eigen's summation order; the double evaluation rounded once is this library's definition;
 *           6. W <- transformation * W in float: the copy is moved incrementally and accumulates rounding, as PCL's does;
 *           7. final = transformation * final, a float 4x4 product summed left to right;   8. ++nr_iterations;
 *           9. (a) nr_iterations >= max_iterations: state 1, converged.  (b) cos = 0.5 (trace R - 1), t2 = |t|^2 of transformation in double
 *              from its float entries; cos >= rotation_thr && t2 <= translation_thr: state 2, converged when similar >= max_similar, else
 *              the step is marked similar.  (c) mse = mean of the pairs' float squared distances summed in double;
 *              |mse - prev_mse| < abs_mse_thr: the same rule with state 3; |mse - prev_mse| / prev_mse < rel_mse_thr: with state 4.
 *              (d) similar is incremented when the step was marked and reset otherwise; prev_mse = mse; continue.
 *   end     T_out = final, converged and nr_iterations as the loop left them.
 * In this mode
 *   - gorio_apd_align runs the loop; H_out is zero-filled, n_linearize = correspondence passes.  Of gorio_apd_params only max_iterations,
 *     transformation_epsilon, corr_dist_threshold and search are read.  No k-NN lists and no covariances are computed: a cloud with fewer
 *     points than k_correspondences is accepted.  In pruned mode the target index is built, and the source index to order the query waves;
 *   - gorio_apd_linearize, gorio_apd_compute_error and gorio_apd_align_batch return GORIO_ERR_UNSUPPORTED and change nothing;
 *     gorio_apd_get_mahalanobis, the sharded-source calls (gorio_apd_comm_init, gorio_apd_debug_set_shard with more than one rank) and the
 *     gorio_apd_gicp_omp_* entry points that compute return GORIO_ERR_STATE; the gorio_apd_icp_* calls return GORIO_ERR_STATE on a handle of
 *     another method;
 *   - setters, hand-offs (host, device, scan, keyframe, submap, shared target), gorio_apd_transform_source and the fitness scores work as
 *     in the other modes; gorio_apd_get_correspondences gives the pairs of the last pass: the target index and the float squared distance
 *     of a pair, -1 and +infinity for a point without one (no neighbour inside the gate, or not reciprocal).
 * use_reciprocal = setUseReciprocalCorrespondences (0 / 1, default 0), euclidean_fitness_epsilon = setEuclideanFitnessEpsilon (default
 * -DBL_MAX), transformation_rotation_epsilon = setTransformationRotationEpsilon (default 0).  GORIO_ERR_INVALID for another
 * use_reciprocal and for NaN.  Stored in every mode, read in ICP mode.
 */
int gorio_apd_set_icp_params(gorio_apd_t* h, int use_reciprocal, double euclidean_fitness_epsilon, double transformation_rotation_epsilon);
int gorio_apd_get_icp_params(const gorio_apd_t* h, int* use_reciprocal, double* euclidean_fitness_epsilon, double* transformation_rotation_epsilon);
/* Of the last align (any output may be NULL): nr_iterations, pcl::registration::DefaultConvergenceCriteria::ConvergenceState (0 not
 * converged, 1 iterations, 2 transform, 3 abs MSE, 4 rel MSE, 5 no correspondences, 6 failure after max iterations -- never produced),
 * the mean squared pair distance and the pair count of the last pass (-1: none held). */
int gorio_apd_icp_diag(const gorio_apd_t* h, int* iterations, int* state, double* mse, int* pairs);
/* Parity hook: ONE correspondence pass on the copy T16 * source (row-major float 4x4).  pairs = the pair count; sums17 = count, sum d^2,
 * sum q (3), sum t (3), sum t q^T (9, row-major: t along the rows) over the pairs, block partials of 256 source points added in block
 * order; T_est16 = the rigid transform of step 5 (the identity when fewer than 3 pairs).  Any output may be NULL.
 * gorio_apd_get_correspondences then gives the pairs. */
int gorio_apd_icp_step(gorio_apd_t* h, const float T16[16], int* pairs, double sums17[17], float T_est16[16]);
/*
 * Batched ICP aligns in lock-step rounds: every round each unfinished handle has one correspondence pass pending.  Per round: one search
 * launch, one launch that commits the moved copies, gates and reduces the pairs, one launch that adds every handle's block sums in block
 * order (three launches; a round with a reciprocal handle pending adds one), one copy back, one synchronisation -- on the stream and with
 * the tables of handles[0].  rounds = the largest nr_iterations of the batch (a handle that ends with fewer than 3 pairs counts that pass).
 *   - validation is that of gorio_apd_gicp_omp_align_batch: count == 0 is GORIO_OK; count < 0, a null array or entry, the same handle
 *     twice, handles on two devices, differing gorio_apd_params: GORIO_ERR_INVALID; a handle of another method, or without its clouds:
 *     GORIO_ERR_STATE.  Checked before anything is built or launched; the message on handles[0] names the index ("handle <q>: ...").
 *   - the ICP parameters are per handle and may differ; targets and sources may be shared.
 *   - "fewer than 3 correspondences" ends that handle alone with converged[q] = 0; the call still returns GORIO_OK.
 *   - every output of handle q, its correspondences and its gorio_apd_icp_diag values are bit for bit those of its own gorio_apd_align:
 *     the single align runs the same rounds with count = 1.
 * gorio_apd_icp_batch_diag, of the last batch led by `lead`: lock-step rounds and kernel launches.
 */
int gorio_apd_icp_align_batch(gorio_apd_t** handles, int count, const float* guesses /* count x 16 */, float* T_out /* count x 16 */,
                              int* converged, int* nr_iterations /* each count, may be NULL */);
int gorio_apd_icp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches);

/*
 * GORIO_METHOD_NDT_CUDA: fast_gicp::NDTCuda, the point-to-distribution (P2D) and distribution-to-distribution (D2D) NDT of the reference's
 * CUDA back end under the LsqRegistration shell of the GICP family.  Reference lines: NC = src/fast_gicp/cuda/ndt_cuda.cu, ND =
 * src/fast_gicp/cuda/ndt_compute_derivatives.cu, GV = src/fast_gicp/cuda/gaussian_voxelmap.cu, FV = src/fast_gicp/cuda/
 * find_voxel_correspondences.cu, CR = src/fast_gicp/cuda/covariance_regularization.cu, NH / NI = include/fast_gicp/ndt/ndt_cuda.hpp and
 * its impl, NS = ndt/ndt_settings.hpp.  The reference sums with float atomics and a tree reduction (its results are not reproducible) and
 * its hash table may drop voxels; THIS TEXT is the definition, tests/ndt_cuda_restatement.py restates it.
 *   map      (replaces GaussianVoxelMap::create_voxelmap, GV:205-227, and covariance_regularization, NC:128 / 139)  res = (float)resolution;
 *            per axis coord = (int)floorf(x / res - 0.5f) IN FLOAT (GV:118-121; not the double rule of the FastVGICP map).  Per occupied
 *            voxel, in input order, in float: n, s += p, S += p p^T (each product rounded, then added).  mean = s / (float)n, cov_raw =
 *            (S - mean s^T) / (float)n (GV:185-188; 9 floats, mean s^T is not symmetric in float).  cov = sum_i max(1e-3, lambda_i) v_i v_i^T
 *            with (lambda, v) from this library's fp64 cyclic Jacobi on the UPPER triangle of cov_raw widened to double, summed in double,
 *            rounded to float once (the reference: Eigen's float closed form and V diag V^-1, CR:73-87 -- a library detail replaced here).
 *            Voxels of any size are regularised.  Voxels are numbered in ascending packed id, i.e. lexicographic (x, y, z) coordinate order
 *            (the reference's numbering is its insertion race); no voxel is ever dropped (GV:254-285 tolerates 1 % unassigned points).
 *   offsets  (replaces set_neighbor_search_method, NC:35-88) in table order: DIRECT1 (0,0,0); DIRECT7 the centre, +x, -x, +y, -y, +z, -z;
 *            DIRECT27 i, j, k nested, k fastest, each -1..1; DIRECT_RADIUS every integer offset with norm <= radius + 1e-3 from the same
 *            triple loop over -ceil(radius)..ceil(radius).  0 < radius <= 3; larger: GORIO_ERR_UNSUPPORTED; <= 0 or not finite:
 *            GORIO_ERR_INVALID (the reference would build an empty table).
 *   pairs    (replaces update_correspondences, NC:142-160, FV:32-60, 83-111)  items: P2D the source points, D2D the means of the source
 *            cloud's own map in voxel order.  At linearize(x): Tf = (float)x, q = R p + t per row, left to right, un-fused, in float; for
 *            every offset in table order and every item there is a pair when voxel coord(q) + offset exists.  The list is offset-major,
 *            then item order; x is remembered as x_lin.
 *   terms    (replaces the functors of ND:50-91 and ND:120-163) per pair, all in float; a pair is skipped when the TARGET voxel has
 *            num_points <= 6.  a' = R a + t at the evaluation pose; e = mean_B - a'; Q = cov_B (P2D) or cov_B + (R_lin cov_A) R_lin^T (D2D);
 *            C = adj(Q) / det(Q), adj by the nine 2x2 cofactors (minuend first: c00 = q11 q22 - q12 q21, c01 = q02 q21 - q01 q22, c02 = q01 q12
 *            - q02 q11, c10 = q12 q20 - q10 q22, c11 = q00 q22 - q02 q20, c12 = q02 q10 - q00 q12, c20 = q10 q21 - q11 q20, c21 = q01 q20 - q00
 *            q21, c22 = q00 q11 - q01 q10), det = (q00 c00 + q01 c10) + q02 c20; w = k^2 / (k^2 + n n), k = res, n = sqrtf((e0 e0 + e1 e1) + e2
 *            e2) (the Cauchy kernel, ND:15-18); J = [skew(a') | -I]; A = w J^T, B = A C, H = B J, b = B e, err = ((w e)^T C) e; every
 *            3-term sum left to right.  The upper triangle of H is taken.
 *   sums     the float terms are widened and added in fp64: wave, then block, then blocks in block order.  No floating-point atomics: two
 *            runs give the same bits.
 *   shell    LsqRegistration unchanged (LSQ:55-173): linearize = pairs + terms + sums; compute_error(x) = terms + sums over the STALE pairs
 *            with R_lin (NC:162-177).  corr_dist_threshold is not read.
 *   maps     built lazily at the first linearise / align (NI:76-79) and reused while the cloud and the resolution stay the same; P2D builds
 *            no source map; gorio_apd_swap_source_and_target swaps clouds and maps (NC:90-93).  DEVIATION: a changed resolution rebuilds the
 *            maps (the reference keeps the old ones, NC:120-140).
 * gorio_apd_set_method(h, GORIO_METHOD_NDT_CUDA, voxel_resolution, voxel_search, voxel_mode): voxel_resolution = setResolution,
 * voxel_search = setNeighborSearchMethod (DIRECT_RADIUS is accepted in this method only and uses the radius stored by
 * gorio_apd_set_ndt_cuda_params, checked as above); voxel_mode is ignored; voxel_resolution <= 0: GORIO_ERR_UNSUPPORTED.  In this mode
 *   - gorio_apd_linearize, gorio_apd_compute_error, gorio_apd_align, gorio_apd_align_batch (all handles must agree in method, resolution,
 *     offsets and distance mode: GORIO_ERR_INVALID otherwise; results bit for bit the single aligns'), the fitness scores,
 *     gorio_apd_transform_source, shared targets (the sharers share the map; a sharer with another resolution gets GORIO_ERR_INVALID) and
 *     the scan / keyframe / submap hand-offs work;
 *   - gorio_apd_get_correspondences, gorio_apd_get_mahalanobis, the covariance getters, setters and gorio_apd_calculate_covariances, and the
 *     sharded-source calls return GORIO_ERR_STATE;
 *   - no k-NN, covariance estimate or search index is made for an align.
 * gorio_apd_set_ndt_cuda_params: distance_mode = setDistanceMode (NS:6: P2D = 0, D2D = 1; default D2D, NC:21), radius = the second argument
 * of setNeighborSearchMethod (default -1, NH:55).  Stored in every mode; another distance_mode or a NaN radius: GORIO_ERR_INVALID; while the
 * handle is in this method with DIRECT_RADIUS the radius is checked as above.
 * Parity hooks: gorio_apd_ndt_cuda_get_voxels gives the map of the source (which = 0) or target (1), building it when stale -- except the
 * source's in P2D mode, where the map held (or 0 voxels) is reported: coords 3 ints, num_points, mean 3 floats, cov_raw and cov 9 floats
 * row-major per voxel.  n_voxels always receives the count; the arrays (any may be NULL) are filled when capacity >= it.
 * gorio_apd_ndt_cuda_get_pairs gives the pair list of the last linearise (item index, target voxel index), GORIO_ERR_STATE when none is held.
 */
int gorio_apd_set_ndt_cuda_params(gorio_apd_t* h, int distance_mode, double radius);
int gorio_apd_get_ndt_cuda_params(const gorio_apd_t* h, int* distance_mode, double* radius);
int gorio_apd_ndt_cuda_get_voxels(gorio_apd_t* h, int which, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov_raw, float* cov);
int gorio_apd_ndt_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel);

/*
 * GORIO_METHOD_VGICP_CUDA: fast_gicp::FastVGICPCuda, the voxelised GICP of the reference's CUDA back end (FAST_VGICP_CUDA of
 * select_registration_method, REG:52-61) under the LsqRegistration shell.  Reference lines (paths relative to the reference's
 * fast_apdgicp/): VH / VI = include/fast_gicp/gicp/fast_vgicp_cuda.hpp and impl/fast_vgicp_cuda_impl.hpp, VC = src/fast_gicp/cuda/
 * fast_vgicp_cuda.cu, CE = covariance_estimation.cu, RB = covariance_estimation_rbf.cu, CR = covariance_regularization.cu, GV =
 * gaussian_voxelmap.cu, FV = find_voxel_correspondences.cu, CD = compute_derivatives.cu (all in src/fast_gicp/cuda/).  As with NDTCuda the
 * reference is not reproducible (float atomics in the voxel sums, a thrust tree over the derivatives, an insertion race for the voxel
 * numbering, an unspecified heap order in the brute-force k-NN); THIS TEXT is the definition, tests/vgicp_cuda_restatement.py restates it.
 * Every float expression is un-fused and evaluated in the one order written here.
 *   neighbours  (VH:21; default CPU_PARALLEL_KDTREE, VI:27)  CPU_PARALLEL_KDTREE (0) and GPU_BRUTEFORCE (1) are ONE path: the exact k-NN list of
 *            every point in its own cloud, k = params.k_correspondences, in ascending (float squared distance ((dx dx + dy dy) + dz dz),
 *            index) order, the point itself included.  GPU_RBF_KERNEL (2) uses no list and builds no search index.
 *   k-NN covariance  (CE:26-34) in float, in list order: mean += p, S_ab += p_a p_b for a <= b; then mean /= (float)k and cov_ab = S_ab /
 *            (float)k - mean_a mean_b.  Six floats per point (00 01 02 11 12 22).
 *   RBF covariance  (RB:67-85, 98-108, 116-151)  g = (float)kernel_width is the exponent factor itself, not its reciprocal (RB:120, 80); m2
 *            = (float)max_dist squared, max_dist = kernel_max_dist, or 5 kernel_width when that is <= 0 (VI:46-50).  The cloud is extended
 *            to a multiple of 512 points with points at the origin, which take part like any other (RB:127-129).  Per point x and per
 *            block of 512 consecutive points, in index order, from zero: d2 = (dx dx + dy dy) + dz dz with d = x - p; skipped when d2 > m2;
 *            w = expf(-g d2); sw += w; s_a += w p_a; S_ab += (w p_a) p_b for a <= b.  The block partials are added in block order to a
 *            total that starts at zero.  mean = s / sw; cov_ab = (S_ab - mean_a s_b) / sw.  DEVIATION: the reference keeps nine sums, this
 *            library the upper triangle.  QUIRK (replicated): a cloud whose size is no multiple of 512 gives every point within max_dist of
 *            the origin up to 511 phantom neighbours at the origin.
 *   regularisation  (CR:91-117; params.regularization) on the six floats widened to double, eigenvalues w0 <= w1 <= w2 with vectors v0, v1, v2
 *            from this library's fp64 cyclic Jacobi; every rebuilt matrix is summed in double and rounded to float once.  PLANE: a point
 *            is KEPT when w1 > w2 * 0.1 (CR:29) and dropped otherwise, cov = 1e-3 v0 v0^T + v1 v1^T + v2 v2^T.  MIN_EIG: sum_i max(1e-3, w_i)
 *            v_i v_i^T.  FROBENIUS: C = cov + 1e-3 I, result ||C^-1||_F C.  NONE and NORMALIZED_MIN_EIG leave the raw covariance (the
 *            reference prints "unimplemented" and does the same, CR:114-116).  Only PLANE drops points.  The kept points keep their input
 *            order; source and target are both filtered and the dropped points take no further part.
 *   map      (GV:229-252, VC:257-263) of the kept TARGET points and their regularised covariances: coordinates by the float rule of the
 *            NDTCuda map, voxels in ascending packed id; per voxel, in the kept points' order, in float: n, s += p, Csum += cov; mean = s /
 *            (float)n, cov = Csum / (float)n.  No voxel is dropped.  There is no source map.  No kept point: an empty map.
 *   pairs    (VC:265-274, FV) the NDTCuda rule with items = the kept source points: offset-major, float transform, x remembered as x_lin.
 *   terms    (CD:50-92, 106-135) per pair, all in float: a' = R a + t at the evaluation pose; e = mean_B - a'; Q = cov_B + (R_lin cov_A)
 *            R_lin^T; C = adj(Q) / det(Q) as written out for NDTCuda above; w = sqrtf((float)num_points) -- no Cauchy kernel and no
 *            num_points > 6 gate; J = [skew(a') | -I]; A = w J^T, B = A C, H = B J, b = B e, err = ((w e)^T C) e.
 *   sums     the float terms are widened and added in fp64: wave, then block, then blocks in block order.  Two runs give the same bits.
 *   shell    LsqRegistration unchanged; compute_error runs over the STALE slots with R_lin; corr_dist_threshold is not read.
 *   lifecycle  covariances, kept points and map are made lazily at the first linearise / align and reused while the cloud, k, the neighbour
 *            method, the kernel parameters, the regularisation and the resolution stay the same; a change rebuilds what depends on it.
 *            gorio_apd_swap_source_and_target swaps clouds with their covariances and kept points and builds the new target's map
 *            (VC:97-107).  DEVIATION, as for NDTCuda: a changed resolution rebuilds the map (in the reference setResolution reaches only the
 *            first map ever built and computeTransformation resets the core to 1.0: VI:41-43, 145; VC:257-263).
 *            gorio_apd_transform_source and the fitness scores work on the whole uploaded cloud, filter or not, as PCL does with input_.
 * gorio_apd_set_method(h, GORIO_METHOD_VGICP_CUDA, voxel_resolution, voxel_search, voxel_mode): as for GORIO_METHOD_NDT_CUDA -- DIRECT_RADIUS is
 * accepted with the radius of gorio_apd_set_ndt_cuda_params and its checks, voxel_mode is ignored, voxel_resolution <= 0:
 * GORIO_ERR_UNSUPPORTED.  In this mode
 *   - gorio_apd_linearize, gorio_apd_compute_error, gorio_apd_align, gorio_apd_align_batch (all handles must agree in method, resolution,
 *     offsets, neighbour method, kernel parameters and regularisation: GORIO_ERR_INVALID otherwise; results bit for bit the single aligns'),
 *     the fitness scores, gorio_apd_transform_source, shared targets (the sharers share covariances, kept points and map; a sharer that
 *     disagrees in a setting that shapes a stage held gets GORIO_ERR_INVALID) and the scan / keyframe / submap hand-offs work (they deliver
 *     points: covariances stored with a keyframe are not used);
 *   - gorio_apd_get_correspondences, gorio_apd_get_mahalanobis, the double covariance getters and setters,
 *     gorio_apd_calculate_covariances and the sharded-source calls return GORIO_ERR_STATE;
 *   - in the k-NN modes a cloud with fewer than k points is refused with GORIO_ERR_INVALID, as the handle's covariance estimate refuses it;
 *   - when the filter keeps no source point linearize returns zero sums and an align behaves as the shell does on an empty pair list.
 * gorio_apd_set_vgicp_cuda_params: nn_method = setNearestNeighborSearchMethod, kernel_width / kernel_max_dist = setKernelWidth (defaults 0, 0.5,
 * 3.0: VI:27, 31).  Stored in every method; another nn_method, a non-finite value or kernel_width <= 0: GORIO_ERR_INVALID.
 * Parity hooks (this method only; they build what is stale; a count always arrives, the arrays -- any may be NULL -- are filled when
 * capacity >= the count): gorio_apd_vgicp_cuda_get_points gives for the source (which = 0) or target (1) n, cov_raw [n][6], n_kept,
 * kept_index [n_kept] and the regularised cov [n_kept][6] (capacity counts points: >= n fills all three); gorio_apd_vgicp_cuda_get_voxels
 * gives the target map: coords 3 ints, num_points, mean 3 floats, cov 6 floats per voxel; gorio_apd_vgicp_cuda_get_pairs gives the pair
 * list of the last linearise (kept-item index, voxel index), GORIO_ERR_STATE when none is held.
 */
int gorio_apd_set_vgicp_cuda_params(gorio_apd_t* h, int nn_method, double kernel_width, double kernel_max_dist);
int gorio_apd_get_vgicp_cuda_params(const gorio_apd_t* h, int* nn_method, double* kernel_width, double* kernel_max_dist);
int gorio_apd_vgicp_cuda_get_points(gorio_apd_t* h, int which, int capacity, int* n, float* cov_raw, int* n_kept, int* kept_index, float* cov);
int gorio_apd_vgicp_cuda_get_voxels(gorio_apd_t* h, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov);
int gorio_apd_vgicp_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel);

/*
 * GORIO_METHOD_GICP_MP: fast_gicp::FastGICPMultiPoints, the multi-point GICP of the reference's experimental directory.  Reference lines (paths
 * relative to the reference's fast_apdgicp/): MPH / MPI = include/fast_gicp/gicp/experimental/fast_gicp_mp.hpp and fast_gicp_mp_impl.hpp
 * (instantiated in src/fast_gicp/gicp/experimental/fast_gicp_mp.cpp).  Every source point is matched against a distribution MERGED from all target
 * points within neighbor_search_radius of its transformed position, distance-weighted and redone at every Gauss-Newton pass.  What MPI leaves
 * open -- fast_gicp/opt/gauss_newton.hpp and Sophus are not in the reference tree, FLANN's result order is not specified -- is fixed HERE: this text
 * is the definition, tests/gicp_mp_restatement.py restates it.  Every float expression is un-fused and evaluated in the one order written.
 *   covariances  (MPI:225-276; made lazily, reused while the cloud, k and the regularisation stay) per point of either cloud from its exact k-NN
 *            list in its own cloud, k = params.k_correspondences, in ascending (float squared distance, index) order, the point itself
 *            included.  In float, in list order: s += p; mean = s / (float)k; then with d = p - mean, cov_ab += d_a d_b for a <= b -- NOT divided
 *            by k (MPI:242).  FROBENIUS, in double: C = cov + 1e-3 I; X = C^-1 (cofactors times 1 / det, det expanded along the first row); f =
 *            sqrt of the sum of the nine squared entries of X, row by row; result = (X / f)^-1, rounded to float.  PLANE / MIN_EIG /
 *            NORMALIZED_MIN_EIG: the reference takes JacobiSVD<Matrix3f>; the matrix is symmetric positive semi-definite, so this library's
 *            fp64 symmetric 3 x 3 eigen-solver STANDS IN for it: eigenvalues w0 >= w1 >= w2 with vectors v0, v1, v2 of the six floats widened
 *            to double, s_i = |(float)w_i|, values (1, 1, 1e-3f) / max(s_i, 1e-3f) / max(s_i / max(s), 1e-3f), result = sum_i value_i v_i v_i^T
 *            summed in double in that order and rounded to float once.  NONE: GORIO_ERR_UNSUPPORTED (the reference aborts, MPI:255-257).  A
 *            cloud with fewer than k points: GORIO_ERR_INVALID (the reference reads uninitialised columns there).
 *   exp / log  Rodrigues and its inverse in double from float inputs, rounded to float wherever the reference holds a float (x0, delta,
 *            trans).  exp(w) = I + A K + B K^2, K = skew(w), K^2 = w w^T - t2 I, t2 = (w0 w0 + w1 w1) + w2 w2; t2 < 1e-12: A = 1 - t2 / 6, B = 1 / 2
 *            - t2 / 24; otherwise A = sin(t) / t, B = 2 sin^2(t / 2) / t2.  log(R): v = (R21 - R12, R02 - R20, R10 - R01) / 2, c = ((R00 + R11) + R22 -
 *            1) / 2, s = |v|, t = atan2(s, c), w = (t / s) v, or (1 + t^2 / 6) v when s < 1e-6.  Rotations near pi are outside its domain.
 *   loop     (MPI:80-115) x0 = [float(log(R_guess)), t_guess].  Pass i = 0 .. max_iterations - 1 sets iterations = i: trans = [float(exp(
 *            x0.head)) | x0.tail]; queries q = trans p by the float transform of the GICP family (((m0 x + m1 y) + m2 z) + m3); neighbours of
 *            q in the target by the rule and order of include/gorio_search.h: d < (float)(r r) strictly, ascending (d, original index); an
 *            empty neighbourhood stays empty.  Then the terms, H = sum J^T J, g = sum J^T r, delta = float(LDLT6(H) \ g) with this library's
 *            pivoted 6 x 6 LDLT in double, x0.head = float(log(exp(-delta.head) exp(x0.head))) (the product in double), x0.tail -= delta.tail
 *            (float), and the float test max(|float(exp(delta.head)) - I| (float)(1 / rotation_epsilon), |delta.tail| (float)(1 /
 *            transformation_epsilon)) < 1 ends the align converged.  The final transformation is trans of the last x0.
 *   term     (MPI:170-213) of source point i with neighbours j (skipped without one): w_j = max(1e-3, min(1, 1 - (double)sqrtf(d_j) / r)) in
 *            double (the square root is the float one of MPI:184); sw += w_j, sm += w_j b_j, sC += w_j C_j (six entries) in double in the
 *            neighbours' order; mean_B = float(sm / sw), cov_B = float(sC / sw).  In float: a' = q_i; d = mean_B - a'; M = R C_a (each entry (R_r0
 *            A_0c + R_r1 A_1c) + R_r2 A_2c); Q = cov_B + M R^T (likewise); C = adj(Q) / det(Q), the cofactor form of FastVGICPCuda above (RCR(3,
 *            3) = 1 decouples the fourth row); residual r = C d and Jacobian J = C [skew(a') | -I], each entry of C skew(a') the three-term sum
 *            left to right with its zeros, the last three columns -C.
 *   sums     per point the 21 + 6 entries (J_0a J_0b + J_1a J_1b) + J_2a J_2b and (J_0a r_0 + J_1a r_1) + J_2a r_2 in double from the widened
 *            floats; per block of 256 consecutive source points the halving tree of a wave (lanes l and l + 32, 16, 8, 4, 2, 1) and (w0 + w1) +
 *            (w2 + w3) over its four waves; the blocks added in block order.  No atomics: two runs give the same bits.
 *   DEVIATIONS  the reference's solver is not in its tree; as recalled it factors with LLT and substitutes a random step for a non-finite one.
 *            Here a non-finite delta, or a pass in which no source point has a neighbour, ENDS the align unconverged with the current x0.
 * gorio_apd_set_method(h, GORIO_METHOD_GICP_MP, ...): the voxel arguments are ignored, as for ICP.  Read from gorio_apd_params:
 * k_correspondences, regularization, max_iterations, rotation_epsilon, transformation_epsilon, search (of the k-NN lists); nothing else.  The
 * class's own defaults (MPI:20-36: k 20, 64 iterations, both epsilons 1e-5, PLANE) are the caller's to set.  In this mode
 *   - gorio_apd_align runs the loop: nr_iterations = the index of the last pass, n_linearize = the passes run, H_out = the last H;
 *   - gorio_apd_linearize, gorio_apd_compute_error, gorio_apd_get_correspondences, gorio_apd_get_mahalanobis and gorio_apd_align_batch return
 *     GORIO_ERR_UNSUPPORTED and change nothing (the batched form of this method is gorio_apd_gicp_mp_align_batch below); the other methods'
 *     batch calls refuse such a handle as they refuse any foreign one; the double
 *     covariance getters / setters, gorio_apd_calculate_covariances and the sharded-source calls return GORIO_ERR_STATE;
 *   - fitness and inlier scores, gorio_apd_transform_source, shared targets (the sharers share the float covariances: a sharer with another k
 *     or regularisation gets GORIO_ERR_INVALID) and the scan / keyframe hand-offs work; the target's search index is the one every method
 *     builds, its points are uploaded once.  A neighbour total above 2^31 - 1 returns the search's GORIO_ERR_UNSUPPORTED.
 * gorio_apd_set_gicp_mp_params: neighbor_search_radius (default 0.5, MPI:35; the reference has no setter).  Stored in every method; not finite
 * or <= 0: GORIO_ERR_INVALID.  Changing the method, the radius or either cloud drops the pass held.
 * Parity hooks (this method only; GORIO_ERR_STATE otherwise): gorio_apd_gicp_mp_get_covariances gives the float covariances of the source
 * (which = 0) or target (1), six floats per point (00 01 02 11 12 22), filled when capacity >= n.  gorio_apd_gicp_mp_pass runs ONE pass at the
 * float pose T16 (its 12 leading floats are trans) and returns the points used, the neighbour total, H (36) and g (6) (any may be NULL); it
 * leaves on the device the CSR and the merged distributions, which gorio_apd_gicp_mp_get_neighbors (offsets [n + 1], idx / sqd [total], filled
 * when capacity >= total) and gorio_apd_gicp_mp_get_merged (mean_B 3 floats, cov_B 6 floats, used flag per source point; capacity >= n) deliver.
 * An align leaves the CSR of its last pass but no merged distributions.  gorio_apd_gicp_mp_diag: passes of the last align, points used and
 * neighbour total of the last pass, and the seconds spent per stage (query transform, radius search, merge + linearise, shell) while
 * gorio_apd profiling was on.  gorio_apd_gicp_mp_last_hessian: the 36 doubles gorio_apd_align gave as H_out, held for the last align of the
 * handle, single or batched (zeros before any).
 *
 * gorio_apd_gicp_mp_align_batch: `count` aligns in lock step, handle q from guesses + 16 q to T_out + 16 q (converged / nr_iterations: count
 * entries each, may be NULL).  Every unfinished handle has one pass pending at its own pose; a ROUND is one query-transform launch over all of
 * them, ONE batched radius search (include/gorio_search.h: gorio_search_radius_batch's core, every handle against its own target with its own
 * radius), one merge-and-linearise launch, one fold launch and one copy back of 28 doubles per pending handle -- two synchronisations per
 * round whatever the count, on the stream of handles[0].  The kernels run the single align's per-workgroup bodies, so afterwards every
 * handle's T_out, converged, nr_iterations, gorio_apd_gicp_mp_diag, gorio_apd_gicp_mp_last_hessian and gorio_apd_gicp_mp_get_neighbors are
 * bit for bit those of its own gorio_apd_align.  A handle that ends early (converged, no neighbour at all, a non-finite step) ends alone.
 * gorio_apd_params and the radius are per handle and MAY differ; targets and sources may be shared by the rules of the single align (sharers
 * of one cloud: one k_correspondences and regularization).  count == 0: GORIO_OK.  count < 0, a null array or entry, the same handle twice,
 * handles on two devices: GORIO_ERR_INVALID; a handle of another method or without its clouds: GORIO_ERR_STATE; whatever else the single align
 * refuses for a member, with that member's code -- all checked before anything is built or launched, the text on handles[0] naming the index
 * ("handle <q>: ...").  Preparation (covariances, the target's index, buffers) runs handle by handle before the first round.
 * gorio_apd_gicp_mp_batch_diag (of the lead, handles[0]): rounds = the most passes any member ran, launches and synchronisations of all
 * rounds, and the launches of the most expensive round.
 */
int gorio_apd_gicp_mp_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations);
int gorio_apd_gicp_mp_batch_diag(const gorio_apd_t* lead, int* rounds, int* launches, int* syncs, int* max_round_launches);
int gorio_apd_gicp_mp_last_hessian(const gorio_apd_t* h, double* H36);
int gorio_apd_set_gicp_mp_params(gorio_apd_t* h, double neighbor_search_radius);
int gorio_apd_get_gicp_mp_params(const gorio_apd_t* h, double* neighbor_search_radius);
int gorio_apd_gicp_mp_get_covariances(gorio_apd_t* h, int which, int capacity, int* n, float* cov);
int gorio_apd_gicp_mp_pass(gorio_apd_t* h, const float T16[16], int* used, long long* total, double* H, double* g);
int gorio_apd_gicp_mp_get_neighbors(gorio_apd_t* h, long long capacity, int* n_queries, long long* total, long long* offsets, int* idx, float* sqd);
int gorio_apd_gicp_mp_get_merged(gorio_apd_t* h, int capacity, int* n, float* mean_B, float* cov_B, int* used);
int gorio_apd_gicp_mp_diag(const gorio_apd_t* h, int* passes, int* used, long long* total, double* stage_seconds);

/* parity hooks (VGICP mode; they build the map when it is stale): voxelmap_ (VGH:85) as arrays over the occupied voxels in ascending
 * lexicographic (x, y, z) coordinate order -- coord3: 3 ints, num_points, mean4: GaussianVoxel::mean, cov16: GaussianVoxel::cov row-major
 * (VOX:74-76).  n_voxels always receives the voxel count; the arrays (any may be NULL) are filled when capacity >= that count.
 * gorio_apd_get_voxel_correspondences: voxel_correspondences_ (VGH:86) of the last linearise as the fixed table [n_source][n_offsets],
 * offsets in the order of VOX:16-43, entries = voxel position in the order above or -1. */
int gorio_apd_get_voxelmap(gorio_apd_t* h, int* coord3, int* num_points, double* mean4, double* cov16, int capacity, int* n_voxels);
int gorio_apd_get_voxel_correspondences(gorio_apd_t* h, int* voxel_idx, int n_source_times_offsets);

/*
 * setInputSource APD:115-124 / setInputTarget APD:127-135.  xyz points at the first x; consecutive points are
 * `point_stride_bytes` apart (48 for pcl::PointXYZINormal, 12 for packed xyz); label points at the first cluster label
 * (PointXYZINormal::normal_x, written by preprocessing_nodelet_ntu.cpp:561-568) with the same stride, or NULL (all 0).
 * Copies the cloud to the device as SoA and invalidates that cloud's covariances (APD:122, 133).  The pointer-equality
 * early-out of APD:116-118 / 128-130 is the C++ shim's job (it owns the shared_ptrs).
 */
int gorio_apd_set_source(gorio_apd_t* h, const float* xyz, const float* label, int n, int point_stride_bytes);
int gorio_apd_set_target(gorio_apd_t* h, const float* xyz, const float* label, int n, int point_stride_bytes);
/* Same, from DEVICE-resident SoA buffers (x, y, z, label each n floats; label may be NULL): device-to-device copy. */
int gorio_apd_set_source_device(gorio_apd_t* h, const float* d_x, const float* d_y, const float* d_z, const float* d_label, int n);
int gorio_apd_set_target_device(gorio_apd_t* h, const float* d_x, const float* d_y, const float* d_z, const float* d_label, int n);

/* Batched form of the two calls above for `count` handles on one device: ONE copy launch for all clouds.  source / target: arrays
 * of `count` descriptors, or NULL to leave that side of every handle untouched.  Same semantics as the single calls: the clouds are
 * copied (device-to-device, on the library's stream) and the covariances of every touched cloud are invalidated. */
typedef struct {
  const float* x;
  const float* y;
  const float* z;
  const float* label; /* may be NULL */
  int n;
} gorio_apd_device_cloud;
int gorio_apd_set_clouds_device_batch(gorio_apd_t** handles, int count, const gorio_apd_device_cloud* source, const gorio_apd_device_cloud* target);

/* Batch extension (no counterpart in the reference, where every FastAPDGICP object builds its own kd-tree and covariances even when
 * two objects are handed the same cloud pointer): h's target becomes THE SAME device-resident cloud as owner's current target --
 * points, covariances and search index exist once per GPU however many handles register against them (BASELINE config C5: 512 scan
 * pairs against one 1 M-point map: one upload, one index build and one k-NN pass instead of 512).  Both handles must live on one
 * device.  Results are identical to giving h a private copy PROVIDED every sharer estimates covariances with the same k_correspondences
 * and regularization (the reference estimates them per object with its own settings, APD:149-154; here the shared cloud carries one set):
 * sharing with, or aligning / linearizing on, a handle whose two parameters differ from the ones the shared covariances were estimated with
 * fails with GORIO_ERR_INVALID (covariances supplied through gorio_apd_set_target_covariances carry no parameters and suit every
 * sharer).  The link is by value of the moment: a later setInputTarget / clearTarget on either handle detaches that handle only.
 * gorio_apd_set_target_covariances on a shared target is seen by every sharer. */
int gorio_apd_set_target_shared(gorio_apd_t* h, gorio_apd_t* owner);

/*
 * Scan-to-submap target assembly (scan_matching_odometry_nodelet.cpp:602-618, "SMO"): what the nodelet does on the CPU before
 * registration_s2m->setInputTarget -- every keyframe cloud moved by rel_pose = odom_i^-1 * odom_newest (pcl::transformPointCloud with
 * a double matrix, SMO:606-608), concatenated in the order given (SMO:609), passed through downsample() (SMO:611, 405-415) -- here on
 * the GPU, straight into the handle's device-resident target (the covariances of the new target are stale, as after setInputTarget).
 *   voxel_leaf <= 0   downsample_method NONE of the shipped launch files: pcl::PassThrough, i.e. only non-finite points are dropped
 *   voxel_leaf  > 0   pcl::VoxelGrid with that leaf size, downsample_all_data (SMO:145-149): one centroid per occupied voxel, in
 *                     ascending voxel index; the label of a voxel is the NORMALISED sum of its points' labels (sign), as
 *                     AccumulatorNormal leaves normal_x
 * n_target (may be NULL) receives the number of points of the assembled target; gorio_apd_get_target_points reads them back (xyz and
 * label strided like set_target's input; label_out may be NULL).
 */
typedef struct {
  const float* xyz;        /* first x of the keyframe cloud (host) */
  const float* label;      /* first normal_x, same stride, or NULL */
  int n;
  int point_stride_bytes;  /* 48 for pcl::PointXYZINormal */
  const double* rel_pose;  /* 16 doubles, ROW-major 4x4 */
} gorio_apd_keyframe;
int gorio_apd_set_target_submap(gorio_apd_t* h, const gorio_apd_keyframe* frames, int count, double voxel_leaf, int* n_target);
int gorio_apd_get_target_points(gorio_apd_t* h, float* xyz_out, float* label_out, int n, int point_stride_bytes);

/*
 * downsample_method of the nodelets (SMO:140-154): which filter the voxel_leaf > 0 branch of gorio_apd_set_target_submap and
 * gorio_apd_set_target_submap_keyframes runs.  VOXELGRID is the default and today's behaviour, bit for bit.  APPROX_VOXELGRID runs
 * pcl::ApproximateVoxelGrid (definition: include/gorio_prep.h, gorio_prep_approx_voxel_downsample) with the cubic leaf (float)voxel_leaf
 * over the assembled (x, y, z, label) points, all four fields averaged alike: the label is the plain float mean, not VoxelGrid's
 * normalised sign, and the output is in the filter's flush order.  A cloud the filter refuses (a cell coordinate outside
 * (-2^30, 2^30)) gives GORIO_ERR_INVALID and leaves the previous target in place.  voxel_leaf <= 0 is the same in both modes.
 * The method stays until it is set again.  A value other than the two is GORIO_ERR_INVALID.
 */
typedef enum { GORIO_DOWNSAMPLE_VOXELGRID = 0, GORIO_DOWNSAMPLE_APPROX_VOXELGRID = 1 } gorio_downsample_method;
int gorio_apd_set_submap_downsample(gorio_apd_t* h, int method);
int gorio_apd_get_submap_downsample(const gorio_apd_t* h, int* method);

/* clearSource APD:101-105, clearTarget APD:107-112, swapSourceAndTarget APD:89-98 */
int gorio_apd_clear_source(gorio_apd_t* h);
int gorio_apd_clear_target(gorio_apd_t* h);
int gorio_apd_swap_source_and_target(gorio_apd_t* h);

/* setSourceCovariances APD:138-140 / setTargetCovariances APD:143-145: n * 16 doubles.  When n differs from the size of the cloud
 * currently set (or no cloud is set) the call leaves that cloud WITHOUT covariances and returns GORIO_OK: the reference keeps such a
 * vector but recomputes the covariances at the next align because the sizes differ (APD:149-154). */
int gorio_apd_set_source_covariances(gorio_apd_t* h, const double* cov4x4, int n);
int gorio_apd_set_target_covariances(gorio_apd_t* h, const double* cov4x4, int n);
/* getSourceCovariances APDH:73-75 / getTargetCovariances APDH:77-79.  Returns the number of covariances currently held
 * (0 when stale, as source_covs_.size() would); copies min(count, n) of them when cov4x4 != NULL. */
int gorio_apd_get_source_covariances(gorio_apd_t* h, double* cov4x4, int n);
int gorio_apd_get_target_covariances(gorio_apd_t* h, double* cov4x4, int n);
/* calculate_covariances APD:351-411 for whichever cloud is stale (what computeTransformation does first, APD:149-154) */
int gorio_apd_calculate_covariances(gorio_apd_t* h);
/* parity hook: the k neighbour indices (sorted by distance, ties by index) used for cloud `which` (0 source, 1 target);
 * idx holds n*k ints.  Only valid after the covariances were computed by this library with params.keep_knn_indices set. */
int gorio_apd_get_knn_indices(gorio_apd_t* h, int which, int* idx, int n_times_k);

/*
 * computeTransformation APD:148-157 + LsqRegistration::computeTransformation LSQ:55-80 (what pcl::Registration::align
 * dispatches to).  guess / T_out: row-major float 4x4 (final_transformation_, LSQ:78); H_out: 36 doubles
 * (final_hessian_, LSQ:120/168; may be NULL); converged = hasConverged(); nr_iterations = nr_iterations_ (LSQ:68).
 * n_linearize (may be NULL) = number of linearize() calls executed = the unit of the throughput metric.
 */
int gorio_apd_align(gorio_apd_t* h, const float guess[16], float T_out[16], double* H_out, int* converged, int* nr_iterations, int* n_linearize);

/* same for `count` independent handles advanced in lock-step on one device (one launch set per iteration).
 * guesses / T_out: count * 16 floats; H_out: count * 36 doubles or NULL; the int outputs: count entries or NULL.
 * All handles must be distinct, live on one device and carry the same parameters (cl_weight_points is per handle); otherwise
 * GORIO_ERR_INVALID.  Targets may be shared between the handles (gorio_apd_set_target_shared). */
int gorio_apd_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize);

/* linearize APD:224-307 (== evaluateCost LSQ:50-52 with a double pose): updates correspondences + Mahalanobis matrices at
 * T (row-major double 4x4) and returns H (36, may be NULL together with b), b (6) and the weighted error. */
int gorio_apd_linearize(gorio_apd_t* h, const double T[16], double* H, double* b, double* error);
/* compute_error APD:310-346: error at T with the correspondences / Mahalanobis matrices of the last linearize */
int gorio_apd_compute_error(gorio_apd_t* h, const double T[16], double* error);
/* parity hooks: correspondences_ / sq_distances_ (APDH:113-114) and mahalanobis_ (APDH:111; n*16 doubles, row/col 3 zero;
 * entries of rejected points are zero) of the last linearize.  The matrices are materialised by gorio_apd_linearize and by a
 * Levenberg-Marquardt align (whose error trials read them); a Gauss-Newton align skips the store, after it get_mahalanobis and
 * compute_error return GORIO_ERR_STATE until the next gorio_apd_linearize. */
int gorio_apd_get_correspondences(gorio_apd_t* h, int* corr, float* sq_dist, int n);
int gorio_apd_get_mahalanobis(gorio_apd_t* h, double* maha4x4, int n);

/* pcl::transformPointCloud(*input_, output, final_transformation_) of LSQ:79 on the device-resident source:
 * xyz_out strided like set_source's input (only x, y, z are written). */
int gorio_apd_transform_source(gorio_apd_t* h, const float T[16], float* xyz_out, int n, int point_stride_bytes);

/* pcl::Registration::getFitnessScore(max_range) as the callers use it (scan_matching_odometry_nodelet.cpp:675,
 * loop_detector.cpp:411): mean squared NN distance of the source moved by T over the points whose SQUARED distance is <= max_range
 * (PCL compares the squared distance with max_range), DBL_MAX when no point qualifies.  When inlier_fraction != NULL it also
 * receives the inlier fraction of publish_scan_matching_status (scan_matching_odometry_nodelet.cpp:677-689): the share of source
 * points whose squared NN distance is < inlier_dist * inlier_dist.  The nodelet hard-codes max_correspondence_dist = 0.5 m there
 * (SMO:677); pass inlier_dist <= 0 to get exactly that.  Neither statistic depends on corr_dist_threshold.  A handle that searches only
 * its rank's share of the source (gorio_apd_comm_init / gorio_apd_debug_set_shard with more than one rank) returns GORIO_ERR_STATE: score
 * the pose on an unsharded handle. */
int gorio_apd_fitness_score(gorio_apd_t* h, const float T[16], double max_range, double inlier_dist, double* score, double* inlier_fraction);

/* gorio_apd_fitness_score for `count` handles in one pass: N x getFitnessScore (SMO:675, loop_detector.cpp:411) -- the scoring of the loop
 * candidates of loop_detector.cpp:386-422, one target and N aligned sources -- without N round trips.  T: count * 16 floats (row-major, pose
 * of handle i at T + 16 i); score: count entries; inlier_fraction: count entries or NULL.  score[i] / inlier_fraction[i] are BIT FOR BIT
 * those of gorio_apd_fitness_score(handles[i], T + 16 i, max_range, inlier_dist, ...): DBL_MAX when no point qualifies, inlier_dist <= 0
 * means 0.5 m, every handle searches in its own search mode with the same rounded-up bound.  One index build for the clouds that lack one
 * (a target shared through gorio_apd_set_target_shared is built once), one 1-NN search launch per search mode, one reduction launch, one
 * device-to-host copy and one synchronisation for the whole batch.  Handles must be distinct, live on one device and have both clouds set;
 * their parameters may differ.  A sharded handle (gorio_apd_comm_init / gorio_apd_debug_set_shard with more than one rank) gives
 * GORIO_ERR_STATE.  count == 0 returns GORIO_OK.  On a validation error no handle is changed and handles[0]'s last error names the index
 * of the offending handle.  Afterwards, as after the single call, no handle holds correspondences (gorio_apd_get_correspondences fails). */
int gorio_apd_fitness_score_batch(gorio_apd_t** handles, int count, const float* T, double max_range, double inlier_dist, double* score, double* inlier_fraction);

/*
 * Sharded-source mode -- "one large co-registration" (no counterpart in the reference, whose parallelism is one OpenMP
 * team): several processes, one per GPU, each with a handle holding the SAME source and target clouds, form an RCCL communicator
 * (RCCL = the "nccl" of ROCm, over xGMI inside a node).  From then on gorio_apd_align / _linearize / _compute_error on those handles
 * are COLLECTIVE calls -- every rank makes them, in the same order with the same arguments.  Each rank searches and linearises only
 * its contiguous part of the source (a spatially compact run of the search order); the covariances are estimated on the whole
 * clouds by every rank, so they are exactly those of an unsharded run.  The only exchange is one in-place ncclAllReduce of 28
 * doubles (H upper triangle, b, error) per linearisation and of 1 double per Levenberg-Marquardt trial, enqueued on the launch stream
 * between the kernels; every rank then takes the same 6 x 6 step, so all ranks return the same pose without a broadcast and the
 * result equals the unsharded one up to the rounding of the reordered fp64 sums.
 *   rank 0:   gorio_comm_get_unique_id(id);  hand the 128 bytes to the other ranks by any means (MPI, torch.distributed, a file)
 *   all:      gorio_apd_comm_init(h, world_size, rank, id);  ...  gorio_apd_comm_destroy(h);
 * A handle with a communicator cannot be part of a gorio_apd_align_batch.  librccl is loaded on first use.
 */
int gorio_comm_get_unique_id(char id[128]);
int gorio_apd_comm_init(gorio_apd_t* h, int world_size, int rank, const char id[128]);
int gorio_apd_comm_destroy(gorio_apd_t* h);
/* What RCCL reports about the handle's communicator (ncclCommCount, ncclCommUserRank) and how many ncclAllReduce calls the handle has
 * enqueued on it since comm_init: evidence for benchmarks and tests that the collective path ran across that many ranks.  Any output
 * pointer may be NULL.  GORIO_ERR_STATE without a communicator. */
int gorio_apd_comm_info(gorio_apd_t* h, int* world_size, int* rank, long long* allreduce_count);
/* Test hook: the source partition of rank `rank` of `world_size` WITHOUT a communicator -- gorio_apd_linearize / _compute_error then
 * return this rank's partial sums (a test adds them up itself; two such handles can live on one GPU, which two RCCL ranks cannot).
 * world_size = 1 switches it off. */
int gorio_apd_debug_set_shard(gorio_apd_t* h, int world_size, int rank);
/* Test hooks of the two schedule optimisations of a Gauss-Newton align, so that a regression can be localised (both default to on; neither
 * changes a result):
 *   fuse_step   != 0: the optimiser step of LSQ:107-123 runs in the LAST workgroup of the linearisation launch (a fence-free hand-over
 *                     validated on gfx950); 0: it runs as its own launch after the linearisation.
 *   plan_search != 0: from the third correspondence search of an align on, query waves that were slow in the second one are cut into
 *                     parts and dispatched heaviest first; 0: every search uses the natural schedule. */
int gorio_apd_debug_set_schedule(gorio_apd_t* h, int fuse_step, int plan_search);
/* Test hook: read back the search index of the source (which = 0) or the target (1) as the pruned searches see it.  sizes receives
 * { n, n_spad, n_tiles, n_super, n_blocks, kd chunk size }; every other pointer may be NULL (call once for the sizes, then again):
 *   sxyz [7 * n_spad]   sx, sy, sz (n_spad floats each), then s4 as n_spad x (x, y, z, original index bits)
 *   orig [n_spad]       original index per sorted position, 0x7fffffff for padding
 *   tbox [n_tiles * 8], sbox [n_super * 8], bbox [n_blocks * 8]   lo.x lo.y lo.z 0 hi.x hi.y hi.z 0
 * GORIO_ERR_STATE when the handle holds no valid index for that cloud. */
int gorio_apd_debug_get_index(gorio_apd_t* h, int which, int sizes[6], float* sxyz, int* orig, float* tbox, float* sbox, float* bbox);
/* Test hook: how many 64-point groups the redo pass of the last k-NN covariance estimation this handle led did (pruned search, k <= 20:
 * the groups in which some point has more than 24 neighbours at or below its k-th distance, i.e. massive ties; 0 on ordinary clouds).
 * Waits for the handle's stream.  GORIO_ERR_STATE when the handle has led no such estimation. */
int gorio_apd_debug_knn_redo_groups(gorio_apd_t* h, int* groups);

/* seconds spent inside device kernels of the last align / align_batch, by stage (HIP events on the launch stream):
 * [0] k-NN + covariance estimation, [1] correspondence search, [2] linearize, [3] LM/GN solve + error trials, [4] search-index build
 * (Morton sort, kd refinement, boxes; pruned mode only), [5..7] reserved (0); plus launch-set counts in counts[0..7] (either may be
 * NULL).  Filled only after gorio_apd_set_profiling(h, 1). */
int gorio_apd_set_profiling(gorio_apd_t* h, int enable);
int gorio_apd_get_stage_times(gorio_apd_t* h, double seconds[8], int counts[8]);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_APD_H */
