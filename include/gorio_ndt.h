/*
 * gorio_ndt.h -- C ABI of NDT_OMP registration on the MI355X (libgorio_amd.so): pclomp::NormalDistributionsTransform, the default
 * that select_registration_method hands out (REG:27, 102-135), with its DIRECT1 / DIRECT7 / DIRECT26 neighbourhoods.
 *
 * Paths relative to the Go-RIO sources:
 *   NDT  = ndt_omp/include/pclomp/ndt_omp_impl.hpp       NDTH = ndt_omp/include/pclomp/ndt_omp.h
 *   VGC  = ndt_omp/include/pclomp/voxel_grid_covariance_omp_impl.hpp
 *   REG  = 4DRadarSLAM/src/radar_graph_slam/registrations.cpp
 *
 * Same conventions as include/gorio_sc.h: plain pointers, host pointers caller-owned and only read / written during the call, 0 on
 * success or a negative gorio_status (include/gorio_apd.h), gorio_ndt_last_error() gives the text (thread-local).  No CPU fallback:
 * without a HIP device gorio_ndt_create fails with GORIO_ERR_NO_DEVICE.  The handle is its own type: NDT shares no optimiser, search
 * or per-point state with the GICP family of include/gorio_apd.h.  One handle must not be used from two threads at once.
 *
 * Where the work runs: the voxel map (VGC:60-370), the derivative sums (NDT:180-285, 540-645) and the score (NDT:935-983) on the device;
 * the Newton / More-Thuente shell (NDT:81-171, 648-932) on the host in plain C++, one derivative evaluation per round trip (28 doubles
 * down, one small kernel argument up).  Sums of a leaf run in input order in fp64; the derivative sums are reduced wave -> block ->
 * block order without floating-point atomics, so two runs give the same bits.
 *
 * What is fixed here where the reference leaves it to a library (DESIGN.md section 2 lists the same definitions; parity is against a
 * NumPy restatement of them, the reference cannot be compiled without PCL and Eigen):
 *   - float sin / cos / atan2 / exp are the correctly rounded float results (computed in double, rounded once);
 *   - 3-term float products sum left to right, un-fused; pcl::transformPointCloud is ((m0 x + m1 y) + m2 z) + m3 in float;
 *   - Transform<float, 3, Affine>::rotation() (NDT:109) is taken as the linear part of the guess (exact for an orthonormal guess);
 *   - DIRECT26 walks the 26 offsets of pcl::getAllNeighborCellIndices (PCL 1.10 voxel_grid.h) in its order: no centre cell;
 *   - SelfAdjointEigenSolver of a leaf is the library's fp64 cyclic Jacobi on the lower triangle; cov_.inverse() the cofactor inverse;
 *   - the Hessian of computeDerivatives is the upper triangle hessian(i, j), i <= j (NDT:529), mirrored (the reference's 36 float
 *     terms are symmetric only up to rounding);
 *   - JacobiSVD<6x6>::solve(-g): symmetric Jacobi eigen-decomposition H = V L V^T, x = V L^+ V^T (-g), singular values |L| not above
 *     6 eps max|L| count as zero (Eigen's default threshold);
 *   - non-finite target points are skipped (VGC:136-138, 213-215) and the bounding box is that of the finite points.
 * Reference behaviour kept although it looks like a slip: the float table row d1 of computeAngleDerivatives holds +sy (NDT:383) where
 * the double row used by computeHessian holds -sy (NDT:361).  So computeHessian (NDT:929, after a line search with inner iterations) is
 * NOT computeDerivatives asked for the Hessian only: it is the same traversal and the same formula (NDT:639-641 = NDT:529-531) in
 * double throughout with the double tables; the derivative kernel has both instantiations.
 * A non-finite SOURCE point is refused at set time (GORIO_ERR_INVALID): the reference converts floor(x / leaf) of it to int, which is
 * undefined.  A finite point whose cell coordinate does not fit 31 bits has no neighbour.
 *
 * Many aligns at once: gorio_ndt_align_batch advances `count` handles in lock-step, one derivative evaluation of every unfinished handle
 * per round, so a round costs the launches and the round trip of ONE evaluation whatever the count.  The host shell is the same
 * resumable machine that gorio_ndt_align drives; the batched kernels run the single kernels' per-workgroup body over the same 256-point
 * blocks and add the block partials in the same order.  The contract of the call: every output of handle i is BIT FOR BIT that of
 * gorio_ndt_align(handles[i], guesses + 16 i, ...).  gorio_ndt_set_target_shared lets handles look at one target (points and voxel
 * map exist once on the device), as the loop-closure flow wants it: N candidate sources against one keyframe.
 *
 * Inputs that are already on the device: gorio_ndt_set_source_from_scan / _set_target_from_scan take the output of the scan pipeline
 * (include/gorio_scan.h), gorio_ndt_set_target_from_apd the current target of a registration handle of include/gorio_apd.h (the
 * scan-to-submap target, say), each as one device-to-device copy.  gorio_ndt_calculate_score_batch is the score's batch form.
 *
 * The radius neighbourhood: pcl::NormalDistributionsTransform (REG:109-115, plain "NDT") and pclomp's KDTREE (NDT:234-235, 573-574,
 * 948-949) take every neighbourhood from target_cells_.radiusSearch(x_trans_pt, resolution_, ...) over the cloud of leaf centroids.
 * gorio_ndt_set_radius_search(h, 1) selects it, whatever params.search holds; params.search = GORIO_NDT_KDTREE itself stays refused
 * by gorio_ndt_set_params (GORIO_ERR_UNSUPPORTED; the text names gorio_ndt_set_radius_search).  What is fixed here for that mode:
 *   - CENTROID CLOUD (VGC:282-326): one point per leaf with nr_points >= min_points_per_voxel, in ascending leaf index.  A leaf that
 *     VGC:337-341 or VGC:360-364 disables afterwards stays in the cloud (it is pushed before the `continue`) and is a neighbour with
 *     a ZERO inverse covariance: the constructor's value (VGCH:108) for the first rule; for the second the reference would carry
 *     the infinities, here the leaf's icov is zero as gorio_ndt_get_voxels reports it;
 *   - CENTROID COORDINATES are float: the running float sum of the leaf's points in input order (VGC:242-243) divided per element
 *     by (float) nr_points (VGC:289, a true division).  The search index is over these floats; cell->getMean() in the pair
 *     arithmetic stays the double mean.  A float sum that overflows makes the cloud non-finite: the evaluation is refused
 *     (GORIO_ERR_INVALID);
 *   - SEARCH: radius resolution_ (the float member), max_nn = 0, the rule of include/gorio_search.h: un-fused float L2_Simple,
 *     strictly below (float)((double) r * (double) r), results in ascending (distance, centroid index) -- the order a point's pair
 *     terms are added in.  A query without a centroid in range has no neighbour; there is no cell-range test on this path; a map
 *     without an eligible leaf gives zero sums;
 *   - PAIR ARITHMETIC is unchanged (the float path, the float path with the Hessian, the double computeHessian); calculateScore
 *     divides a point's sum by neighborhood.size().
 * An evaluation is one query launch (the float-transformed source: the bits the search sees are the bits the pair arithmetic reads),
 * one radius search (a CSR) and one launch that walks each point's segment; they run on the device's launch stream, where the search
 * runs.  The centroid cloud and its index belong to the target state (sharers of gorio_ndt_set_target_shared see ONE index) and are
 * built by the first call that needs them.
 *
 * Out of scope: RCCL sharding; params.search = GORIO_NDT_KDTREE as a spelling of the radius mode (it stays refused, see above).
 */
#ifndef GORIO_NDT_H
#define GORIO_NDT_H

#ifdef __cplusplus
extern "C" {
#endif

/* pclomp::NeighborSearchMethod, NDTH:52-57, in its order */
enum gorio_ndt_search { GORIO_NDT_KDTREE = 0, GORIO_NDT_DIRECT26 = 1, GORIO_NDT_DIRECT7 = 2, GORIO_NDT_DIRECT1 = 3 };

typedef struct {
  double resolution;              /* setResolution, NDTH default 1.0 (a float member); REG:108 passes 0.5.  <= 0: GORIO_ERR_UNSUPPORTED */
  double step_size;               /* setStepSize, 0.1 */
  double outlier_ratio;           /* setOutlierRatio, 0.55 */
  double transformation_epsilon;  /* 0.1 (NDT:71); REG:124 passes 0.01 */
  int max_iterations;             /* 35 (NDT:72); REG:125 passes 64 */
  int search;                     /* gorio_ndt_search, DIRECT7 (NDT:74) */
  int min_points_per_voxel;       /* VoxelGridCovariance: 6 */
  double min_covar_eigvalue_mult; /* VoxelGridCovariance: 0.01 */
} gorio_ndt_params;

/* What one align did. */
typedef struct {
  int n_derivatives;  /* computeDerivatives calls (NDT:119, 837, 881) */
  int n_hessians;     /* computeHessian calls (NDT:929) */
  int n_mt_iterations;/* More-Thuente inner iterations, summed over the outer iterations (NDT:850-923) */
  double score;       /* the score of the last evaluation */
} gorio_ndt_diag;

typedef struct gorio_ndt gorio_ndt_t;
struct gorio_scan; /* gorio_scan_t of include/gorio_scan.h */
struct gorio_apd;  /* gorio_apd_t of include/gorio_apd.h */

/* The constructor's values, NDT:47-76. */
void gorio_ndt_default_params(gorio_ndt_params* p);
/* new pclomp::NormalDistributionsTransform (NDT:47-76) with the default parameters. */
int gorio_ndt_create(gorio_ndt_t** out, int device);
void gorio_ndt_destroy(gorio_ndt_t* h);
/* The setters of NDTH:115-191 in one call.  A changed resolution (or leaf rule) marks the voxel map stale (NDTH:133-142).  KDTREE
 * (its neighbourhood is selected by gorio_ndt_set_radius_search instead), unknown search values and resolution <= 0 are refused with
 * GORIO_ERR_UNSUPPORTED and change nothing. */
int gorio_ndt_set_params(gorio_ndt_t* h, const gorio_ndt_params* p);
int gorio_ndt_get_params(const gorio_ndt_t* h, gorio_ndt_params* p);

/* The radius neighbourhood of pcl::NormalDistributionsTransform / pclomp::KDTREE (see the head of this file): 0 by default.  While it
 * is on, every neighbourhood of computeDerivatives, computeHessian and calculateScore is the radius search over the leaf centroids,
 * whatever params.search holds; params.search is kept and rules again when the switch goes off.  A changed value keeps the map and
 * invalidates the neighbour lists gorio_ndt_get_neighbours reports.  NULL arguments: GORIO_ERR_INVALID. */
int gorio_ndt_set_radius_search(gorio_ndt_t* h, int enable);
int gorio_ndt_get_radius_search(const gorio_ndt_t* h, int* enabled);

/* setInputTarget (NDTH:122-127): xyz points at the first x, stride_bytes between points (a multiple of 4, >= 12), n >= 0.  The map is
 * built at the next call that needs it.  Non-finite points are accepted and skipped by the map. */
int gorio_ndt_set_target(gorio_ndt_t* h, const float* xyz, int n, int stride_bytes);
/* setInputSource.  A non-finite point is refused with GORIO_ERR_INVALID and the source held stays. */
int gorio_ndt_set_source(gorio_ndt_t* h, const float* xyz, int n, int stride_bytes);
/* The same from device arrays x[n], y[n], z[n] of the handle's device (copied on the handle's stream). */
int gorio_ndt_set_target_device(gorio_ndt_t* h, const float* x, const float* y, const float* z, int n);
int gorio_ndt_set_source_device(gorio_ndt_t* h, const float* x, const float* y, const float* z, int n);

/* h's target becomes owner's current target: points and voxel map exist once (no reference member; the semantics of
 * gorio_apd_set_target_shared).  Both handles must live on one device (GORIO_ERR_INVALID) and the owner must have a target
 * (GORIO_ERR_STATE).  The link is by value of the moment: a later gorio_ndt_set_target / _set_target_device on either handle detaches that
 * handle only, and destroying the owner leaves the sharers working.
 * Map parameters (resolution, min_points_per_voxel, min_covar_eigvalue_mult): while a target is held by ONE handle a changed value marks
 * the map stale and the next use rebuilds it.  While it is held by several, a handle whose three values differ from those the valid map
 * was built with gets GORIO_ERR_INVALID from every call that needs the map (the text names the parameter); when no valid map exists
 * yet, the first handle that needs one builds it with its own values.  search, step_size, outlier_ratio, transformation_epsilon and
 * max_iterations are per handle and may differ between sharers. */
int gorio_ndt_set_target_shared(gorio_ndt_t* h, gorio_ndt_t* owner);

/* Parity hook: the leaves of VoxelGridCovariance::applyFilter (VGC:60-370) in ascending linear leaf index (the order of the reference's
 * std::map).  *n_leaves is always set; the arrays (any may be NULL) need capacity >= *n_leaves leaves: leaf_index, nr_points (-1 for a
 * leaf the reference disables, VGC:336-339, 360-363), mean [3], cov_raw [9] (VGC:329-330, before the inflation; zero below
 * min_points_per_voxel), cov [9] (after VGC:341-357), icov [9] (zero for leaves that are not neighbours), row-major; min_b [3], div_b [3]. */
int gorio_ndt_get_voxels(gorio_ndt_t* h, int capacity, int* n_leaves, int* leaf_index, int* nr_points, double* mean, double* cov_raw, double* cov, double* icov,
                         int* min_b, int* div_b);

/* Parity hooks of the radius mode.  gorio_ndt_get_centroids: the centroid cloud (built now when it is stale, switch on or off);
 * *n_centroids is always set, xyz [3 per centroid] and leaf_pos [position of the centroid's leaf in gorio_ndt_get_voxels' order] may be
 * NULL and need capacity >= *n_centroids.  gorio_ndt_get_neighbours: the CSR of this handle's LAST radius evaluation (derivatives,
 * Hessian, score, or the last evaluation of an align, single or batched): offsets [source size + 1], then per neighbour its leaf
 * position and float squared distance, in the order the pair terms were added; capacity (entries of leaf_pos / sqd) below the total
 * gives GORIO_ERR_INVALID and writes nothing.  GORIO_ERR_STATE when there is no such evaluation, or the source, the target or the
 * switch changed since. */
int gorio_ndt_get_centroids(gorio_ndt_t* h, int capacity, int* n_centroids, float* xyz, int* leaf_pos);
int gorio_ndt_get_neighbours(gorio_ndt_t* h, long long* offsets, int* leaf_pos, float* sqd, long long capacity);

/* setInputSource / setInputTarget with the output of the pipeline's last OK run (the points gorio_scan_get_output reports, in its
 * order), without a host round trip: one device-to-device copy of x, y, z into the handle's own buffers, ordered behind the pipeline's
 * stream by an event.  It is a copy, not a share: the pipeline may load its next frame at once, and none of its counters moves (no
 * upload, no index build, no download).  Afterwards the handle is as gorio_ndt_set_source_device / _set_target_device leave it for the
 * same points: a target detaches from its sharers and marks the map stale; a source is checked for non-finite points on the device
 * in the pass that copies it, and a refusal (GORIO_ERR_INVALID) leaves the source held in place.
 * Reported before any device call: a NULL handle of either kind or handles on different devices GORIO_ERR_INVALID, a pipeline whose
 * last run produced no frame GORIO_ERR_STATE. */
int gorio_ndt_set_source_from_scan(gorio_ndt_t* ndt, struct gorio_scan* scan);
int gorio_ndt_set_target_from_scan(gorio_ndt_t* ndt, struct gorio_scan* scan);
/* setInputTarget with the CURRENT target of a registration handle of gorio_apd.h (what gorio_apd_set_target_submap assembled, a scan
 * handed over to it, a device or host cloud), in the order gorio_apd_get_target_points reports it: the scan-to-submap mode
 * (SMO:602-618 of scan_matching_odometry_nodelet.cpp) for the default method.  The same copy, ordering and errors as above; a handle
 * without a target gives GORIO_ERR_STATE.  The registration handle is not changed and may take its next target at once. */
int gorio_ndt_set_target_from_apd(gorio_ndt_t* ndt, struct gorio_apd* apd);

/* No reference member: the elements the handle's device buffers hold, capacities[4] = target points, source points, leaves, sort keys
 * (the centroid cloud of the radius mode is at most one point per leaf and is not listed).
 * Buffers grow with the clouds and are kept when a smaller (or empty) cloud follows: equal capacities mean nothing was reallocated.
 * A handle whose target came through gorio_ndt_set_target_shared owns none of it and reports 0 for target points, leaves and sort keys.
 * A source that comes from the device (gorio_ndt_set_source_device, _set_source_from_scan) is checked while it is copied into a staging
 * buffer, which then changes places with the buffer held: "source points" is the buffer held. */
int gorio_ndt_get_capacities(const gorio_ndt_t* h, long long* capacities);

/* computeDerivatives (NDT:180-285) at pose vector p = (x, y, z, roll, pitch, yaw): the source is moved by the float matrix NDT:827-830
 * builds from p, the Gaussian constants are those of NDT:89-93 for the current parameters.  hessian is 6 x 6 row-major and may be NULL
 * when compute_hessian == 0 (NDT:881: the 21 Hessian sums are then skipped). */
int gorio_ndt_derivatives(gorio_ndt_t* h, const double* p, int compute_hessian, double* score, double* gradient, double* hessian);
/* computeHessian (NDT:540-645) at p: double throughout, see above. */
int gorio_ndt_hessian(gorio_ndt_t* h, const double* p, double* hessian);
/* calculateScore (NDT:935-983) of the source moved by the float 4 x 4 row-major T, constants as for gorio_ndt_derivatives. */
int gorio_ndt_calculate_score(gorio_ndt_t* h, const float* T, double* score);
/* computeTransformation (NDT:81-171) from the 4 x 4 row-major float guess (NULL: identity): T_out = final_transformation_,
 * converged, nr_iterations_, trans_probability_.  Any output but T_out may be NULL.  GORIO_ERR_STATE without a source or without a
 * target that has at least one finite point. */
int gorio_ndt_align(gorio_ndt_t* h, const float* guess, float* T_out, int* converged, int* nr_iterations, double* trans_probability, gorio_ndt_diag* diag);

typedef struct {
  int rounds;       /* lock-step rounds = device round trips of the batch */
  int evaluations;  /* derivative + Hessian evaluations summed over the handles */
  int launches;     /* kernel launches of the rounds (map builds not counted) */
} gorio_ndt_batch_stats;

/* computeTransformation for `count` handles in lock-step.  guesses: count * 16 floats (handle i's at guesses + 16 i) or NULL (identity);
 * T_out: count * 16 floats; converged / nr_iterations / trans_probability / diag: count entries or NULL; stats may be NULL.
 * Every output of handle i is BIT FOR BIT that of gorio_ndt_align(handles[i], guesses + 16 i, ...): the same host shell, the same
 * per-workgroup kernel body over source points [256 b, 256 b + 256) of block b, the block partials added in block order.
 * A round collects the pending evaluation of every unfinished handle, sends one job table (one asynchronous copy from pinned memory),
 * launches the derivative kernel once per evaluation mode present (score + gradient; + Hessian; computeHessian), folds all jobs in
 * one launch, and ends with one copy of 28 doubles per job and one synchronisation: launches <= 4 * rounds while every handle is DIRECT,
 * and rounds = max_i (n_derivatives_i + n_hessians_i).  Handles with the radius switch on may be mixed with DIRECT ones.  A round with
 * radius jobs adds ONE query launch over those jobs, ONE batched radius search over them (include/gorio_search.h: query keys and their
 * tiled sort, count, scan, fill, segment sort = 6 + s launches, s = 0 while the largest radius source has at most 4096 points and
 * m (m + 3) / 2 for 4096 * 2^m; segments hold at most 27 centroids, so the search's long-segment path never runs) and one walk launch
 * per evaluation mode present among them, and it runs on the device's launch stream: launches <= (14 + s) * rounds.  Stale maps are built before the first round, once per target state; finished
 * handles drop out of the later rounds.  The rounds run on handles[0]'s stream and scratch.
 * count == 0 returns GORIO_OK and touches no device.  count < 0, NULL handles or T_out, a NULL entry, a handle that appears twice or
 * handles on different devices: GORIO_ERR_INVALID.  A handle gorio_ndt_align would refuse (no target, no or an empty source, no finite
 * target point, a sharer whose map parameters do not fit the shared map) gives that error with the handle's index in the text.  On a
 * validation error no handle is changed and no evaluation runs.  Handles need not agree in any parameter. */
int gorio_ndt_align_batch(gorio_ndt_t* const* handles, int count, const float* guesses, float* T_out, int* converged, int* nr_iterations, double* trans_probability,
                          gorio_ndt_diag* diag, gorio_ndt_batch_stats* stats);

/* calculateScore (NDT:935-983) for `count` handles in one round trip.  T: count * 16 floats (handle i's at T + 16 i) or NULL (identity
 * for all); score: count doubles.  score[i] is BIT FOR BIT what gorio_ndt_calculate_score(handles[i], T + 16 i, &s) returns: the same
 * per-workgroup body over the same 256-point blocks, the block partials added in block order, the division by the source size on
 * the host (NDT:982).  One job table goes up, one score launch runs over all DIRECT handles (and, for handles with the radius switch
 * on, one query launch, one batched radius search and one walk launch), one fold launch, one copy of count doubles
 * and one synchronisation follow, on handles[0]'s stream and scratch; stale maps are built before, once per target state.
 * Validation as for gorio_ndt_align_batch: count == 0 returns GORIO_OK and touches no device; count < 0, NULL handles or score, a NULL
 * entry, a handle that appears twice or handles on different devices: GORIO_ERR_INVALID; a handle the single call would refuse gives
 * that error with the handle's index in the text.  On a validation error no handle is changed and nothing runs. */
int gorio_ndt_calculate_score_batch(gorio_ndt_t* const* handles, int count, const float* T, double* score);

const char* gorio_ndt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_NDT_H */
