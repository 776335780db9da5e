/*
 * gorio_scan.h -- C ABI of the whole radar preprocessing callback on the MI355X (libgorio_amd.so): one raw scan in, the cloud the
 * nodelet publishes out, the scan resident on the device through every stage in between.
 *
 * Paths relative to the Go-RIO sources:
 *   PREP = apps/preprocessing_nodelet_ntu.cpp      REVE = src/radar_ego_velocity_estimator.cpp
 *
 * Same conventions as include/gorio_prep.h and include/gorio_ground.h: plain pointers, host pointers caller-owned and only read /
 * written during the call, 0 on success or a negative gorio_status (include/gorio_apd.h), gorio_scan_last_error() gives the text
 * (thread-local).  No CPU fallback: gorio_scan_create only checks and stores the parameters; the first gorio_scan_load makes the device
 * side of the handle and fails with GORIO_ERR_NO_DEVICE without a HIP device.  Argument and state errors are reported before any device call.
 *
 * A pipeline is a handle because it carries per-sensor state across frames: the adaptive thresholds of the Patchwork++ segmenter it
 * wraps (include/gorio_ground.h), its device buffers and its staging.  One handle must not be used from two threads at once.
 *
 * One frame is two calls, gorio_scan_load then gorio_scan_run, because the caller draws the RANSAC samples of REVE and needs the
 * number of valid targets for that (the contract of gorio_prep_ego_velocity, include/gorio_prep.h).
 *
 * What crosses between host and device (DESIGN.md "Scan pipeline"): the raw scan goes up once.  Coming down are only what the host
 * parts of the stages already read in the single-call ABI -- the REVE feature rows (unit direction and corrected Doppler per target),
 * one float or int per point of the outlier filters, the Patchwork++ per-patch records and per-point patch ids, the DBSCAN adjacency,
 * three floats per cluster -- and going up are masks, orders and labels.  No stage downloads point coordinates and none is uploaded
 * again; gorio_scan_get_counters pins that.
 *
 * Deviation from the reference: PREP:385-386 compares coordinates with NAN and INFINITY by ==.  A comparison with NAN is always false,
 * so NaN points pass there (and -Inf passes the second test), and everything after them is undefined (std::sort on NaN heights, kd-tree
 * on NaN).  This pipeline drops every point with a NaN or +-Inf coordinate at the gate.
 */
#ifndef GORIO_SCAN_H
#define GORIO_SCAN_H

#include "gorio_apd.h"
#include "gorio_ground.h"
#include "gorio_prep.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { GORIO_SCAN_OUTLIER_NONE = 0, GORIO_SCAN_OUTLIER_STATISTICAL = 1, GORIO_SCAN_OUTLIER_RADIUS = 2 } gorio_scan_outlier_method;

/*
 * gorio_scan_default_params gives the NODELET's own defaults (the second argument of each private_nh.param, PREP:97-181, 526-529, 705).
 * The launch files (launch/ntu_*.launch) differ in: distance_far 200, z_high 100, outlier_method RADIUS with min_neighbors 1 (loop2) or
 * 5 (cp, loop3, nyl), mean_k 30, stddev_mul 1.2, and enable_dynamic_object_removal true in ntu_nyl.launch.  rotation defaults to the
 * identity: Radar_to_livox is a product of calibration matrices (PREP:104-129) that belongs to the sensor rig.
 */
typedef struct {
  float power_threshold;               /* PREP:98, 383: a point stays when its power is > this.  0 */
  double rotation[9];                  /* row-major 3 x 3 of Radar_to_livox; the reference zeroes the translation (PREP:390-394).  identity */
  int enable_dynamic_object_removal;   /* PREP:97, 464-478: continue with the REVE inliers only.  0 */
  int deskew;                          /* PREP:484, 658-719; applied only when gorio_scan_run is given an angular velocity.  1 */
  double scan_period;                  /* PREP:705.  0.1 */
  double distance_near, distance_far, z_low, z_high; /* PREP:178-181, 643-647.  1, 100, -5, 20; all finite */
  int outlier_method;                  /* gorio_scan_outlier_method, PREP:153-175.  STATISTICAL */
  int mean_k;                          /* PREP:155.  20; in [1, 31] */
  double stddev_mul;                   /* PREP:156.  1.0 */
  double radius;                       /* PREP:164.  2 */
  int min_neighbors;                   /* PREP:165.  2 */
  int ground;                          /* PREP:505-518: Patchwork++ and full_scan = ground + nonground.  1; 0 keeps the filtered cloud as it is */
  gorio_ground_params ground_params;   /* gorio_ground_default_params */
  int dbscan_core_min_pts;             /* PREP:526.  10 */
  double dbscan_eps;                   /* PREP:527.  0.9 */
  int dbscan_min_cluster_size;         /* PREP:528.  20 */
  int dbscan_max_cluster_size;         /* PREP:529.  25000 */
  gorio_reve_config reve;              /* gorio_prep_reve_default_config */
} gorio_scan_params;

typedef struct gorio_scan gorio_scan_t;

void gorio_scan_default_params(gorio_scan_params* p);
int gorio_scan_create(gorio_scan_t** out, int device, const gorio_scan_params* p);
void gorio_scan_destroy(gorio_scan_t* h);

/*
 * PREP:381-412 and the target gates of REVE:75-90.  One upload of the raw message fields; on the device the power test, the finite test
 * and the rotation R . (x, y, z) -- in double, r0 x + r1 y + r2 z summed left to right, rounded to float once -- then the survivors
 * compacted in order (the "gated cloud"), then the REVE features of the gated cloud.
 *   xyz / power / doppler   first x, first power (channels[2]), first Doppler (channels[0]); stride_bytes between points (a multiple of 4;
 *                           xyz needs 12 bytes)
 *   n_gated                 points of the gated cloud
 *   n_valid                 REVE targets that pass the gates: the RANSAC sample indices of gorio_scan_run address these, in order
 * n may be 0 (an empty message): both counts are 0 then and gorio_scan_run reports GORIO_SCAN_EMPTY.
 */
int gorio_scan_load(gorio_scan_t* h, const float* xyz, const float* power, const float* doppler, int n, int stride_bytes, int* n_gated, int* n_valid);

typedef enum {
  GORIO_SCAN_OK = 0,             /* a frame was produced */
  GORIO_SCAN_ZERO_VELOCITY = 1,  /* PREP:427-430: the estimate succeeded and |v_r| < 0.05: the frame is skipped */
  GORIO_SCAN_EMPTY = 2,          /* PREP:480-482: the cloud was empty after a stage (a later stage than the reference tests is reported alike) */
  GORIO_SCAN_REFUSED = 3         /* a stage refused the cloud; gorio_scan_run returns that stage's error code and gorio_scan_last_error its text */
} gorio_scan_status;

typedef enum {
  GORIO_SCAN_STAGE_GATE = 0,      /* PREP:381-412 */
  GORIO_SCAN_STAGE_DYNAMIC = 1,   /* PREP:464-478 */
  GORIO_SCAN_STAGE_DESKEW = 2,    /* PREP:484 (drops nothing) */
  GORIO_SCAN_STAGE_DISTANCE = 3,  /* PREP:502 */
  GORIO_SCAN_STAGE_OUTLIER = 4,   /* PREP:503 */
  GORIO_SCAN_STAGE_GROUND = 5,    /* PREP:511-518: ground ++ nonground */
  GORIO_SCAN_STAGE_COUNT = 6,     /* the stages that put out a cloud: what gorio_scan_get_stage accepts */
  GORIO_SCAN_STAGE_DBSCAN = 6     /* PREP:520-568: drops and moves nothing (its cloud is that of GROUND), so it is a value of
                                     gorio_scan_result.stage only: a refusal of the label stage (index build, clustering) names it */
} gorio_scan_stage;

typedef struct {
  int status;                 /* gorio_scan_status */
  int stage;                  /* gorio_scan_stage the run ended in when status is EMPTY or REFUSED (the stage that left nothing / refused), else -1.
                                 A refusal of REVE itself (bad sample indices) is reported as GATE, the stage whose cloud it reads. */
  int reve_success;           /* what RadarEgoVelocityEstimator::estimate returned */
  double v_r[3], sigma_v_r[3];/* PREP:422-443; zeros when the estimate failed (the reference leaves them unset) */
  int n_out, n_ground, n_clusters;
} gorio_scan_result;

/*
 * PREP:421-568 on the loaded scan, in the callback's order: REVE (sample_idx[n_iter][reve.n_ransac_points] as gorio_prep_ego_velocity
 * takes them), dynamic-object removal, deskew (ang_vel = the IMU's angular velocity, 3 doubles, or NULL = no IMU message, PREP:660-662),
 * distance filter, outlier removal, Patchwork++ with id = 1 (PREP:511), DBSCAN labels.  Returns 0 for the statuses OK, ZERO_VELOCITY
 * and EMPTY and the refusing stage's negative code for REFUSED; GORIO_ERR_STATE without a gorio_scan_load before it.  Every run
 * consumes its load.  The Patchwork++ state advances only when that stage ran.
 */
int gorio_scan_run(gorio_scan_t* h, const unsigned int* sample_idx, int n_iter, const double* ang_vel, gorio_scan_result* result);

/* What the nodelet publishes (PREP:570-579) after a run with status OK: n_out points.  Any pointer may be NULL.  label is normal_x
 * (PREP:566), doppler the curvature field (PREP:407).  stride_bytes between points for every array; capacity in points >= n_out. */
int gorio_scan_get_output(gorio_scan_t* h, float* xyz, float* intensity, float* doppler, float* label, int stride_bytes, int capacity);

/* The survivors of `stage`, in that stage's output order, as indices into the gated cloud (for GORIO_SCAN_STAGE_GATE: into the raw
 * message).  This is what attributes a difference in the output to one stage.  *count receives the size even when capacity is too small
 * (GORIO_ERR_INVALID then); a stage the last run did not reach has count 0; a stage that is switched off reports its input.
 * index_out may be NULL (the count only).  _points: the coordinates the stage put out, 3 floats per point. */
int gorio_scan_get_stage(gorio_scan_t* h, int stage, int* index_out, int capacity, int* count);
int gorio_scan_get_stage_points(gorio_scan_t* h, int stage, float* xyz_out, int capacity, int* count);

/*
 * FastAPDGICP::setInputSource / setInputTarget with the output of the last OK run (points and labels), without a host round trip.
 * The registration handle SHARES the output cloud and the search index the DBSCAN stage built for it (as gorio_apd_set_target_shared
 * shares a target), so the hand-off builds no index; the pipeline starts its next frame in fresh buffers.  The handle is left as
 * gorio_apd_set_source / _target leave it for the same points: covariances stale, correspondences invalid.  Both handles must live on
 * one device.
 * Two limits of the sharing:
 *  - One cloud carries one set of covariances.  Handles that share a scan output (as source or as target) must agree in
 *    k_correspondences and regularization: the hand-off refuses a handle that disagrees with covariances already estimated, and align /
 *    linearize refuse one whose settings differ from those another sharer has estimated them with since (GORIO_ERR_INVALID).
 *  - The shared index was built for the scan alone, with the 2048-point kd chunks of scan-sized clouds.  gorio_apd_set_source followed by
 *    an align against a cloud of more than 131072 points (a large submap) would build the scan's index with 4096-point chunks instead;
 *    the shared one is kept as it is.  Search results and the alignment are the same (the searches are exact); only
 *    gorio_apd_debug_get_index shows the other chunking.  Against scan-sized clouds the two indices are identical.
 */
int gorio_apd_set_source_from_scan(gorio_apd_t* apd, gorio_scan_t* scan);
int gorio_apd_set_target_from_scan(gorio_apd_t* apd, gorio_scan_t* scan);

/* Cumulative since create: point_uploads = copies of point data host -> device (1 per load); index_builds = search indices built
 * (1 per outlier stage that ran, 1 per DBSCAN stage); point_downloads = copies of point data device -> host (gorio_scan_get_output
 * and gorio_scan_get_stage_points: 1 each). */
int gorio_scan_get_counters(const gorio_scan_t* h, long long* point_uploads, long long* index_builds, long long* point_downloads);

const char* gorio_scan_last_error(void);

#ifdef __cplusplus
}
#endif

/* the batched section: N scans through the same stages in lock-step rounds (an extension, not in the reference) */
#include "gorio_scan_batch.h"

#endif /* GORIO_SCAN_H */
