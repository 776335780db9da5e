/*
 * gorio_ground.h -- C ABI of Patchwork++ ground segmentation on the MI355X (libgorio_amd.so), the stage the preprocessing nodelet
 * runs between the outlier filter and the DBSCAN labels (PREP:505-519).
 *
 * Paths relative to the Go-RIO sources:
 *   PREP = apps/preprocessing_nodelet_ntu.cpp      PWP = include/patchworkpp/patchworkpp.hpp
 *
 * Same conventions as include/gorio_prep.h: plain pointers, host pointers caller-owned and only read / written during the call,
 * 0 on success or a negative gorio_status (include/gorio_apd.h), gorio_ground_last_error() gives the text (thread-local).  No CPU
 * fallback: without a HIP device the calls fail with GORIO_ERR_NO_DEVICE.
 *
 * A segmenter keeps the reference's state across frames (adaptive elevation / flatness thresholds, their storages, the sensor height
 * that A-GLE re-estimates), so it is a handle.  One handle must not be used from two threads at once.
 */
#ifndef GORIO_GROUND_H
#define GORIO_GROUND_H

#ifdef __cplusplus
extern "C" {
#endif

#define GORIO_GROUND_RINGS_OF_INTEREST 4 /* elevation_thr / flatness_thr have 4 entries (PWP:165-166, num_rings_of_interest_ = their size) */
#define GORIO_GROUND_MAX_FITS 9          /* 1 + num_iter plane fits per patch; num_iter in [1, 8] */

/* Patchwork++ Params (PWP:86-168).  gorio_ground_default_params gives Params() with verbose = false, as the nodelet uses it
 * (PREP:100-102).  enable_RVPF = 1 is refused (GORIO_ERR_INVALID): it is off in the reference and in every caller. */
typedef struct {
  int enable_RNR, enable_RVPF, enable_TGR;
  int num_iter, num_lpr, num_min_pts;
  double RNR_ver_angle_thr, RNR_intensity_thr;
  double sensor_height, th_seeds, th_dist, th_seeds_v, th_dist_v, max_range, min_range, uprightness_thr, adaptive_seed_selection_margin;
  int num_sectors_each_zone[4], num_rings_each_zone[4]; /* num_zones is 4 (the reference throws otherwise, PWP:221-223) */
  int max_flatness_storage, max_elevation_storage;
  double elevation_thr[GORIO_GROUND_RINGS_OF_INTEREST], flatness_thr[GORIO_GROUND_RINGS_OF_INTEREST];
} gorio_ground_params;

typedef struct gorio_ground gorio_ground_t;

void gorio_ground_default_params(gorio_ground_params* p);
/* Up to 512 patches (sum over zones of sectors x rings); min_range < max_range; num_iter in [1, 8]; num_min_pts >= 1.
 * num_lpr >= 1 and th_seeds > 0: then every fitted patch has at least one seed.  With num_lpr = 0 the reference's LPR height is 0
 * (PWP:646) and a patch above th_seeds has no seeds; its first plane fit then reads pc_mean_ / cov_ of the previous patch, which
 * the per-patch kernels do not carry, so such parameters are refused (GORIO_ERR_INVALID). */
int gorio_ground_create(gorio_ground_t** out, int device, const gorio_ground_params* p);
void gorio_ground_destroy(gorio_ground_t* h);

/*
 * PatchWorkpp::estimate_ground(cloud_in, ego_vel, cloud_ground, cloud_nonground, time_taken, id) (PWP:684-890).  ego_vel is unused
 * by the reference (PWP:761, 784 are commented out) and so is not an argument here.
 *   xyz / intensity   first x and first intensity of the scan; stride_bytes between points (48 for pcl::PointXYZINormal)
 *   id                0: estimate_plane (SVD only), 1: estimate_plane_cov (SVD + the LM plane fit), as the nodelet (PREP:511)
 *   order_out         n ints: indices into the input of cloud_ground ++ cloud_nonground, in the reference's order
 *   n_ground, n_out   sizes; n_out <= n because the under-ground pass erases points (PWP:872-884)
 * Every coordinate must be finite (std::sort on a NaN height is undefined in the reference).  n >= 1.
 */
int gorio_ground_estimate(gorio_ground_t* h, const float* xyz, const float* intensity, int n, int stride_bytes, int id, int* order_out, int* n_ground, int* n_out);

/* The same for `count` independent segmenters in one launch over all their patches: arrays of per-handle arguments.  All handles on
 * one device, each at most once.  On a validation error no handle is changed and the error names the index. */
int gorio_ground_estimate_batch(gorio_ground_t* const* handles, int count, const float* const* xyz, const float* const* intensity, const int* n, const int* stride_bytes,
                                int id, int* const* order_out, int* n_ground, int* n_out);

/* Adaptive state: elevation_thr_[4], flatness_thr_[4], sensor_height_, update_elevation_[4] and update_flatness_[4] (PWP:380-381).
 * Storages are [4][storage_stride] row-major with *_count[r] valid values in row r.  get: any pointer may be NULL; a row longer
 * than storage_stride fails with GORIO_ERR_INVALID (the counts are still written).  set: counts in [0, storage_stride]. */
int gorio_ground_get_state(const gorio_ground_t* h, double elevation_thr[4], double flatness_thr[4], double* sensor_height, double* elevation_storage,
                           int elevation_count[4], double* flatness_storage, int flatness_count[4], int storage_stride);
int gorio_ground_set_state(gorio_ground_t* h, const double elevation_thr[4], const double flatness_thr[4], double sensor_height, const double* elevation_storage,
                           const int elevation_count[4], const double* flatness_storage, const int flatness_count[4], int storage_stride);

/* What the five-way decision (PWP:792-822) and TGR (PWP:952-1018) did with a patch's regionwise ground. */
typedef enum {
  GORIO_GROUND_SKIPPED = 0,       /* fewer than num_min_pts points: all non-ground, unsorted */
  GORIO_GROUND_NOT_UPRIGHT = 1,   /* non-ground */
  GORIO_GROUND_FAR = 2,           /* outside the rings of interest: ground */
  GORIO_GROUND_HEADING = 3,       /* heading >= 0: non-ground */
  GORIO_GROUND_FLAT = 4,          /* not elevated, or flat: ground */
  GORIO_GROUND_TGR_REVERT = 5,    /* TGR candidate reverted to ground */
  GORIO_GROUND_TGR_REJECT = 6     /* TGR candidate kept non-ground */
} gorio_ground_decision;

typedef struct {
  int zone, ring, sector, concentric_idx;
  int n_points;        /* binned into the patch */
  int segment_offset;  /* where the patch's points start in patch_order (gorio_ground_get_diagnostics) */
  int n_ground;        /* regionwise_ground size */
  int decision;        /* gorio_ground_decision */
  double uprightness, elevation, flatness, line_variable, heading;
  float mean[3], cov[9], singular_values[3], normal[3], d; /* pc_mean_, cov_, singular_values_, normal_, d_ after the last fit */
  int n_fits;                                   /* 1 + num_iter, 0 when skipped */
  int fit_points[GORIO_GROUND_MAX_FITS];        /* points in each plane fit */
  int lm_iterations[GORIO_GROUND_MAX_FITS];     /* LM iterations of each fit (0 with id = 0 or an empty fit) */
  int lm_termination[GORIO_GROUND_MAX_FITS];    /* 0 none, 1 function tol, 2 parameter tol, 3 gradient tol, 4 max iterations, 5 radius */
} gorio_ground_patch_diag;

typedef struct {
  int n_points, n_noise, n_out_of_range, n_patches, n_ground, n_erased;
  int final_fit_points, final_lm_iterations, final_lm_termination;
  float final_mean[3], final_cov[9], final_singular_values[3], final_normal[3], final_d; /* the plane of the under-ground pass */
} gorio_ground_frame_diag;

/* Diagnostics of the handle's last estimate.  Any pointer may be NULL.
 *   patches        patch_capacity entries, patch id order (zone, then ring, then sector)
 *   point_label    n_points ints: -2 RNR noise, -1 outside (min_range, max_range], otherwise the patch id
 *   patch_order    n_points ints: the patches' points, patch after patch from segment_offset: sorted by (z, input index) for fitted
 *                  patches, in input order for skipped ones; the entries past the last patch are -1 */
int gorio_ground_get_diagnostics(const gorio_ground_t* h, gorio_ground_frame_diag* frame, gorio_ground_patch_diag* patches, int patch_capacity, int* point_label,
                                 int* patch_order, int n_points);

const char* gorio_ground_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_GROUND_H */
