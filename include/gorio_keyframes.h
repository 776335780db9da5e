/*
 * gorio_keyframes.h -- C ABI of the keyframe store on the MI355X (libgorio_amd.so): the place where a keyframe's cloud LIVES on the
 * device under a stable id, and the entry points through which the registration handles (include/gorio_apd.h), NDT (include/gorio_ndt.h)
 * and the Scan Context database (include/gorio_sc.h) take a keyframe by that id instead of by host pointers.
 *
 * Paths relative to the Go-RIO sources (4DRadarSLAM):
 *   SMO = apps/scan_matching_odometry_nodelet.cpp    RGS = apps/radar_graph_slam_nodelet.cpp    LD = src/radar_graph_slam/loop_detector.cpp
 *
 * In the reference a keyframe is a pcl::PointCloud on the host, and every user of it copies it again: the scan-to-submap target
 * (SMO:602-618), the keyframe's Scan Context descriptor (RGS:727-731), loop-closure verification (LD:222-236, 391-422) and the next
 * scan-to-scan target (SMO:588).  Here the front end keeps a scan on the device from the raw message to the registration handle
 * (include/gorio_scan.h); this store carries it on from there.
 *
 * Same conventions as include/gorio_scan.h: plain pointers, host pointers caller-owned and only read / written during the call, 0 on
 * success or a negative gorio_status (include/gorio_apd.h), gorio_kf_last_error gives the text (thread-local; the consumers below that
 * belong to another handle type report through that type's own last-error call).  No CPU fallback: gorio_kf_create only checks and stores
 * its arguments; the first call that needs the device fails with GORIO_ERR_NO_DEVICE without a HIP device.  Argument and state errors
 * are reported before any device call, and a failed call changes nothing.  One store must not be used from two threads at once.
 *
 * A keyframe is one device cloud (points, labels, and whatever has been derived from them: covariances with the (k_correspondences,
 * regularization) they were estimated with, search index, voxel map), an optional intensity column of its own, and its point count.
 * Ids are 0, 1, 2, ... in order of addition and are never reused.
 *
 * Sharing.  A registration handle that is given a keyframe SHARES its device cloud, as gorio_apd_set_target_shared shares a target:
 *  - what one sharer derives (covariances, search index, voxel map) every other sharer finds; that is the point of the store: the
 *    keyframe that was the source of the align that made it becomes the next target with its covariances and index in place;
 *  - one cloud carries one set of covariances: sharers must agree in k_correspondences / regularization (GORIO_ERR_INVALID otherwise,
 *    at the hand-off for covariances that exist, at align / linearize for ones another sharer has estimated since), and in VGICP mode in
 *    voxel_resolution / voxel_mode;
 *  - gorio_apd_set_source_covariances / _set_target_covariances on a handle that shares a keyframe writes the shared cloud: EVERY sharer,
 *    and the store, sees the new covariances (as include/gorio_apd.h says of shared targets);
 *  - gorio_apd_set_source / _set_target (new points) detach the handle from the keyframe first; the keyframe is never overwritten.
 * gorio_kf_release and gorio_kf_destroy only drop the STORE's share: handles that were given the keyframe keep it alive and keep
 * registering against it, as a registration handle keeps a scan after its pipeline is destroyed.
 */
#ifndef GORIO_KEYFRAMES_H
#define GORIO_KEYFRAMES_H

#include "gorio_apd.h"
#include "gorio_ndt.h"
#include "gorio_sc.h"
#include "gorio_scan.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gorio_kf gorio_kf_t;

/* The keyframe containers of the nodelets (keyframes of SMO:94-96 / RGS:1040-1050: std::vector / std::deque of clouds).  Only checks
 * and stores its arguments (device >= 0). */
int gorio_kf_create(gorio_kf_t** out, int device);
/* Drops the store's share of every keyframe (see "Sharing" above). */
void gorio_kf_destroy(gorio_kf_t* kf);

/*
 * keyframe_cloud = filtered (SMO:481, 586; RGS:484 `cloud` of a KeyFrame) from host memory.  The cloud is held exactly as
 * gorio_apd_set_source holds the same arguments (same upload routine: non-finite points are stored as given, nothing derived yet).
 *   xyz / intensity / label   first x / intensity / label (normal_x); stride_bytes between points for all three (a multiple of 4, >= 12).
 *                             intensity and label may be NULL (no intensity column; labels 0).
 *   n                         may be 0: an empty keyframe (every consumer treats it as its host entry point treats an empty cloud)
 *   id                        receives the new id
 */
int gorio_kf_add(gorio_kf_t* kf, const float* xyz, const float* intensity, const float* label, int n, int stride_bytes, int* id);

/*
 * The same (SMO:481, 586) with the output of the pipeline's last OK run (include/gorio_scan.h): the store SHARES the pipeline's output
 * cloud -- the one gorio_apd_set_source_from_scan shares, with the search index the DBSCAN stage built -- so no point is copied.  Only
 * the intensity column is copied, device to device and ordered behind the pipeline's stream: the pipeline reuses its stage buffers for
 * the next frame.  GORIO_ERR_STATE without an output; the pipeline's counters do not move.
 */
int gorio_kf_add_from_scan(gorio_kf_t* kf, gorio_scan_t* scan, int* id);

/*
 * SMO:586-588: the cloud a registration handle holds NOW as its source (which = 0) or target (which = 1) becomes a keyframe, shared with
 * everything it carries: covariances with their (k, regularization), search index, voxel map.  After an align the source carries the
 * k-NN covariances and the index that align made, so gorio_apd_set_target_from_keyframe of that id replaces the reference's
 * setInputTarget(keyframe) without estimating either again.  intensity: host, n floats at intensity_stride_bytes (a multiple of 4),
 * or NULL.  GORIO_ERR_STATE without a cloud on that side.
 */
int gorio_kf_add_from_apd(gorio_kf_t* kf, gorio_apd_t* apd, int which, const float* intensity, int intensity_stride_bytes, int* id);

/* keyframes.pop_front() / a KeyFrame::Ptr going out of scope (SMO:596-599): the store lets go of that keyframe's device memory.  The id
 * stays taken: every later call with it returns GORIO_ERR_STATE.  GORIO_ERR_INVALID for an id never added. */
int gorio_kf_release(gorio_kf_t* kf, int id);
/* keyframes.size(): ids handed out so far, and how many of them the store still holds.  Either pointer may be NULL. */
int gorio_kf_count(const gorio_kf_t* kf, int* n_added, int* n_resident);

typedef struct {
  int n;             /* points */
  int resident;      /* 0 after gorio_kf_release (every other field is 0 then) */
  int has_intensity;
  int cov_count;     /* n when the cloud carries valid covariances, else 0 (source_covs_.size(), fast_apdgicp.hpp) */
  int cov_k, cov_reg;/* k_correspondences / regularization they were estimated with; -1: supplied through gorio_apd_set_*_covariances */
  int index_built;   /* the search index of the pruned searches is valid */
  int sharers;       /* holders of the device cloud besides the store (registration handles, a scan pipeline) */
} gorio_kf_info_t;
/* What a keyframe carries right now (no device call).  A released id gives GORIO_OK with resident = 0; an id never added GORIO_ERR_INVALID. */
int gorio_kf_info(const gorio_kf_t* kf, int id, gorio_kf_info_t* out);

/* keyframe->cloud read back (RGS:727 `keyframe->cloud`): any of xyz / intensity / label may be NULL; stride_bytes between points for all
 * arrays (a multiple of 4; >= 12 with xyz); capacity in points >= n.  intensity of a keyframe without that column: GORIO_ERR_STATE. */
int gorio_kf_get(gorio_kf_t* kf, int id, float* xyz, float* intensity, float* label, int stride_bytes, int capacity);

/* Cumulative since create, one per successful call: point_uploads = keyframes whose points came from the host (gorio_kf_add);
 * point_downloads = gorio_kf_get; device_copies = device-to-device copies of point columns (the intensity column of
 * gorio_kf_add_from_scan, x / y / z of gorio_ndt_set_*_from_keyframe, the packed scans of gorio_sc_add_keyframes).  Sharing a keyframe
 * with a registration handle and assembling a submap from keyframes move none of them. */
int gorio_kf_get_counters(const gorio_kf_t* kf, long long* point_uploads, long long* point_downloads, long long* device_copies);

const char* gorio_kf_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------- consumers */

/*
 * registration->setInputSource(keyframe) / setInputTarget(keyframe) -- SMO:588 (the next scan-to-scan target), LD:222 and LD:391 (the
 * new keyframe against each loop candidate) -- as a pointer share, for all three methods (APD-GICP, GICP, VGICP), with exactly the checks
 * of gorio_apd_set_target_shared: GORIO_ERR_INVALID for covariances estimated with another k_correspondences / regularization than this
 * handle's, and in VGICP mode for a voxel map built with other voxel settings; GORIO_ERR_INVALID for an empty keyframe (as n <= 0 in
 * gorio_apd_set_source) and for a store on another device; GORIO_ERR_STATE for a released id.  The handle is left as gorio_apd_set_source
 * / _set_target leave it for the same points (correspondences invalid), EXCEPT that valid covariances, search index and voxel map stay
 * valid.  Errors: gorio_apd_last_error of that handle.
 */
int gorio_apd_set_source_from_keyframe(gorio_apd_t* apd, gorio_kf_t* kf, int id);
int gorio_apd_set_target_from_keyframe(gorio_apd_t* apd, gorio_kf_t* kf, int id);

/*
 * The same for pclomp::NormalDistributionsTransform (LD:222, 391 with registration_method NDT_OMP).  NDT keeps SoA clouds of its own and
 * wants neither labels nor an index: these COPY x, y, z on the device (as gorio_ndt_set_source_from_scan does) and count one in
 * device_copies.  A source with a non-finite point is refused as there.  Errors: gorio_ndt_last_error.
 */
int gorio_ndt_set_source_from_keyframe(gorio_ndt_t* ndt, gorio_kf_t* kf, int id);
int gorio_ndt_set_target_from_keyframe(gorio_ndt_t* ndt, gorio_kf_t* kf, int id);

/*
 * SMO:602-618 from resident keyframes: gorio_apd_set_target_submap without the host staging and the upload.  ids[count] in the order the
 * frames are concatenated, rel_poses[count][16] row-major double (odom_i^-1 * odom_newest; rows 0..2 are used).  The assembled target is
 * bit for bit the one gorio_apd_set_target_submap assembles from host copies of the same keyframes: frames in the order given, points in
 * their own order, non-finite points skipped, empty frames contributing nothing, "no finite point in any keyframe" GORIO_ERR_INVALID,
 * and from the voxel_leaf > 0 branch on the same code.  On the device: per 256-point block of every frame the finite points are counted
 * (ballot + popcount), one exclusive scan over all block counts, then one pass writes each finite point, transformed in double (the four
 * products summed left to right, rounded to float once), at its rank.  The total comes back in one 4-byte copy.  A keyframe may be listed
 * more than once.  Errors: gorio_apd_last_error of that handle.
 */
int gorio_apd_set_target_submap_keyframes(gorio_apd_t* apd, gorio_kf_t* kf, const int* ids, const double* rel_poses, int count, double voxel_leaf, int* n_target);

/*
 * scManager.makeAndSaveScancontextAndKeys(*keyframe->cloud) (RGS:727-731) for the listed keyframes, in order: a pack kernel writes
 * (x, y, intensity, 0) and the scan offsets into the layout gorio_sc_add_scans uploads, then the same descriptor kernel runs.
 * Descriptors, ring keys and sector keys equal those of gorio_sc_add_scans on host copies bit for bit.  A keyframe without an intensity
 * column gives GORIO_ERR_STATE (nothing is added); an empty keyframe is an empty scan, as there.  Errors: gorio_sc_last_error.
 */
int gorio_sc_add_keyframes(gorio_sc_t* sc, gorio_kf_t* kf, const int* ids, int count, int* first_index_out);

#ifdef __cplusplus
}
#endif

/* Pose-graph edges between resident keyframes (InformationMatrixCalculator of the back end): fitness score and information matrix of
 * any number of edges in one pass.  Part of this ABI, kept in a file of its own. */
#include "gorio_kf_edges.h"

#endif /* GORIO_KEYFRAMES_H */
