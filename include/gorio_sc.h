/*
 * gorio_sc.h -- C ABI of the Intensity Scan Context loop-candidate search on the MI355X (libgorio_amd.so): SCManager, the stage of
 * LoopDetector that picks which keyframe to verify (LD:192-236) and whose descriptor the back end makes for every keyframe
 * (RGS:727-731).
 *
 * Paths relative to the Go-RIO sources:
 *   SC  = src/radar_graph_slam/Scancontext.cpp        SCH = include/scan_context/Scancontext.h
 *   LD  = src/radar_graph_slam/loop_detector.cpp      NF  = include/scan_context/nanoflann.hpp (v1.3.2)
 *   RGS = apps/radar_graph_slam_nodelet.cpp
 *
 * Same conventions as include/gorio_ground.h: plain pointers, host pointers caller-owned and only read / written during the call,
 * 0 on success or a negative gorio_status (include/gorio_apd.h), gorio_sc_last_error() gives the text (thread-local).  No CPU
 * fallback: without a HIP device gorio_sc_create fails with GORIO_ERR_NO_DEVICE, so no other call can run.  Arguments are checked
 * before any state changes; a refused call leaves the handle as it was.
 *
 * The handle is the SCManager: the keyframe database (descriptor, ring key, sector key per added scan, index = order of addition),
 * the tree-making counter and the tree snapshot.  One handle must not be used from two threads at once.
 *
 * Fixed as in the reference (const members, SCH:111-129): 40 rings, 20 sectors, max radius 80 m, NUM_EXCLUDE_RECENT 10,
 * NUM_CANDIDATES_FROM_TREE 3, SEARCH_RATIO 0.1 (so the search radius is round(0.5 * 0.1 * 20) = 1 shift), TREE_MAKING_PERIOD_ 10.
 *
 * What is pinned, and what is assumed:
 *   - atan2f is taken to be correctly rounded: computed as float(atan2(double x, double y)).  The rest of the azimuth is in double
 *     as SC:185 writes it, stored as float.
 *   - abs(azim_angle) (SC:187) is taken to be the float overload that libstdc++'s <math.h> puts in the global namespace.  Were it
 *     int abs(int), points with |azimuth| in (range, floor(range) + 1) would be kept.
 *   - Eigen's reduction order (mean, norm, dot) is not pinned by the reference; every sum here runs in index order.
 *   - A NaN x or y passes both skip tests (SC:187-191); x86's float-to-int conversion then gives INT_MIN, which clamps to 1, so the
 *     point lands in bin (ring 1, sector 1).  This is reproduced explicitly.  An infinite range is skipped.
 *   - The kd-tree's order among exactly equal key distances is not reproducible; here ties go to the lower snapshot position.
 *   - Keys whose float distance to the query is not below FLT_MAX (inf, NaN) never enter the k-NN result, as NF:1358-1361 has it.
 */
#ifndef GORIO_SC_H
#define GORIO_SC_H

#ifdef __cplusplus
extern "C" {
#endif

#define GORIO_SC_RINGS 40            /* PC_NUM_RING (SCH:112) */
#define GORIO_SC_SECTORS 20          /* PC_NUM_SECTOR (SCH:113) */
#define GORIO_SC_MAX_RADIUS 80.0     /* PC_MAX_RADIUS (SCH:114) */
#define GORIO_SC_EXCLUDE_RECENT 10   /* NUM_EXCLUDE_RECENT (SCH:119) */
#define GORIO_SC_CANDIDATES 3        /* NUM_CANDIDATES_FROM_TREE (SCH:120) */
#define GORIO_SC_TREE_PERIOD 10      /* TREE_MAKING_PERIOD_ (SCH:129) */

/* The two values LoopDetector sets (LD:69-70, 88-89).  gorio_sc_default_params gives what every launch file sets: 0.5 and 56.5.
 * The nodelet's own fallbacks, used when a launch file omits them, are 0.3 and 0.3.  setAzimuthRange makes the range symmetric
 * (SC:69-73), so the in-class -56.6 (SCH:111) never survives LoopDetector.  azimuth_range must be finite and > 0. */
typedef struct {
  double sc_dist_thresh;  /* setScDistThresh: SC_DIST_THRES */
  double azimuth_range;   /* setAzimuthRange: PC_AZIMUTH_ANGLE_MAX = range, MIN = -range, UNIT_SECTOR_ANGLE = 2 range / 20 */
} gorio_sc_params;

/* What one detectLoopClosureID call (SC:272-373) did. */
typedef struct {
  int early_return;    /* (int)index < NUM_EXCLUDE_RECENT (SC:284-288): nothing below is set, the counter is unchanged */
  int rebuilt;         /* counter % TREE_MAKING_PERIOD_ == 0: the snapshot was rebuilt from this call's candidates (SC:294-306) */
  int counter;         /* tree_making_period_conter after the call */
  int snapshot_size;   /* polarcontext_invkeys_to_search_.size() seen by the k-NN */
  int n_found;         /* entries the k-NN delivered, min(3, snapshot entries with a distance below FLT_MAX) */
  int position[GORIO_SC_CANDIDATES];    /* knn_candidate_indexes: ascending key distance; 0 where nothing was found (zero-initialised) */
  float key_dist[GORIO_SC_CANDIDATES];  /* out_dists_sqr: squared float distances; unfound entries keep 0, the last FLT_MAX (NF:158-163) */
  int keyframe[GORIO_SC_CANDIDATES];    /* candidate_keyframe_indices[position] of the CURRENT call, -1 where position > size - 1 (SC:332) */
  double sc_dist[GORIO_SC_CANDIDATES];  /* distanceBtnScanContext of (query, keyframe); NaN where skipped */
  int sc_shift[GORIO_SC_CANDIDATES];    /* its argmin shift; -1 where skipped */
} gorio_sc_diag;

typedef struct gorio_sc gorio_sc_t;

void gorio_sc_default_params(gorio_sc_params* p);
/* new SCManager() + setScDistThresh + setAzimuthRange (LD:88-89). */
int gorio_sc_create(gorio_sc_t** out, int device, const gorio_sc_params* p);
void gorio_sc_destroy(gorio_sc_t* h);

/*
 * makeAndSaveScancontextAndKeys (SC:255-269) for `count` keyframes, in order, in one upload and one launch.  The database index of
 * scan k is *first_index_out + k.  Per scan: xyz / intensity point at the first x and the first intensity, stride_bytes between
 * points (48 for pcl::PointXYZINormal, a multiple of 4 and >= 12), n >= 0 points (an empty scan gives an all-zero descriptor).
 * Any float value is accepted: NaN / Inf coordinates and NaN intensities follow the reference (see above).
 */
int gorio_sc_add_scans(gorio_sc_t* h, int count, const float* const* xyz, const float* const* intensity, const int* n, const int* stride_bytes, int* first_index_out);

/* Number of scans added so far, the tree-making counter, and the snapshot as database indices in snapshot position order
 * (snapshot may be NULL; otherwise capacity must be >= *snapshot_size). */
int gorio_sc_get_state(const gorio_sc_t* h, int* n_scans, int* counter, int* snapshot_size, int* snapshot, int capacity);

/* polarcontexts_[index] (40 x 20, row-major: desc[ring * 20 + sector]), polarcontext_invkeys_[index] (ring key, 40) and
 * polarcontext_vkeys_[index] (sector key, 20) -- getConstRefRecentSCD is index = n_scans - 1.  Any output may be NULL. */
int gorio_sc_get_descriptor(const gorio_sc_t* h, int index, double* desc, double* ring_key, double* sector_key);

/* distanceBtnScanContext(polarcontexts_[i], polarcontexts_[j]) (SC:127-160): (1e7, 0) when no shift has an effective column. */
int gorio_sc_distance(gorio_sc_t* h, int i, int j, double* dist, int* shift);

/*
 * detectLoopClosureID(candidate_keyframes, new_keyframe) (SC:272-373) with new_keyframe->index = query_index and the candidates'
 * indices in order.  loop_id: the matched keyframe or -1; yaw_rad: deg2rad(float(nn_align * unit_sector_angle)), returned even when
 * there is no loop (0 on the early return); min_dist: the smallest SC distance (1e7 when none was computed or on the early return).
 * diag may be NULL.  An empty candidate list is refused with GORIO_ERR_INVALID (the reference would index out of bounds there;
 * LoopDetector never calls it so, LD:195-197), as are indices that were not added.
 */
int gorio_sc_detect(gorio_sc_t* h, int query_index, const int* candidates, int n_candidates, int* loop_id, float* yaw_rad, double* min_dist, gorio_sc_diag* diag);

/* The same as `count` gorio_sc_detect calls in order, the counter and snapshot included, in one device pass: the snapshot each
 * query sees is worked out on the host from the inputs (keys never change once added).  Outputs are arrays of `count`; diag may
 * be NULL.  On a validation error nothing changes and the error names the query. */
int gorio_sc_detect_batch(gorio_sc_t* h, int count, const int* query_index, const int* const* candidates, const int* n_candidates, int* loop_id, float* yaw_rad,
                          double* min_dist, gorio_sc_diag* diag);

const char* gorio_sc_last_error(void);

#ifdef __cplusplus
}
#endif

/* the exhaustive section: listed pairs, matrices, best matches and the detect without the tree (an extension, not in the reference) */
#include "gorio_sc_pairs.h"
/* the cross-database section: the same calls between two handles, and the K best matches per keyframe (an extension as well) */
#include "gorio_sc_cross.h"

#endif /* GORIO_SC_H */
