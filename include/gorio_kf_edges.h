/*
 * gorio_kf_edges.h -- the pose-graph edge section of the keyframe store's C ABI (libgorio_amd.so).  include/gorio_keyframes.h includes this
 * file at its end: a user of the store includes that header and has these calls with it.
 *
 * Paths relative to the Go-RIO sources (4DRadarSLAM):
 *   IMC  = src/radar_graph_slam/information_matrix_calculator.cpp    IMCH = include/radar_graph_slam/information_matrix_calculator.hpp
 *   RGS  = apps/radar_graph_slam_nodelet.cpp                         LD   = src/radar_graph_slam/loop_detector.cpp
 *
 * InformationMatrixCalculator::calc_information_matrix (IMC:29-86) is the back end's last reader of keyframe->cloud: once per queued
 * keyframe for the odometry edges (RGS:585-591) and once per accepted loop (LD:315).  Each call there builds a kd-tree over one keyframe,
 * moves the other one by the edge's relative pose and turns the mean squared nearest-neighbour distance into the diagonal of the edge's
 * 6 x 6 information matrix.  Here the two keyframes are named by their ids in the store and any number of edges is scored in one pass.
 *
 * Conventions of include/gorio_keyframes.h: 0 or a negative gorio_status, the text through gorio_kf_last_error (it names edges[e]), every
 * check before any device call and before any state change, a failed call changes nothing, no CPU fallback.
 *
 * THE SCORE is defined by what the library already ships.  Take a fresh registration handle in GORIO_SEARCH_PRUNED mode, give it
 * gorio_apd_set_target_from_keyframe(target_id) and gorio_apd_set_source_from_keyframe(source_id), let Tf be relpose with each entry
 * rounded to float once (relpose.cast<float>(), IMC:63).  score[e] is, bit for bit, the score gorio_apd_fitness_score(h, Tf, max_range,
 * 0, &score, NULL) returns: that call's float transform arithmetic; FLANN L2_Simple float squared distances compared to max_range with
 * <= (IMC:75: max_range is a SQUARED distance); partial sums per 256 source points in original order, added in block order on the host;
 * DBL_MAX when no point is in range (IMC:85).  The inlier statistic of that call is not part of an edge.
 *
 * ONE CALL, whatever count is: one index build for the named keyframes that lack a search index (a keyframe named by many edges is one
 * cloud; the index stays with the keyframe, so every sharer finds it), one staged upload of the edge table, one launch that arms every
 * edge's keys, one exact 1-NN search launch over all edges (the search of the registration), one reduction launch, one device-to-host
 * copy and one stream synchronisation.  The scratch is the store's own, grows and never shrinks, and holds a key array per EDGE: one
 * keyframe may be the source (and the target) of any number of edges of a call, and an edge may name one keyframe on both sides.
 * Untouched: every registration handle, every keyframe's covariances, the three counters of gorio_kf_get_counters (no point column is
 * copied in either direction).
 *
 * Errors (all before any device call):
 *   count == 0                                                                          GORIO_OK, nothing is looked at
 *   null pointer, count < 0, an id never added, a non-finite relpose entry, NaN max_range   GORIO_ERR_INVALID
 *   a released id                                                                       GORIO_ERR_STATE
 *   more than 65535 edges, or more than 2^31 - 1 source points over all edges           GORIO_ERR_UNSUPPORTED
 * An EMPTY keyframe on either side is legal: that edge scores DBL_MAX with n_in_range = 0 and takes no part in the launches.  For an
 * empty source that is the reference's own result.  DEVIATION: for an empty target the reference's kd-tree finds nothing and IMC:75
 * reads the distance the previous query left in nn_dists (0 for the first one); here nothing is in range.  Keyframes with non-finite
 * points behave as gorio_apd_fitness_score does on them.
 */
#ifndef GORIO_KF_EDGES_H
#define GORIO_KF_EDGES_H

#include "gorio_keyframes.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int target_id;      /* cloud1 of IMC:55: the cloud that gets the kd-tree */
  int source_id;      /* cloud2: the cloud moved by relpose */
  double relpose[16]; /* row-major; rows 0..2 are used, each entry rounded to float once (IMC:63) */
} gorio_kf_edge;

/* calc_fitness_score (IMC:55-86) for `count` edges in one pass.  max_range: IMC's max_range (a squared distance; DBL_MAX = no limit).
 * score[count]; n_in_range[count] (nr of IMC:78) may be NULL. */
int gorio_kf_edge_fitness(gorio_kf_t* kf, const gorio_kf_edge* edges, int count, double max_range, double* score, long long* n_in_range);

typedef struct {
  int use_const_inf_matrix;
  double const_stddev_x, const_stddev_q, var_gain_a, min_stddev_x, max_stddev_x, min_stddev_q, max_stddev_q, fitness_score_thresh;
} gorio_inf_params;
/* The defaults of the CONSTRUCTOR (IMC:15-24), which is what the nodelet uses (RGS:114): false, 0.5, 0.1, 20, 0.1, 5, 0.05, 0.2 and
 * fitness_score_thresh = 0.5.  (The unused load() of IMCH:21-32 says 2.5.) */
void gorio_kf_default_inf_params(gorio_inf_params* p);

/*
 * calc_information_matrix (IMC:29-53) for `count` edges: inf_diag[2 e] = 1 / w_x (the three translation entries of the diagonal),
 * inf_diag[2 e + 1] = 1 / w_q (the three rotation entries).  The score is gorio_kf_edge_fitness with max_range = DBL_MAX (IMC:37); the
 * rest is host arithmetic that restates IMC:39-49: min / max variances by std::pow(., 2), weight() (IMCH:39-42) in double, w_x and w_q
 * rounded to float (IMC:44-45), the outputs 1.0 / (double)w.  A DBL_MAX score goes through weight() unchanged (exp(-a x) is 0).
 * score[count] may be NULL.  With use_const_inf_matrix the outputs are 1 / const_stddev_x and 1 / const_stddev_q (NOT squared, as in
 * IMC:32-33), no device call is made, edges is not read (ids are not looked at, as there) and score is not written.
 * The caller overwrites (5, 5) with 1.0 for odometry edges (RGS:591).
 */
int gorio_kf_edge_information(gorio_kf_t* kf, const gorio_inf_params* p, const gorio_kf_edge* edges, int count, double* inf_diag, double* score);

/* Cumulative since create, over the calls that reached the device: calls; edges_scored (empty-keyframe edges included); index_builds =
 * keyframes whose search index one of these calls built; synchronisations = stream synchronisations (one per call).  Any pointer may be NULL. */
int gorio_kf_edge_counters(const gorio_kf_t* kf, long long* calls, long long* edges_scored, long long* index_builds, long long* synchronisations);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_KF_EDGES_H */
