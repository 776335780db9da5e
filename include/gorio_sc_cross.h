/*
 * gorio_sc_cross.h -- the cross-database section of the Scan Context C ABI (libgorio_amd.so): the calls of gorio_sc_pairs.h between TWO
 * handles, and the K best matches per keyframe.  include/gorio_sc.h includes this header after gorio_sc_pairs.h; the handle, the status
 * codes, gorio_sc_last_error and the conventions are those of gorio_sc.h.
 *
 * An EXTENSION with no counterpart in the Go-RIO sources, like gorio_sc_pairs.h: the reference holds one SCManager per run and verifies
 * the NUM_CANDIDATES_FROM_TREE = 3 tree picks of a query (SC:294-348).  These calls match the keyframes of one session (the query handle
 * Q) against the database of another (the database handle D), and keep up to GORIO_SC_TOP_MAX matches per keyframe.  What they keep of
 * the reference: the distance itself (distanceBtnScanContext, SC:127-160), and in gorio_sc_cross_detect the strict minimum in list order
 * (SC:341-348), the threshold and the yaw (SC:354-371).
 *
 * dx(q, c) below is distanceBtnScanContext(Q.polarcontexts_[q], D.polarcontexts_[c]) with q the unshifted side; it is not symmetric.  It
 * has, by definition, the bits gorio_sc_distance(M, q', c') gives on any handle M that holds both descriptors, (1e7, 0) included when no
 * shift has an effective column; with Q == D (which is legal) it is gorio_sc_distance(Q, q, c).  All of these calls run the one per-pair
 * device function of gorio_sc_distance.
 *
 * The two handles: work runs on Q's stream and in Q's scratch buffers and counts in Q's cross counters.  D is only read: its tree-making
 * counter, snapshot, gorio_sc_pairs_counters and cross counters do not move, and neither do Q's tree-making counter, snapshot and
 * gorio_sc_pairs_counters.  gorio_sc_add_scans and gorio_sc_add_keyframes synchronise before they return, so everything added to D before
 * the call is visible to it.  Neither handle may be in use by another thread during the call.
 *
 * Refused with GORIO_ERR_INVALID: a null handle; handles on different devices; Q.azimuth_range != D.azimuth_range (the descriptors are not
 * comparable; the text names both values); an index that was not added (the text says whether it is a query-handle or a database-handle
 * index and gives that handle's scan count).  sc_dist_thresh may differ between the handles; decisions use Q's.
 *
 * Conventions, those of gorio_sc_pairs.h: every check happens before any device call and before any state change, a refused call changes
 * nothing and writes nothing, the text names the offending entry, count == 0 (or an empty extent) returns GORIO_OK and touches nothing.
 * Each call that computes uses one upload, a launch count that does not depend on the extents, one copy back per output array and ONE
 * stream synchronisation; results are deterministic (no floating-point atomics, no waits between workgroups).
 */
#ifndef GORIO_SC_CROSS_H
#define GORIO_SC_CROSS_H

#ifdef __cplusplus
extern "C" {
#endif

/* The most matches per row gorio_sc_cross_top_matches keeps. */
#define GORIO_SC_TOP_MAX 8

/* dist[k], shift[k] = dx(q[k], c[k]) for k < count.  One launch. */
int gorio_sc_cross_distance_pairs(gorio_sc_t* Q, gorio_sc_t* D, const int* q, const int* c, int count, double* dist, int* shift);

/* dist[i * n_cols + j], shift[i * n_cols + j] = dx(rows[i], cols[j]).  rows NULL means 0 .. Q.n_scans - 1, cols NULL means
 * 0 .. D.n_scans - 1 (the extent must then be that count).  Either output may be NULL (not both).  Indices may repeat.
 * n_rows * n_cols > 2^31 - 1: GORIO_ERR_UNSUPPORTED, before anything is allocated.  One launch. */
int gorio_sc_cross_distance_matrix(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* cols, int n_cols, double* dist, int* shift);

/* The mining primitive.  For row i (r = rows[i], NULL: i) let e_i = col_end ? col_end[i] : D.n_scans (0 <= e_i <= D.n_scans, else
 * GORIO_ERR_INVALID naming col_end[i]).  The slots index / dist / shift [i * k + 0 .. k - 1] receive, in ascending lexicographic (d, c)
 * order -- d compared as a double, ties to the lower c -- the k smallest of { (dx(r, c), c) : 0 <= c < e_i, dx(r, c) < 1e7 }; slots
 * beyond what exists hold (-1, 1e7, 0).  1 <= k <= GORIO_SC_TOP_MAX (k < 1: GORIO_ERR_INVALID, k > GORIO_SC_TOP_MAX:
 * GORIO_ERR_UNSUPPORTED).  shift may be NULL.  The matrix is never materialised: column tiles are folded into a running k-list per row
 * on the device, only n_rows * k results come down, device memory is O(n_rows * k * runs + tile).  Two launches.
 * With Q == D, k = 1 and col_end[i] = max(0, rows[i] - min_gap + 1) the result is that of gorio_sc_best_matches. */
int gorio_sc_cross_top_matches(gorio_sc_t* Q, const int* rows, int n_rows, gorio_sc_t* D, const int* col_end, int k, int* index, double* dist, int* shift);

/* For `count` queries of Q, each with its own list of D indices: the strict minimum from 1e7 of dx(query, c) in LIST order (SC:341-348);
 * loop_id = that c if min_dist < Q.sc_dist_thresh else -1; yaw_rad from the shift exactly as gorio_sc_detect_exhaustive computes it (the
 * yaw of shift 0 when nothing scored below 1e7); min_dist.  There is NO early return for query < NUM_EXCLUDE_RECENT and NO
 * recent-keyframe filter: the indices of two sessions are unrelated (with Q == D the caller filters, or calls
 * gorio_sc_detect_exhaustive).  An empty list: GORIO_ERR_INVALID naming the query.  More than 2^31 - 1 candidates in all:
 * GORIO_ERR_UNSUPPORTED.  Two launches: the pair kernel over a CSR of the lists and one segmented reduction. */
int gorio_sc_cross_detect(gorio_sc_t* Q, gorio_sc_t* D, int count, const int* query_index, const int* const* candidates, const int* n_candidates,
                          int* loop_id, float* yaw_rad, double* min_dist);

/* Cumulative over Q's life: calls of this header that reached the device, pairs they evaluated, kernels they launched and stream
 * synchronisations they made.  Any output may be NULL. */
int gorio_sc_cross_counters(const gorio_sc_t* Q, long long* calls, long long* pairs, long long* launches, long long* synchronisations);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_SC_CROSS_H */
