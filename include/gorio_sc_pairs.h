/*
 * gorio_sc_pairs.h -- the exhaustive section of the Scan Context C ABI (libgorio_amd.so).  include/gorio_sc.h includes this header at
 * its end; the handle, the status codes, gorio_sc_last_error and the conventions are those of gorio_sc.h.
 *
 * An EXTENSION with no counterpart in the Go-RIO sources.  The reference computes the descriptor distance for the 3 nearest ring keys
 * of a kd-tree that is rebuilt every 10th call (SC:294-348); these calls compute it for every pair asked for.  What they keep of the
 * reference: the distance itself (distanceBtnScanContext, SC:127-160), and in gorio_sc_detect_exhaustive the early return
 * (SC:284-288), the recent-keyframe filter (SC:294-306), the strict minimum in list order (SC:341-348), the threshold and the yaw
 * (SC:354-371).  What they drop: the ring-key k-NN, NUM_CANDIDATES_FROM_TREE, the tree-making counter and the stale snapshot.
 *
 * d(q, c) below is distanceBtnScanContext(polarcontexts_[q], polarcontexts_[c]) with q the unshifted side; it is not symmetric.  Every
 * value these calls return is, bit for bit, what gorio_sc_distance(h, q, c, ...) returns, (1e7, 0) included when no shift has an
 * effective column: all of them run one per-pair device function.
 *
 * Conventions: every check happens before any device call and before any state change, a refused call changes nothing and writes
 * nothing, the text names the offending entry, count == 0 (or an empty extent) returns GORIO_OK and touches nothing.  None of these
 * calls reads or writes the tree-making counter or the snapshot.  Each call that computes uses one upload, a launch count that does
 * not depend on the extents, one copy back per output array and ONE stream synchronisation; results are deterministic (no
 * floating-point atomics, no waits between workgroups).
 */
#ifndef GORIO_SC_PAIRS_H
#define GORIO_SC_PAIRS_H

#ifdef __cplusplus
extern "C" {
#endif

/* The tile kernel of gorio_sc_distance_matrix and gorio_sc_best_matches stages this many row and column records per workgroup;
 * extents around them (N - 1, N, N + 1, 2 N + 3) are where its partial tiles begin.  The listed-pairs kernel of
 * gorio_sc_distance_pairs and gorio_sc_detect_exhaustive evaluates GORIO_SC_PAIRS_PER_GROUP pairs per workgroup. */
#define GORIO_SC_TILE_ROWS 8
#define GORIO_SC_TILE_COLS 8
#define GORIO_SC_PAIRS_PER_GROUP 4

/* dist[k], shift[k] = d(q[k], c[k]) for k < count.  One launch. */
int gorio_sc_distance_pairs(gorio_sc_t* h, const int* q, const int* c, int count, double* dist, int* shift);

/* dist[i * n_cols + j], shift[i * n_cols + j] = d(rows[i], cols[j]).  rows or cols may be NULL, meaning 0 .. n_scans - 1 (the extent
 * must then be n_scans).  Either output may be NULL (not both).  Indices may repeat, a row may equal a column.
 * n_rows * n_cols > 2^31 - 1: GORIO_ERR_UNSUPPORTED, before anything is allocated.  One launch. */
int gorio_sc_distance_matrix(gorio_sc_t* h, const int* rows, int n_rows, const int* cols, int n_cols, double* dist, int* shift);

/* The loop-mining primitive.  For each row r = rows[i] (NULL: 0 .. n_scans - 1) the minimum of d(r, c) over the database indices
 * 0 <= c <= r - min_gap, min_gap >= 1; ties go to the lower c.  (best_index, best_dist, best_shift) = (-1, 1e7, 0) when there is no
 * such c or none scores below 1e7.  best_shift may be NULL.  The matrix is never materialised: column tiles are folded into a running
 * (dist, index) per row on the device, only n_rows results come down, device memory is O(n_rows + tile).  Two launches. */
int gorio_sc_best_matches(gorio_sc_t* h, const int* rows, int n_rows, int min_gap, int* best_index, double* best_dist, int* best_shift);

/*
 * detectLoopClosureID (SC:272-373) with the tree stage (SC:294-338) replaced by ALL candidates, for `count` queries in one pass.
 * Per query: query_index < NUM_EXCLUDE_RECENT returns (-1, 0, 1e7) (SC:284-288).  Otherwise a candidate c of the CURRENT list is kept
 * iff (size_t)(query - c) >= NUM_EXCLUDE_RECENT (SC:300 applied to this call's list: a candidate after the query wraps and is kept),
 * d(query, c) is computed for every kept candidate, the minimum is strict from 1e7 and in list order (SC:341-348), and loop_id,
 * yaw_rad, min_dist follow SC:354-371 exactly as gorio_sc_detect computes them (no kept candidate, or none below 1e7: -1, the yaw of
 * shift 0, 1e7).  Stateless: the counter and the snapshot are neither read nor written.  An empty list, or indices never added:
 * GORIO_ERR_INVALID, as in gorio_sc_detect.  Two launches: the pair kernel over a CSR of kept candidates and one segmented reduction.
 */
int gorio_sc_detect_exhaustive(gorio_sc_t* h, int count, const int* query_index, const int* const* candidates, const int* n_candidates, int* loop_id, float* yaw_rad,
                               double* min_dist);

/* Cumulative over the handle's life: calls of this header that reached the device, pairs they evaluated, kernels they launched and
 * stream synchronisations they made.  Any output may be NULL. */
int gorio_sc_pairs_counters(const gorio_sc_t* h, long long* calls, long long* pairs, long long* launches, long long* synchronisations);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_SC_PAIRS_H */
