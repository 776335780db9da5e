/*
 * gorio_search.h -- C ABI of the exact batched k-NN and radius queries against a cloud that lives on the MI355X (libgorio_amd.so):
 * the library's spatial index (a Morton order refined by median splits, boxes of 32-point tiles) behind a handle of
 * its own, for arbitrary query points.  The role pcl::search::KdTree::nearestKSearch / radiusSearch play on the host.
 *
 * Same conventions as include/gorio_sc.h: plain pointers, host pointers caller-owned and only read / written during the call, 0 on
 * success or a negative gorio_status (include/gorio_apd.h), gorio_search_last_error() gives the text (thread-local).  No CPU
 * fallback: without a HIP device gorio_search_create fails with GORIO_ERR_NO_DEVICE, so no other call can run.  Arguments are
 * checked before any device call and before any state changes; a refused call leaves the handle as it was, the cloud and the radius
 * result held included (a HIP error in the middle of a call may leave the handle without that result).  One handle must not be
 * used from two threads at once.
 *
 * Definitions (the ones the project already holds):
 *   - DISTANCE: the float squared distance of FLANN L2_Simple, un-fused: ((dx * dx) + dy * dy) + dz * dz -- sqdist3 of
 *     apd_kernels.hip, knn_self of the oracle.
 *   - K-NN: count = min(k, n) for a finite query; entries in ascending squared distance, equal distances in ascending ORIGINAL index
 *     of the cloud.  The unused slots count .. k-1 hold index -1 and distance +inf.
 *   - RADIUS: a neighbour has d < (float)(radius * radius), the product in double, the comparison strict (the FLANN rule of
 *     apd_prep.hip).  Order: ascending (d, index).  max_nn == 0 keeps every neighbour, max_nn > 0 the first max_nn of that order.
 *     Whether that truncation picks the neighbours PCL's radiusSearch(max_nn) picks is NOT pinned: FLANN stops its tree walk after
 *     max_nn hits, which need not be the nearest ones.
 *   - NON-FINITE QUERY (NaN or Inf in any coordinate): count 0, its k-NN slots filled as unused; it changes no other query's result.
 *   - A cloud with a non-finite point is refused (GORIO_ERR_INVALID) and the cloud already held stays.  n = 0 is a legal cloud:
 *     every query then has no neighbour.
 *
 * Query layout: q_xyz points at the first x, stride_bytes between queries (a multiple of 4, >= 12).  q_xyz == NULL means "the
 * cloud's own points in original order" (nq must then be the cloud's size); every point is then its own first neighbour, or the
 * lowest-index duplicate of it is.
 */
#ifndef GORIO_SEARCH_H
#define GORIO_SEARCH_H

#include "gorio_apd.h"
#include "gorio_keyframes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GORIO_SEARCH_MAX_K 32 /* the register-list cap of every k-NN in the library (gorio_apd_params.k_correspondences) */

typedef struct gorio_search_handle gorio_search_t; /* (gorio_search itself is the search-mode enum of gorio_apd.h) */

int gorio_search_create(gorio_search_t** out, int device);
void gorio_search_destroy(gorio_search_t* s);

/* The cloud from host memory: xyz points at the first x, stride_bytes between points (a multiple of 4, >= 12).  Uploads the points
 * and builds the index. */
int gorio_search_set_cloud(gorio_search_t* s, const float* xyz, int n, int stride_bytes);
/* The same from three device columns of n floats (on the handle's device); no host copy of the points is made. */
int gorio_search_set_cloud_device(gorio_search_t* s, const float* x, const float* y, const float* z, int n);

/* The cloud a registration handle holds (which = 0: its source, 1: its target) or a keyframe of a store, SHARED with the semantics
 * of gorio_apd_set_target_shared, "by value of the moment": both sides look at the same device-resident points and the same index
 * -- no point copy, no second index, none of this handle's counters moves.  When the owner has not built the index yet it is built
 * now through the owner, who then finds it built.  A later set_* on either side detaches that side only; destroying the owner (or
 * releasing the keyframe) leaves this handle working.  GORIO_ERR_STATE when the owner holds no such cloud, GORIO_ERR_INVALID for
 * another device or a cloud with a non-finite point. */
int gorio_search_set_cloud_from_apd(gorio_search_t* s, gorio_apd_t* apd, int which);
int gorio_search_set_cloud_from_keyframe(gorio_search_t* s, gorio_kf_t* kf, int id);

/* Size of the cloud held (0 before any set_*). */
int gorio_search_cloud_size(const gorio_search_t* s, int* n);

/* Calls that uploaded points from the host, index builds run through this handle, calls that downloaded results. */
int gorio_search_get_counters(const gorio_search_t* s, long long* point_uploads, long long* index_builds, long long* result_downloads);

/*
 * The k nearest cloud points of nq queries.  1 <= k <= 32 (k > 32: GORIO_ERR_UNSUPPORTED).  idx_out / sqd_out: nq * k entries,
 * query-major; count_out: nq entries (may be NULL).  nq == 0 is legal and does nothing.
 */
int gorio_search_knn(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, int k, int* idx_out, float* sqd_out, int* count_out);
/* The same with DEVICE pointers for the queries and the outputs: enqueued on the handle's stream (the launch stream its device's
 * handles share), no host copy of queries or results, returns without waiting for the device. */
int gorio_search_knn_device(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, int k, int* idx_out, float* sqd_out, int* count_out);

/*
 * All cloud points within `radius` (finite, > 0) of nq queries: a count pass, an exclusive scan and a fill pass on the device, every
 * query's neighbours then sorted by (d, index).  The result stays on the device as a CSR until the next radius call;
 * count_out[q] (host, nq entries, may be NULL) = neighbours kept for query q, *total = their sum.  When the neighbours found (before
 * max_nn cuts them) exceed 2^31 - 1 the call returns GORIO_ERR_UNSUPPORTED after the count pass, with nothing allocated or filled.
 */
int gorio_search_radius(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, double radius, int max_nn, int* count_out, long long* total);
/* The same with a DEVICE pointer for the queries; count_out stays a host array. */
int gorio_search_radius_device(gorio_search_t* s, const float* q_xyz, int nq, int stride_bytes, double radius, int max_nn, int* count_out, long long* total);
/*
 * `count` radius calls in one: job j is gorio_search_radius(handles[j], q_xyz[j], nq[j], stride_bytes[j], radius[j], max_nn[j],
 * count_out[j], &totals[j]), and its result -- counts, total and the CSR handles[j] then holds for gorio_search_radius_get -- is bit for
 * bit that call's.  What differs is the cost: the jobs share ONE set of launches and ONE synchronisation for the neighbours found (query
 * keys and their sort over all jobs, count, scan, fill, segment sort, the long segments of all jobs in one table), on the launch stream of
 * handles[0], so neither grows with count.  Queries are host pointers; q_xyz[j] == NULL means the cloud's own points (nq[j] must then be
 * its size).  count_out may be NULL and so may any entry of it; totals holds count entries.  nq[j] == 0 and an empty cloud are legal jobs
 * (no neighbour), and two handles may SHARE one cloud (gorio_search_set_cloud_from_apd / _from_keyframe of one owner).  count == 0 is
 * GORIO_OK and touches nothing.  GORIO_ERR_INVALID ("job <j>: ..."): count < 0, a null array or handle, the same handle twice, handles on
 * two devices, or a radius, max_nn, stride or nq the single call refuses -- checked for every job before any device call and before any
 * state changes.  When ANY job finds more than 2^31 - 1 neighbours the whole call returns GORIO_ERR_UNSUPPORTED ("job <j>: ...") after
 * the count pass, and every handle still holds the result it held before.
 */
int gorio_search_radius_batch(gorio_search_t** handles, int count, const float* const* q_xyz, const int* nq, const int* stride_bytes, const double* radius, const int* max_nn,
                              int* const* count_out, long long* totals);
/* Downloads the CSR of the last radius call: offsets_out[nq + 1], idx_out / sqd_out[total] (each may be NULL).  capacity (entries of
 * idx_out / sqd_out) < total returns GORIO_ERR_INVALID and writes nothing, whichever outputs are asked for; GORIO_ERR_STATE without
 * a radius result. */
int gorio_search_radius_get(gorio_search_t* s, long long* offsets_out, int* idx_out, float* sqd_out, long long capacity);

const char* gorio_search_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_SEARCH_H */
