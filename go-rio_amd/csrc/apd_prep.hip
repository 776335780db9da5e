// apd_prep.hip -- preprocessing that feeds the hot path: the radius searches of the DBSCAN cluster labelling
// (preprocessing_nodelet_ntu.cpp:518-568, DBSCAN_simple.h:28-100).  Kernels first, the host side of include/gorio_prep.h below them.  Included at the end of
// apd_api.hip.
//
// DBSCAN_simple.h is an order-dependent queue (points visited in index order, first cluster to reach a point keeps it as a member,
// seed neighbours re-queued whatever their state) whose cost is entirely in its radius searches -- one per visited point, each a
// kd-tree query in the reference.  Here EVERY point's neighbourhood is found at once on the GPU, through the same exact tile search
// the registration uses, for the larger of the two radii the queue can ask for:
//   seed radius       |norm - 1| / 50 + eps    (DBSCAN_simple.h:36-40)
//   expansion radius  (norm - 1) / 100 + eps   (DBSCAN_simple.h:65-68; never larger than the seed radius)
// as a CSR adjacency (neighbour index, one flag bit for "also inside the expansion radius"); the queue itself is then replayed on
// the host over that adjacency, statement for statement, so the clusters are exactly the reference's.
// A neighbour is a point whose float squared distance (FLANN L2_Simple, un-fused) is < (float)(radius * radius), the query included.
#include <hip/hip_runtime.h>

namespace gorio {

struct RadiusArgs {
  double eps;
  int* cnt;               // [n] by ORIGINAL index: neighbours inside the seed radius
  const long long* offs;  // [n] by original index (fill pass)
  int* adj;               // CSR payload: neighbour original index | 0x80000000 when also inside the expansion radius
};

// mode 0: count; mode 1: fill.  grid: ceil(n_spad / 256), block 256.  One lane = one query in sorted order.
// The search kernels of this file are per-workgroup bodies, `block` the 256-query block, and a __global__ that hands them blockIdx.x; the
// job-table kernels of apd_scan_batch.hip hand the same bodies the block of a (job, block) entry.
template <int MODE>
__device__ __forceinline__ void radius_neighbours_body(const CloudView& cloud, const RadiusArgs& a, int block) {
  const SearchIndex& si = cloud.idx;
  const int n = si.n;
  const int p = block * 256 + threadIdx.x;
  if (block * 256 >= n) return;
  const int lane = threadIdx.x & 63;
  const int pq = p < n ? p : n - 1;
  const float qx = si.sx[pq], qy = si.sy[pq], qz = si.sz[pq];
  // DBSCAN_simple.h:36-39: the seed radius stores std::sqrt(float expression) in a double and continues in double; DBS:65-67: the
  // expansion radius evaluates (std::sqrt(float) - 1) / 100 entirely in FLOAT and only adds the double eps_ in double
  float n2 = qx * qx;
  n2 = n2 + qy * qy;
  n2 = n2 + qz * qz;
  const double norm = (double)sqrtf(n2);
  const float ef = (sqrtf(n2) - 1.0f) / 100.0f;
  const double r_seed = fabs(norm - 1) / 50 + a.eps, r_exp = (double)ef + a.eps;
  const float r2s = p < n ? (float)(r_seed * r_seed) : 0.0f, r2e = (float)(r_exp * r_exp);
  const float qlo[3] = {wave_min(qx), wave_min(qy), wave_min(qz)};
  const float qhi[3] = {wave_max(qx), wave_max(qy), wave_max(qz)};
  const scalar_fp tx = as_scalar(si.sx);
  const scalar_fp ty = as_scalar(si.sy);
  const scalar_fp tz = as_scalar(si.sz);
  const scalar_ip to = (scalar_ip)si.orig;
  const float4* __restrict__ tb4 = reinterpret_cast<const float4*>(si.tbox);
  const int ng = (si.n_tiles + 63) / 64;
  const float wb = wave_max(r2s);
  const int me = p < n ? si.orig[p] : 0;
  int cnt = 0;
  int* out = nullptr;
  if (MODE == 1 && p < n) out = a.adj + a.offs[me];
  for (int g = 0; g < ng; ++g) {
    const int tl = g * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (tl < si.n_tiles) {
      lo = tb4[2 * (size_t)tl];
      hi = tb4[2 * (size_t)tl + 1];
    }
    unsigned long long mask = __ballot(box_box_bound(qlo, qhi, lo, hi) < wb);
    while (mask) {
      const int tlane = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float bx[8] = {lane_f(lo.x, tlane), lane_f(lo.y, tlane), lane_f(lo.z, tlane), 0.f, lane_f(hi.x, tlane), lane_f(hi.y, tlane), lane_f(hi.z, tlane), 0.f};
      if (__ballot(box_bound(qx, qy, qz, bx) < r2s) == 0) continue;
      const int j0 = (g * 64 + tlane) * 32;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) {
        const float d = sqdist3(qx, qy, qz, tx[j0 + u], ty[j0 + u], tz[j0 + u]);
        if (d < r2s) {  // padding points sit at 1e30: d = inf
          if (MODE == 1) out[cnt] = to[j0 + u] | (d < r2e ? (int)0x80000000 : 0);
          ++cnt;
        }
      }
    }
  }
  if (MODE == 0 && p < n) a.cnt[me] = cnt;
}
template <int MODE>
__global__ __launch_bounds__(256) void radius_neighbours_kernel(CloudView cloud, RadiusArgs a) {
  radius_neighbours_body<MODE>(cloud, a, blockIdx.x);
}

// pcl::RadiusOutlierRemoval as the preprocessing nodelet configures it (preprocessing_nodelet_ntu.cpp:163-171, 626-634; launch files:
// radius 2 m, 1 - 5 neighbours): number of points of the SAME cloud, the query included, whose float squared distance is at most the
// squared radius.  r2 = largest float whose double value is <= radius * radius (the comparison PCL makes is in double on float
// distances).  grid: ceil(n_spad / 256), block 256; cnt[] by ORIGINAL index.
__device__ __forceinline__ void radius_count_body(const CloudView& cloud, float r2, int* __restrict__ cnt_out, int block) {
  const SearchIndex& si = cloud.idx;
  const int n = si.n;
  const int p = block * 256 + threadIdx.x;
  if (block * 256 >= n) return;
  const int lane = threadIdx.x & 63;
  const int pq = p < n ? p : n - 1;
  const float qx = si.sx[pq], qy = si.sy[pq], qz = si.sz[pq];
  const float qlo[3] = {wave_min(qx), wave_min(qy), wave_min(qz)};
  const float qhi[3] = {wave_max(qx), wave_max(qy), wave_max(qz)};
  const scalar_fp tx = as_scalar(si.sx);
  const scalar_fp ty = as_scalar(si.sy);
  const scalar_fp tz = as_scalar(si.sz);
  const float4* __restrict__ tb4 = reinterpret_cast<const float4*>(si.tbox);
  const int ng = (si.n_tiles + 63) / 64;
  int cnt = 0;
  for (int g = 0; g < ng; ++g) {
    const int tl = g * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (tl < si.n_tiles) {
      lo = tb4[2 * (size_t)tl];
      hi = tb4[2 * (size_t)tl + 1];
    }
    unsigned long long mask = __ballot(box_box_bound(qlo, qhi, lo, hi) <= r2);
    while (mask) {
      const int tlane = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float bx[8] = {lane_f(lo.x, tlane), lane_f(lo.y, tlane), lane_f(lo.z, tlane), 0.f, lane_f(hi.x, tlane), lane_f(hi.y, tlane), lane_f(hi.z, tlane), 0.f};
      if (__ballot(box_bound(qx, qy, qz, bx) <= r2) == 0) continue;
      const int j0 = (g * 64 + tlane) * 32;
#pragma unroll 4
      for (int u = 0; u < 32; ++u) cnt += sqdist3(qx, qy, qz, tx[j0 + u], ty[j0 + u], tz[j0 + u]) <= r2 ? 1 : 0;  // padding points: d = inf
    }
  }
  if (p < n) cnt_out[si.orig[p]] = cnt;
}
__global__ __launch_bounds__(256) void radius_count_kernel(CloudView cloud, float r2, int* __restrict__ cnt_out) { radius_count_body(cloud, r2, cnt_out, blockIdx.x); }


// pcl::StatisticalOutlierRemoval, first half (PCL 1.10 filters/impl/statistical_outlier_removal.hpp, as preprocessing_nodelet_ntu.cpp:
// 153-162 configures it -- the nodelet's DEFAULT outlier filter, mean_k 20 / 30): for every point the mean of the distances to its
// mean_k nearest neighbours, the point itself (the first of the mean_k + 1 results of nearestKSearch) left out.  The k = mean_k + 1
// smallest float squared distances are kept as in knn_kth_kernel -- an ascending register list, a candidate enters by
// D[t] = med3(D[t-1], c, D[t]) -- with ONE list length for every k <= 32: the 32 - k slots below the list proper hold -inf, which no
// candidate moves, so D[31] is the k-th smallest throughout.  The sum runs over the sorted distances 1 .. k-1 in double, on double
// square roots of the float values, and is divided by mean_k and rounded to float as PCL does.
// grid: ceil(n_spad / 256), block 256; mean_out[] by ORIGINAL index.
__device__ __forceinline__ void sor_mean_distance_body(const CloudView& cloud, int k, float* __restrict__ mean_out, int block) {
  constexpr int K = 32;
  const SearchIndex& si = cloud.idx;
  const int n = si.n;
  const int p = block * 256 + threadIdx.x;
  if (block * 256 >= n) return;
  const int lane = threadIdx.x & 63;
  const int pq = p < n ? p : n - 1;
  const float qx = si.sx[pq], qy = si.sy[pq], qz = si.sz[pq];
  const float qlo[3] = {wave_min(qx), wave_min(qy), wave_min(qz)};
  const float qhi[3] = {wave_max(qx), wave_max(qy), wave_max(qz)};
  const scalar_fp tx = as_scalar(si.sx);
  const scalar_fp ty = as_scalar(si.sy);
  const scalar_fp tz = as_scalar(si.sz);
  const float4* __restrict__ tb4 = reinterpret_cast<const float4*>(si.tbox);
  const int ng = (si.n_tiles + 63) / 64;
  const int g0 = (block * 256 + (threadIdx.x & ~63)) / 32 / 64;  // the group of this wave's own tiles: visited first, it tightens the bounds
  float D[K];
#pragma unroll
  for (int t = 0; t < K; ++t) D[t] = t < K - k ? -INFINITY : INFINITY;
  for (int v = 0; v < 2 * ng; ++v) {
    const int off = (v + 1) >> 1;
    const int g = (v & 1) ? g0 - off : g0 + off;
    if (g < 0 || g >= ng) continue;
    const int tl = g * 64 + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (tl < si.n_tiles) {
      lo = tb4[2 * (size_t)tl];
      hi = tb4[2 * (size_t)tl + 1];
    }
    const float wb = wave_max(D[K - 1]);
    unsigned long long mask = __ballot(box_box_bound(qlo, qhi, lo, hi) < wb);  // strictly below: an equal distance changes no distance list
    while (mask) {
      const int tlane = __builtin_ctzll(mask);
      mask &= mask - 1;
      const float bx[8] = {lane_f(lo.x, tlane), lane_f(lo.y, tlane), lane_f(lo.z, tlane), 0.f, lane_f(hi.x, tlane), lane_f(hi.y, tlane), lane_f(hi.z, tlane), 0.f};
      if (__ballot(box_bound(qx, qy, qz, bx) < D[K - 1]) == 0) continue;
      const int j0 = (g * 64 + tlane) * 32;
#pragma unroll 2
      for (int u = 0; u < 32; ++u) {
        const float c = sqdist3(qx, qy, qz, tx[j0 + u], ty[j0 + u], tz[j0 + u]);  // padding points sit at 1e30: c = inf
        if (__ballot(c < D[K - 1]) == 0) continue;
#pragma unroll
        for (int t = K - 1; t > 0; --t) D[t] = __builtin_amdgcn_fmed3f(D[t - 1], c, D[t]);
        D[0] = __builtin_amdgcn_fmed3f(D[0], c, -INFINITY);
      }
    }
  }
  if (p < n) {
    double sum = 0.0;
#pragma unroll
    for (int t = 1; t < K; ++t)  // slot K - k is the query itself (distance 0, or the nearest of its duplicates)
      if (t > K - k) sum += sqrt((double)D[t]);
    mean_out[si.orig[p]] = (float)(sum / (double)(k - 1));
  }
}
__global__ __launch_bounds__(256) void sor_mean_distance_kernel(CloudView cloud, int k, float* __restrict__ mean_out) { sor_mean_distance_body(cloud, k, mean_out, blockIdx.x); }

// PREP:539-548 for a cloud that lives on the device: the float coordinate sums of every cluster, its members added one after the other in
// ascending index order exactly as the host loop of gorio_prep_dbscan_labels adds them.  One lane = one cluster (there are tens of them);
// grid: ceil(nc / 64), block 64.
__device__ __forceinline__ void cluster_sums_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int* __restrict__ members,
                                                  const int* __restrict__ offs, int nc, float* __restrict__ sums, int block) {
  const int c = block * 64 + threadIdx.x;
  if (c >= nc) return;
  float sx = 0.f, sy = 0.f, sz = 0.f;
  for (int e = offs[c]; e < offs[c + 1]; ++e) {
    const int idx = members[e];
    sx += x[idx];
    sy += y[idx];
    sz += z[idx];
  }
  sums[3 * c] = sx;
  sums[3 * c + 1] = sy;
  sums[3 * c + 2] = sz;
}
__global__ __launch_bounds__(64) void cluster_sums_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, const int* __restrict__ members,
                                                          const int* __restrict__ offs, int nc, float* __restrict__ sums) {
  cluster_sums_body(x, y, z, members, offs, nc, sums, blockIdx.x);
}

}  // namespace gorio

// ----------------------------------------------------------------------------------------------- REVE Doppler ego-velocity
// REVE = the reference's src/radar_ego_velocity_estimator.cpp.  The per-target work of estimate() (REVE:75-90: range,
// azimuth / elevation gates, unit direction, corrected Doppler), of every RANSAC hypothesis (REVE:203-214: |y - H v| against the
// inlier threshold for ALL targets) and of the final least squares (REVE:252-290: H^T H, H^T y, e^T e) are data parallel and run
// here; the 3 x 3 solves, the order statistic and the bookkeeping of the best hypothesis are a few hundred flops on the host.
namespace gorio {

struct ReveCfg {
  double min_dist, max_dist, min_db, az_lim, el_lim, doppler_factor_unused;
  float doppler_factor;
  float pad_;
};

// grid: ceil(n / 256).  f[i][4] = x/r, y/r, z/r, corrected doppler; valid[i]
// px / py / pz: first x, y, z; `stride` floats between targets (5 for the packed upload of gorio_prep_ego_velocity, 1 for device columns)
__device__ __forceinline__ void reve_features_body(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, const float* __restrict__ inten,
                                                   const float* __restrict__ dop, int stride, int n, const ReveCfg& c, double* __restrict__ f, unsigned char* __restrict__ valid, int block) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = px[(size_t)i * stride], y = py[(size_t)i * stride], z = pz[(size_t)i * stride];
  const double r = sqrt((double)x * (double)x + (double)y * (double)y + (double)z * (double)z);  // Vector3(x, y, z).norm(), REVE:78
  const double azimuth = (double)(float)atan2((double)y, (double)x);                           // atan2(float, float), REVE:80
  float rxy2 = x * x;
  rxy2 = rxy2 + y * y;
  const float rxy = (float)sqrt((double)rxy2);
  const double elevation = (double)(float)atan2((double)rxy, (double)z) - 1.57079632679489661923;  // REVE:81
  const bool ok = r > c.min_dist && r < c.max_dist && (double)inten[(size_t)i * stride] > c.min_db && fabs(azimuth) < c.az_lim && fabs(elevation) < c.el_lim;
  valid[i] = ok ? 1 : 0;
  const float d = -dop[(size_t)i * stride] * c.doppler_factor;  // float product, REVE:87
  f[4 * (size_t)i] = x / r;
  f[4 * (size_t)i + 1] = y / r;
  f[4 * (size_t)i + 2] = z / r;
  f[4 * (size_t)i + 3] = (double)d;
}
__global__ __launch_bounds__(256) void reve_features_kernel(const float* __restrict__ px, const float* __restrict__ py, const float* __restrict__ pz, const float* __restrict__ inten,
                                                            const float* __restrict__ dop, int stride, int n, ReveCfg c, double* __restrict__ f, unsigned char* __restrict__ valid) {
  reve_features_body(px, py, pz, inten, dop, stride, n, c, f, valid, blockIdx.x);
}

// grid: (ceil(m / 256), hypotheses).  flags[k][j] = |y_j - h_j . v_k| < thresh (REVE:203-214) over the VALID targets
__device__ __forceinline__ void reve_eval_body(const double* __restrict__ f, int m, const double* __restrict__ v /* [K][3] */, double thresh, unsigned char* __restrict__ flags, int block,
                                               int k) {
  const int j = block * 256 + threadIdx.x;
  if (j >= m) return;
  const double* r = f + 4 * (size_t)j;
  const double err = fabs(r[3] - (r[0] * v[3 * k] + r[1] * v[3 * k + 1] + r[2] * v[3 * k + 2]));
  flags[(size_t)k * m + j] = err < thresh ? 1 : 0;
}
__global__ __launch_bounds__(256) void reve_eval_kernel(const double* __restrict__ f, int m, const double* __restrict__ v /* [K][3] */, double thresh, unsigned char* __restrict__ flags) {
  reve_eval_body(f, m, v, thresh, flags, blockIdx.x, blockIdx.y);
}

// grid: ceil(m / 256).  per block: 10 sums over the selected rows -- H^T H (6 unique), H^T y (3), and, with v, e^T e of e = H v - y
__device__ __forceinline__ void reve_sums_body(const double* __restrict__ f, int m, const unsigned char* __restrict__ sel, const double* __restrict__ v, double* __restrict__ out, int block) {
  const int j = block * 256 + threadIdx.x;
  double a[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) a[q] = 0.0;
  if (j < m && sel[j]) {
    const double* r = f + 4 * (size_t)j;
    a[0] = r[0] * r[0]; a[1] = r[0] * r[1]; a[2] = r[0] * r[2]; a[3] = r[1] * r[1]; a[4] = r[1] * r[2]; a[5] = r[2] * r[2];
    a[6] = r[0] * r[3]; a[7] = r[1] * r[3]; a[8] = r[2] * r[3];
    if (v) {
      const double e = (r[0] * v[0] + r[1] * v[1] + r[2] * v[2]) - r[3];
      a[9] = e * e;
    }
  }
  __shared__ double red[4][10];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 10; ++q) {
    const double s = wave_sum(a[q]);
    if (lane == 0) red[wv][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < 10) out[(size_t)block * 10 + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}
__global__ __launch_bounds__(256) void reve_sums_kernel(const double* __restrict__ f, int m, const unsigned char* __restrict__ sel, const double* __restrict__ v, double* __restrict__ out) {
  reve_sums_body(f, m, sel, v, out, blockIdx.x);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_prep.h)
// Included at the end of apd_api.hip: the filters work through a private registration handle (gorio_apd, DevCloud, run_index_build).

namespace {
thread_local std::string g_prep_err;
int prep_fail(int code, const std::string& m) {
  g_prep_err = m;
  return code;
}

struct PrepCtx {  // per thread: a private registration handle serves as the device-side cloud + search-index holder
  gorio_apd* h = nullptr;
  int device = -1;
  DevBuf<int> d_cnt;  // d_cnt and d_offs: one group of capacity pts_cap (points)
  DevBuf<long long> d_offs;
  size_t pts_cap = 0;
  DevBuf<int> d_adj;
  void reset() {  // back to the empty context; the buffers free on the device they live on
    if (!h) return;
    hipSetDevice(device);
    d_cnt.reset(), d_offs.reset(), d_adj.reset();
    pts_cap = 0;
    gorio_apd_destroy(h);
    h = nullptr;
    device = -1;
  }
  ~PrepCtx() { reset(); }
};
thread_local PrepCtx g_prep;

// a context (the thread's, or the one a scan pipeline owns), ready for `device`; nullptr (and `rc`, the error recorded) when the device
// is not usable
PrepCtx* prep_context(PrepCtx& c, int device, const char* who, int& rc) {
  rc = GORIO_OK;
  if (!c.h || c.device != device) {
    c.reset();
    rc = gorio_apd_create(&c.h, device);
    if (rc) {
      prep_fail(rc, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
      return nullptr;
    }
    c.device = device;
  }
  return &c;
}
PrepCtx* prep_context(int device, const char* who, int& rc) { return prep_context(g_prep, device, who, rc); }

// the source of the context's handle gets its search index built and one d_cnt / d_offs slot per point
int prep_index_source(PrepCtx& c, int n) {
  gorio_apd* h = c.h;
  std::vector<std::pair<gorio_apd*, DevCloud*>> one = {{h, h->src.get()}};
  int rc = run_index_build(h, one);
  if (rc) return prep_fail(rc, h->err);
  const size_t cap = (size_t)n + n / 8;
  GORIO_HIP_CHECK(prep_fail, reserve_group(c.pts_cap, n, cap, c.d_cnt, cap, c.d_offs, cap));
  return GORIO_OK;
}

// the cloud becomes the source of the context's handle, with its search index built and one d_cnt / d_offs slot per point
int prep_index_cloud(PrepCtx& c, const float* xyz, int n, int point_stride_bytes) {
  gorio_apd* h = c.h;
  h->params.search = GORIO_SEARCH_PRUNED;
  int rc = gorio_apd_set_source(h, xyz, nullptr, n, point_stride_bytes);
  if (rc) return prep_fail(rc, h->err);
  return prep_index_source(c, n);
}

// the same for a cloud that already lives on the device as three columns (include/gorio_scan.h): no host copy is made
int prep_index_cloud_device(PrepCtx& c, const float* dx, const float* dy, const float* dz, int n) {
  gorio_apd* h = c.h;
  h->params.search = GORIO_SEARCH_PRUNED;
  int rc = gorio_apd_set_source_device(h, dx, dy, dz, nullptr, n);
  if (rc) return prep_fail(rc, h->err);
  return prep_index_source(c, n);
}

// ---- the stages proper, on the indexed source of the context's handle.  The public entry points below and the scan pipeline
// (apd_scan.hip) both run these; what differs is only where the cloud came from.

void prep_dbscan_replay(const std::vector<int>& cnt, const std::vector<long long>& offs, const std::vector<int>& adj, int n, int core_min_pts, int min_cluster_size, int max_cluster_size,
                        std::vector<std::vector<int>>& clusters);

// DBS:28-100: the radius searches on the device, the queue replayed over their adjacency; clusters in the order the queue closes them,
// members sorted (DBS:91)
int prep_dbscan_clusters(PrepCtx& c, int n, double eps, int core_min_pts, int min_cluster_size, int max_cluster_size, std::vector<std::vector<int>>& clusters) {
  gorio_apd* h = c.h;
  const CloudView cv = h->src->view();
  const int grid = (roundup(n, 512) + 255) / 256;
  RadiusArgs ra{eps, c.d_cnt, c.d_offs, nullptr};
  radius_neighbours_kernel<0><<<grid, 256, 0, h->stream>>>(cv, ra);
  GORIO_HIP_CHECK(prep_fail, hipGetLastError());
  std::vector<int> cnt((size_t)n);
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(cnt.data(), c.d_cnt, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(h->stream));
  std::vector<long long> offs((size_t)n + 1);
  offs[0] = 0;
  for (int i = 0; i < n; ++i) offs[i + 1] = offs[i] + cnt[i];
  const long long E = offs[n];
  GORIO_HIP_CHECK(prep_fail, c.d_adj.reserve((size_t)E, (size_t)E + (size_t)E / 8 + 16));
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(c.d_offs, offs.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  ra.adj = c.d_adj;
  radius_neighbours_kernel<1><<<grid, 256, 0, h->stream>>>(cv, ra);
  GORIO_HIP_CHECK(prep_fail, hipGetLastError());
  std::vector<int> adj((size_t)E);
  if (E > 0) GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(adj.data(), c.d_adj, sizeof(int) * (size_t)E, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(h->stream));
  prep_dbscan_replay(cnt, offs, adj, n, core_min_pts, min_cluster_size, max_cluster_size, clusters);
  return GORIO_OK;
}

// the queue of DBSCAN_simple.h:28-100, statement for statement, over the adjacency (the radius searches are done)
void prep_dbscan_replay(const std::vector<int>& cnt, const std::vector<long long>& offs, const std::vector<int>& adj, int n, int core_min_pts, int min_cluster_size, int max_cluster_size,
                        std::vector<std::vector<int>>& clusters) {
  enum : unsigned char { UN = 0, PROCESSING = 1, PROCESSED = 2 };
  std::vector<unsigned char> types((size_t)n, UN), noise((size_t)n, 0);
  std::vector<int> queue;
  clusters.clear();
  auto seed_count = [&](int i) { return cnt[i]; };  // |N(i, seed radius)|, the point itself included
  auto exp_count = [&](int i) {
    int k = 0;
    for (long long e = offs[i]; e < offs[i + 1]; ++e) k += (adj[(size_t)e] < 0);
    return k;
  };
  for (int i = 0; i < n; ++i) {
    if (types[i] == PROCESSED) continue;
    if (seed_count(i) < core_min_pts) {
      noise[i] = 1;
      continue;
    }
    queue.clear();
    queue.push_back(i);
    types[i] = PROCESSED;
    for (long long e = offs[i]; e < offs[i + 1]; ++e) {
      const int j = adj[(size_t)e] & 0x7fffffff;
      if (j != i) {
        queue.push_back(j);  // DBS:50-54: whatever its state
        types[j] = PROCESSING;
      }
    }
    size_t sq = 1;
    while (sq < queue.size()) {
      const int q = queue[sq];
      if (noise[q] || types[q] == PROCESSED) {
        types[q] = PROCESSED;
        sq++;
        continue;
      }
      if (exp_count(q) >= core_min_pts) {
        for (long long e = offs[q]; e < offs[q + 1]; ++e) {
          if (adj[(size_t)e] >= 0) continue;  // outside the expansion radius
          const int j = adj[(size_t)e] & 0x7fffffff;
          if (types[j] == UN) {
            queue.push_back(j);
            types[j] = PROCESSING;
          }
        }
      }
      types[q] = PROCESSED;
      sq++;
    }
    if ((int)queue.size() >= min_cluster_size && (int)queue.size() <= max_cluster_size) clusters.push_back(queue);  // DBS:83-95
  }
  for (std::vector<int>& m : clusters) std::sort(m.begin(), m.end());  // DBS:91
}

// PREP:550-568 from the float coordinate sums of the clusters (sums[c][3], PREP:539-548): rank[c] = position of cluster c when the
// clusters are ordered by the distance of their centroid
void prep_rank_clusters(const std::vector<std::vector<int>>& clusters, const float* sums, std::vector<int>& order) {
  const int nc = (int)clusters.size();
  std::vector<float> dist((size_t)nc);
  order.resize((size_t)nc);
  for (int cidx = 0; cidx < nc; ++cidx) {
    const int num = (int)clusters[cidx].size();
    const float cx = sums[3 * cidx] / num, cy = sums[3 * cidx + 1] / num, cz = sums[3 * cidx + 2] / num;
    dist[cidx] = (float)std::sqrt((double)cx * cx + (double)cy * cy + (double)cz * cz);  // std::hypot(float, float, float)
    order[cidx] = cidx;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return dist[a] < dist[b]; });
}

// pcl::RadiusOutlierRemoval: the neighbour counts of every point of the indexed source, then the mask
float prep_radius_r2(double radius) {
  const double r2d = radius * radius;
  float r2 = FLT_MAX;
  if (r2d < (double)FLT_MAX) {  // largest float whose double value is <= r^2: (double)d <= r^2  <=>  d <= r2 for every float d
    r2 = (float)r2d;
    while ((double)r2 > r2d) r2 = std::nextafterf(r2, 0.0f);
  }
  return r2;
}
// the mask from the neighbour counts
void prep_radius_keep_from_counts(const int* cnt, int n, int min_neighbors, unsigned char* keep, int* n_kept) {
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    keep[i] = cnt[i] > min_neighbors ? 1 : 0;  // the query itself is one of the counted points
    kept += keep[i];
  }
  if (n_kept) *n_kept = kept;
}
int prep_radius_outlier_keep(PrepCtx& c, int n, double radius, int min_neighbors, unsigned char* keep, int* n_kept) {
  gorio_apd* h = c.h;
  const float r2 = prep_radius_r2(radius);
  radius_count_kernel<<<(roundup(n, 512) + 255) / 256, 256, 0, h->stream>>>(h->src->view(), r2, c.d_cnt);
  GORIO_HIP_CHECK(prep_fail, hipGetLastError());
  std::vector<int> cnt((size_t)n);
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(cnt.data(), c.d_cnt, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(h->stream));
  prep_radius_keep_from_counts(cnt.data(), n, min_neighbors, keep, n_kept);
  return GORIO_OK;
}

// mean and standard deviation of the per-point values and the threshold, in PCL's order and types (statistical_outlier_removal.hpp:
// double sums over the float distances in point order, the n - 1 form of the variance); N numbers: done on the host
void prep_sor_keep_from_distances(const float* dist, int n, double stddev_mul, unsigned char* keep, int* n_kept, float* mean_dist_out) {
  double sum = 0.0, sq_sum = 0.0;
  for (int i = 0; i < n; ++i) {
    sum += dist[i];
    sq_sum += dist[i] * dist[i];
  }
  const double mean = sum / static_cast<double>(n);
  const double variance = (sq_sum - sum * sum / static_cast<double>(n)) / (static_cast<double>(n) - 1);
  const double stddev = std::sqrt(variance);
  const double threshold = mean + stddev_mul * stddev;
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    keep[i] = dist[i] <= threshold ? 1 : 0;  // negative_ = false: the inliers stay
    kept += keep[i];
    if (mean_dist_out) mean_dist_out[i] = dist[i];
  }
  if (n_kept) *n_kept = kept;
}

// pcl::StatisticalOutlierRemoval: the mean neighbour distance of every point of the indexed source, then threshold and mask
int prep_statistical_outlier_keep(PrepCtx& c, int n, int mean_k, double stddev_mul, unsigned char* keep, int* n_kept, float* mean_dist_out) {
  gorio_apd* h = c.h;
  float* d_mean = reinterpret_cast<float*>(c.d_cnt.get());  // one 4-byte word per point, like the neighbour counts
  sor_mean_distance_kernel<<<(roundup(n, 512) + 255) / 256, 256, 0, h->stream>>>(h->src->view(), mean_k + 1, d_mean);
  GORIO_HIP_CHECK(prep_fail, hipGetLastError());
  std::vector<float> dist((size_t)n);
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(dist.data(), d_mean, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(h->stream));
  prep_sor_keep_from_distances(dist.data(), n, stddev_mul, keep, n_kept, mean_dist_out);
  return GORIO_OK;
}

const char* const kSorTooFew = "statistical_outlier_mask: fewer points than mean_k + 1 (PCL then sums distances nearestKSearch never set)";
}  // namespace

extern "C" {

const char* gorio_prep_last_error(void) { return g_prep_err.c_str(); }

int gorio_prep_dbscan_labels(int device, const float* xyz, int n, int point_stride_bytes, double eps, int core_min_pts, int min_cluster_size, int max_cluster_size,
                             float* label_out, int label_stride_bytes, int* n_clusters) {
  if (!xyz || !label_out || n <= 0 || point_stride_bytes < 12 || (point_stride_bytes % 4) || label_stride_bytes < 4 || (label_stride_bytes % 4))
    return prep_fail(GORIO_ERR_INVALID, "dbscan_labels: bad arguments");
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "dbscan_labels", rc);
  if (!ctx) return rc;
  PrepCtx& c = *ctx;
  rc = prep_index_cloud(c, xyz, n, point_stride_bytes);
  if (rc) return rc;
  std::vector<std::vector<int>> clusters;
  rc = prep_dbscan_clusters(c, n, eps, core_min_pts, min_cluster_size, max_cluster_size, clusters);
  if (rc) return rc;
  // ---- preprocessing_nodelet_ntu.cpp:533-568: rank the clusters by the distance of their centroid, write rank + 1
  const int st = point_stride_bytes / 4, lst = label_stride_bytes / 4;
  for (int i = 0; i < n; ++i) label_out[(size_t)i * lst] = 0.0f;
  const int nc = (int)clusters.size();
  std::vector<float> sums((size_t)nc * 3);
  for (int cidx = 0; cidx < nc; ++cidx) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int idx : clusters[cidx]) {
      const float* p = xyz + (size_t)idx * st;
      sx += p[0]; sy += p[1]; sz += p[2];
    }
    sums[3 * (size_t)cidx] = sx; sums[3 * (size_t)cidx + 1] = sy; sums[3 * (size_t)cidx + 2] = sz;
  }
  std::vector<int> order;
  prep_rank_clusters(clusters, sums.data(), order);
  for (int r = 0; r < nc; ++r)
    for (int idx : clusters[order[r]]) label_out[(size_t)idx * lst] = (float)(r + 1);
  if (n_clusters) *n_clusters = nc;
  return GORIO_OK;
}

int gorio_prep_radius_outlier_mask(int device, const float* xyz, int n, int point_stride_bytes, double radius, int min_neighbors, unsigned char* keep, int* n_kept) {
  if (!xyz || !keep || n <= 0 || point_stride_bytes < 12 || (point_stride_bytes % 4) || !(radius > 0.0) || min_neighbors < 0)
    return prep_fail(GORIO_ERR_INVALID, "radius_outlier_mask: bad arguments");
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "radius_outlier_mask", rc);
  if (!ctx) return rc;
  PrepCtx& c = *ctx;
  rc = prep_index_cloud(c, xyz, n, point_stride_bytes);
  if (rc) return rc;
  return prep_radius_outlier_keep(c, n, radius, min_neighbors, keep, n_kept);
}

int gorio_prep_statistical_outlier_mask(int device, const float* xyz, int n, int point_stride_bytes, int mean_k, double stddev_mul, unsigned char* keep, int* n_kept,
                                        float* mean_dist_out) {
  if (!xyz || !keep || n <= 0 || point_stride_bytes < 12 || (point_stride_bytes % 4) || mean_k < 1 || mean_k > 31)
    return prep_fail(GORIO_ERR_INVALID, "statistical_outlier_mask: bad arguments (mean_k must lie in [1, 31])");
  if (n < mean_k + 1) return prep_fail(GORIO_ERR_INVALID, kSorTooFew);
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "statistical_outlier_mask", rc);
  if (!ctx) return rc;
  PrepCtx& c = *ctx;
  rc = prep_index_cloud(c, xyz, n, point_stride_bytes);
  if (rc) return rc;
  return prep_statistical_outlier_keep(c, n, mean_k, stddev_mul, keep, n_kept, mean_dist_out);
}

int gorio_prep_voxel_downsample(int device, const float* xyz, int n, int point_stride_bytes, double leaf, float* xyz_out, int out_stride_bytes, int out_capacity, int* n_out) {
  if (!xyz || !xyz_out || !n_out || n <= 0 || point_stride_bytes < 12 || (point_stride_bytes % 4) || out_stride_bytes < 12 || (out_stride_bytes % 4) || !(leaf > 0.0))
    return prep_fail(GORIO_ERR_INVALID, "voxel_downsample: bad arguments");
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "voxel_downsample", rc);
  if (!ctx) return rc;
  PrepCtx& c = *ctx;
  // the scan-to-submap assembly with ONE frame and the identity pose is exactly pcl::VoxelGrid on that cloud (the float transform by
  // the identity returns every coordinate unchanged)
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  gorio_apd_keyframe fr;
  fr.xyz = xyz;
  fr.label = nullptr;
  fr.n = n;
  fr.point_stride_bytes = point_stride_bytes;
  fr.rel_pose = eye;
  int m = 0;
  rc = gorio_apd_set_target_submap(c.h, &fr, 1, leaf, &m);
  if (rc) return prep_fail(rc, c.h->err);
  *n_out = m;
  if (m > out_capacity) return prep_fail(GORIO_ERR_INVALID, "voxel_downsample: output capacity too small (n_out holds the size needed)");
  rc = gorio_apd_get_target_points(c.h, xyz_out, nullptr, m, out_stride_bytes);
  if (rc) return prep_fail(rc, c.h->err);
  return GORIO_OK;
}

// ---- pcl::ApproximateVoxelGrid (apd_approx_voxel.hip)
static int avg_check_common(int n, int n_fields, const double* leaf, float leaf_f[3], const int* n_out) {
  if (!n_out || !leaf || n < 0 || n > kAvgMaxPoints || n_fields < 3 || n_fields > kAvgMaxFields) return GORIO_ERR_INVALID;
  for (int a = 0; a < 3; ++a) {
    leaf_f[a] = (float)leaf[a];  // setLeafSize takes floats
    if (!std::isfinite(leaf[a]) || !(leaf_f[a] > 0.0f) || !std::isfinite(leaf_f[a])) return GORIO_ERR_INVALID;
  }
  return GORIO_OK;
}

// the launches, the 4-byte read-back and what it says; the context's handle holds the scratch
static int avg_run(PrepCtx& c, hipStream_t stream, const AvgCols& in, int n, int n_fields, const float leaf_f[3], const AvgColsOut& out, int capacity, int* n_out) {
  const int* d_n_out = nullptr;
  int m = 0;
  GORIO_HIP_CHECK(prep_fail, avg_enqueue(stream, c.h->avg, in, n, n_fields, leaf_f, out, capacity, &d_n_out));
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(&m, d_n_out, sizeof(int), hipMemcpyDeviceToHost, stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(stream));
  if (m < 0) {
    *n_out = 0;
    return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample: refused: a coordinate is not finite or a cell coordinate leaves (-2^30, 2^30)");
  }
  *n_out = m;
  if (m > capacity) return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample: output capacity too small (n_out holds the size needed)");
  return GORIO_OK;
}

int gorio_prep_approx_voxel_downsample(int device, const float* pts, int n, int stride_bytes, const int* field_offsets, int n_fields, const double leaf[3], float* out,
                                       int out_stride_bytes, int out_capacity, int* n_out) {
  float leaf_f[3];
  if (avg_check_common(n, n_fields, leaf, leaf_f, n_out) || !field_offsets || stride_bytes <= 0 || (stride_bytes % 4) || out_stride_bytes <= 0 || (out_stride_bytes % 4) ||
      out_capacity < 0 || (out_capacity > 0 && !out) || (n > 0 && !pts))
    return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample: bad arguments");
  const int st = stride_bytes / 4, ost = out_stride_bytes / 4;
  for (int f = 0; f < n_fields; ++f)
    if (field_offsets[f] < 0 || field_offsets[f] >= st || field_offsets[f] >= ost) return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample: a field offset lies outside the point");
  *n_out = 0;
  if (n == 0) return GORIO_OK;
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "approx_voxel_downsample", rc);
  if (!ctx) return rc;
  PrepCtx& c = *ctx;
  gorio_apd* h = c.h;
  GORIO_HIP_CHECK(prep_fail, hipSetDevice(device));
  AvgScratch& w = h->avg;
  const size_t need = (size_t)n * n_fields, grown = ((size_t)n + (size_t)n / 8) * kAvgMaxFields;
  GORIO_HIP_CHECK(prep_fail, w.stage_in.reserve(need, grown));
  GORIO_HIP_CHECK(prep_fail, w.stage_out.reserve(need, grown));
  std::vector<float> cols(need);  // columns [n_fields][n]
  for (int f = 0; f < n_fields; ++f) {
    const float* src = pts + field_offsets[f];
    float* dst = cols.data() + (size_t)f * n;
    for (int i = 0; i < n; ++i) dst[i] = src[(size_t)i * st];
  }
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(w.stage_in, cols.data(), sizeof(float) * need, hipMemcpyHostToDevice, h->stream));
  AvgCols in{};
  AvgColsOut oc{};
  for (int f = 0; f < n_fields; ++f) in.c[f] = w.stage_in + (size_t)f * n, oc.c[f] = w.stage_out + (size_t)f * n;
  in.stride = oc.stride = 1;
  rc = avg_run(c, h->stream, in, n, n_fields, leaf_f, oc, std::min(out_capacity, n), n_out);
  if (rc) return rc;
  const int m = *n_out;
  for (int f = 0; f < n_fields; ++f)
    GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(cols.data() + (size_t)f * n, oc.c[f], sizeof(float) * m, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(h->stream));
  for (int f = 0; f < n_fields; ++f) {
    const float* src = cols.data() + (size_t)f * n;
    float* dst = out + field_offsets[f];
    for (int i = 0; i < m; ++i) dst[(size_t)i * ost] = src[i];
  }
  return GORIO_OK;
}

int gorio_prep_approx_voxel_downsample_device(int device, const float* const* cols, int n_fields, int n, const double leaf[3], float* const* cols_out, int capacity, int* n_out,
                                              void* stream) {
  float leaf_f[3];
  if (avg_check_common(n, n_fields, leaf, leaf_f, n_out) || capacity < 0 || (n > 0 && !cols) || (capacity > 0 && !cols_out))
    return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample_device: bad arguments");
  AvgCols in{};
  AvgColsOut oc{};
  for (int f = 0; f < n_fields; ++f) {
    if ((n > 0 && !cols[f]) || (capacity > 0 && !cols_out[f])) return prep_fail(GORIO_ERR_INVALID, "approx_voxel_downsample_device: a column pointer is NULL");
    in.c[f] = n > 0 ? cols[f] : nullptr;
    oc.c[f] = capacity > 0 ? cols_out[f] : nullptr;
  }
  in.stride = oc.stride = 1;
  *n_out = 0;
  if (n == 0) return GORIO_OK;
  int rc = GORIO_OK;
  PrepCtx* ctx = prep_context(device, "approx_voxel_downsample_device", rc);
  if (!ctx) return rc;
  GORIO_HIP_CHECK(prep_fail, hipSetDevice(device));
  return avg_run(*ctx, static_cast<hipStream_t>(stream), in, n, n_fields, leaf_f, oc, capacity, n_out);
}

}  // extern "C"

// ----------------------------------------------------------------------------------------------- REVE (include/gorio_prep.h)
namespace {

void host_ldlt3_solve(const double* A_in, const double* rhs, double* x) {  // Eigen::LDLT<3x3>: the 6 x 6 routine of the kernels, n = 3
  double A[9];
  int perm[3] = {0, 1, 2};
  std::memcpy(A, A_in, sizeof(A));
  for (int k = 0; k < 3; ++k) {
    int piv = k;
    double best = std::fabs(A[k * 3 + k]);
    for (int i = k + 1; i < 3; ++i)
      if (std::fabs(A[i * 3 + i]) > best) {
        best = std::fabs(A[i * 3 + i]);
        piv = i;
      }
    if (piv != k) {
      for (int c = 0; c < 3; ++c) std::swap(A[k * 3 + c], A[piv * 3 + c]);
      for (int r = 0; r < 3; ++r) std::swap(A[r * 3 + k], A[r * 3 + piv]);
      std::swap(perm[k], perm[piv]);
    }
    const double d = A[k * 3 + k];
    if (d == 0.0) continue;
    double col[3];
    for (int i = k + 1; i < 3; ++i) col[i] = A[i * 3 + k];
    for (int i = k + 1; i < 3; ++i) {
      const double l = col[i] / d;
      for (int j = k + 1; j <= i; ++j) A[i * 3 + j] -= l * col[j];
      A[i * 3 + k] = l;
    }
    for (int i = k + 1; i < 3; ++i)
      for (int j = i + 1; j < 3; ++j) A[i * 3 + j] = A[j * 3 + i];
  }
  double y[3];
  for (int i = 0; i < 3; ++i) y[i] = rhs[perm[i]];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < i; ++j) y[i] -= A[i * 3 + j] * y[j];
  for (int i = 0; i < 3; ++i) y[i] = (A[i * 3 + i] != 0.0) ? y[i] / A[i * 3 + i] : 0.0;
  for (int i = 2; i >= 0; --i)
    for (int j = i + 1; j < 3; ++j) y[i] -= A[j * 3 + i] * y[j];
  for (int i = 0; i < 3; ++i) x[perm[i]] = y[i];
}

struct ReveCtx {  // per thread; move-assigning a new one frees what the old one held
  int device = -1;
  hipStream_t stream = nullptr;
  DevBuf<float> d_in;  // d_in, d_f, d_fv, d_valid and d_out: one group of capacity `cap` (targets)
  DevBuf<double> d_f, d_fv, d_out;
  DevBuf<unsigned char> d_valid;
  size_t cap = 0;
  DevBuf<unsigned char> d_flags;
  DevBuf<double> d_v;
};
thread_local ReveCtx g_reve;

struct ReveFrame {  // what the gates of REVE:75-90 left of one scan: the rows of the valid targets, in input order
  int n = 0, m = 0;
  std::vector<int> vidx;    // [m] input index of each valid target
  std::vector<double> fv;   // [m][4] x/r, y/r, z/r, corrected doppler
};

// the context becomes this device's, with room for n targets
int reve_prepare(ReveCtx& c, int device, int n) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: no usable HIP device (there is no CPU fallback)");
  if (device < 0 || device >= ndev) return prep_fail(GORIO_ERR_INVALID, "ego_velocity: bad device ordinal");
  if (c.device >= 0 && c.device != device) {  // a context of another device: a plain reset, its buffers free on their own device
    hipSetDevice(c.device);
    c = ReveCtx();
  }
  GORIO_HIP_CHECK(prep_fail, hipSetDevice(device));
  if (c.device < 0) {  // a context becomes this device's only once it is complete
    c.stream = device_stream(device);
    if (!c.stream) return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: no stream");
    GORIO_HIP_CHECK(prep_fail, c.d_v.reserve(3 * 64));
    c.device = device;
  }
  const size_t cap = (size_t)n + n / 8;
  GORIO_HIP_CHECK(prep_fail, reserve_group(c.cap, n, cap, c.d_in, 5 * cap, c.d_f, 4 * cap, c.d_fv, 4 * cap, c.d_valid, cap, c.d_out, 10 * (cap / 256 + 2)));
  return GORIO_OK;
}

// REVE:75-90 for n targets on the device (px / py / pz / inten / dop with `stride` floats between targets): features and gates there,
// the rows of the valid targets collected here
ReveCfg reve_device_cfg(const gorio_reve_config* cfg) {
  ReveCfg rc;
  rc.min_dist = cfg->min_dist; rc.max_dist = cfg->max_dist; rc.min_db = cfg->min_db;
  rc.az_lim = (double)cfg->azimuth_thresh_deg * M_PI / 180.0; rc.el_lim = (double)cfg->elevation_thresh_deg * M_PI / 180.0;  // angles::from_degrees
  rc.doppler_factor_unused = 0; rc.doppler_factor = cfg->doppler_velocity_correction_factor; rc.pad_ = 0;
  return rc;
}
// the rows of the valid targets, in input order, from what the features kernel left (f[n][4], valid[n])
void reve_collect(ReveFrame& fr, const std::vector<double>& f, const std::vector<unsigned char>& valid, int n) {
  fr.n = n;
  fr.vidx.clear();
  fr.fv.clear();
  for (int i = 0; i < n; ++i)
    if (valid[i]) {
      fr.vidx.push_back(i);
      fr.fv.insert(fr.fv.end(), f.begin() + 4 * (size_t)i, f.begin() + 4 * (size_t)i + 4);
    }
  fr.m = (int)fr.vidx.size();
}
int reve_features(ReveCtx& c, const float* px, const float* py, const float* pz, const float* inten, const float* dop, int stride, int n, const gorio_reve_config* cfg, ReveFrame& fr) {
  const ReveCfg rc = reve_device_cfg(cfg);
  reve_features_kernel<<<(n + 255) / 256, 256, 0, c.stream>>>(px, py, pz, inten, dop, stride, n, rc, c.d_f, c.d_valid);
  GORIO_HIP_CHECK(prep_fail, hipGetLastError());
  std::vector<double> f((size_t)n * 4);
  std::vector<unsigned char> valid((size_t)n);
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(f.data(), c.d_f, sizeof(double) * f.size(), hipMemcpyDeviceToHost, c.stream));
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(valid.data(), c.d_valid, (size_t)n, hipMemcpyDeviceToHost, c.stream));
  GORIO_HIP_CHECK(prep_fail, hipStreamSynchronize(c.stream));
  reve_collect(fr, f, valid, n);
  return GORIO_OK;
}

// REVE:92-170 over the valid targets of `fr`: zero-velocity test, least squares, RANSAC.  One solve is advanced in phases, so that a batch
// (apd_scan_batch.hip) can put the launches of many solves into one: a phase does its host part, enqueues its uploads on the context's
// stream and names the launch it wants (`want`); after that launch, reve_solve_download and a synchronisation, reve_solve_advance does
// the next host part.  reve_solve below drives one solve with the single kernels.
struct ReveSolve {
  ReveCtx* c = nullptr;
  const gorio_reve_config* cfg = nullptr;
  const ReveFrame* fr = nullptr;
  const unsigned int* sample_idx = nullptr;
  int n_iter = 0;
  double *v_r = nullptr, *sigma_v_r = nullptr;
  unsigned char *inlier_mask = nullptr, *outlier_mask = nullptr;
  int* zero_velocity = nullptr;
  int ok = 0;
  enum Want { DONE = 0, EVAL = 1, SUMS = 2 };
  int want = DONE;
  int K = 0;     // EVAL: hypotheses; flags[K][m] come back
  int pass = 0;  // SUMS: 0 = H^T H and H^T y of the selected rows, 1 = the same with e^T e for v_r
  int rows = 0;  // SUMS: selected rows
  bool ransac = false;
  std::vector<double> vs, part;
  std::vector<unsigned char> flags, sel, best_out;
  size_t nbo = 0;
};

// solve3DFull (REVE:252-303) over the valid rows selected by S.sel: sums on the device (two SUMS launches), 3 x 3 algebra on the host
int reve_solve_start_sums(ReveSolve& S) {
  ReveCtx& c = *S.c;
  const int m = S.fr->m, nb = (m + 255) / 256;
  if (hipMemcpyAsync(c.d_valid, S.sel.data(), (size_t)m, hipMemcpyHostToDevice, c.stream) != hipSuccess) return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: device error");
  S.part.assign((size_t)nb * 10, 0.0);
  S.pass = 0;
  S.want = ReveSolve::SUMS;
  return GORIO_OK;
}

void reve_solve_finish(ReveSolve& S, bool solved) {
  const int m = S.fr->m;
  const std::vector<int>& vidx = S.fr->vidx;
  if (solved) {
    S.ok = 1;  // REVE:301: true whatever the sigma test said
    if (S.inlier_mask)
      for (int j = 0; j < m; ++j)
        if (S.sel[j]) S.inlier_mask[vidx[j]] = 1;
  }
  if (S.ransac && S.outlier_mask && S.nbo > 0)
    for (int j = 0; j < m; ++j)
      if (S.best_out[j]) S.outlier_mask[vidx[j]] = 1;
  S.want = ReveSolve::DONE;
}

int reve_solve_begin(ReveSolve& S) {
  ReveCtx& c = *S.c;
  const gorio_reve_config* cfg = S.cfg;
  const int n = S.fr->n, m = S.fr->m;
  const std::vector<int>& vidx = S.fr->vidx;
  const std::vector<double>& fv = S.fr->fv;
  double *v_r = S.v_r, *sigma_v_r = S.sigma_v_r;
  if (S.inlier_mask) std::memset(S.inlier_mask, 0, (size_t)n);
  if (S.outlier_mask) std::memset(S.outlier_mask, 0, (size_t)n);
  v_r[0] = v_r[1] = v_r[2] = 0.0;
  sigma_v_r[0] = sigma_v_r[1] = sigma_v_r[2] = 0.0;
  if (S.zero_velocity) *S.zero_velocity = 0;
  S.ok = 0;
  S.want = ReveSolve::DONE;
  if (m <= 2) return GORIO_OK;
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(c.d_fv, fv.data(), sizeof(double) * fv.size(), hipMemcpyHostToDevice, c.stream));
  std::vector<double> vd((size_t)m);
  for (int k = 0; k < m; ++k) vd[k] = std::fabs(fv[4 * (size_t)k + 3]);
  const size_t nth = std::min((size_t)((double)m * (1.0 - (double)cfg->allowed_outlier_percentage)), (size_t)m - 1);
  std::nth_element(vd.begin(), vd.begin() + nth, vd.end());  // REVE:105-108
  if (vd[nth] < cfg->thresh_zero_velocity) {                 // REVE:110-121
    if (S.zero_velocity) *S.zero_velocity = 1;
    sigma_v_r[0] = cfg->sigma_zero_velocity_x; sigma_v_r[1] = cfg->sigma_zero_velocity_y; sigma_v_r[2] = cfg->sigma_zero_velocity_z;
    if (S.inlier_mask)
      for (int k = 0; k < m; ++k)
        if (std::fabs(fv[4 * (size_t)k + 3]) < cfg->thresh_zero_velocity) S.inlier_mask[vidx[k]] = 1;
    S.ok = 1;
    return GORIO_OK;
  }
  if (!cfg->use_ransac) {
    S.sel.assign((size_t)m, 1);
    S.rows = m;
    return reve_solve_start_sums(S);
  }
  // solve3DFullRansac, REVE:172-250
  S.ransac = true;
  S.nbo = 0;
  const int K = m >= cfg->n_ransac_points ? S.n_iter : 0;
  S.K = K;
  if (K <= 0) {
    reve_solve_finish(S, false);
    return GORIO_OK;
  }
  if (K > 64) return prep_fail(GORIO_ERR_INVALID, "ego_velocity: more than 64 RANSAC iterations");
  std::vector<double>& vs = S.vs;
  vs.assign((size_t)K * 3, 0.0);
  for (int k = 0; k < K; ++k) {  // the sample systems are N_ransac_points rows: solved here (3 x 3)
    double HTH[9] = {0}, HTy[3] = {0};
    for (int q = 0; q < cfg->n_ransac_points; ++q) {
      const unsigned int row = S.sample_idx[(size_t)k * cfg->n_ransac_points + q];
      if (row >= (unsigned int)m) return prep_fail(GORIO_ERR_INVALID, "ego_velocity: sample index outside the valid targets");
      const double* r = fv.data() + 4 * (size_t)row;
      for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) HTH[a * 3 + b] += r[a] * r[b];
        HTy[a] += r[a] * r[3];
      }
    }
    host_ldlt3_solve(HTH, HTy, vs.data() + 3 * (size_t)k);
  }
  GORIO_HIP_CHECK(prep_fail, c.d_flags.reserve((size_t)K * m, (size_t)K * m + 1024));
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(c.d_v, vs.data(), sizeof(double) * vs.size(), hipMemcpyHostToDevice, c.stream));
  S.flags.assign((size_t)K * m, 0);
  S.want = ReveSolve::EVAL;
  return GORIO_OK;
}

// what the launch named by S.want left, on its way to the host; the caller synchronises the stream before reve_solve_advance
int reve_solve_download(ReveSolve& S) {
  ReveCtx& c = *S.c;
  if (S.want == ReveSolve::EVAL) {
    GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(S.flags.data(), c.d_flags, S.flags.size(), hipMemcpyDeviceToHost, c.stream));
  } else if (S.want == ReveSolve::SUMS) {
    if (hipMemcpyAsync(S.part.data(), c.d_out, sizeof(double) * S.part.size(), hipMemcpyDeviceToHost, c.stream) != hipSuccess)
      return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: device error");
  }
  return GORIO_OK;
}

int reve_solve_advance(ReveSolve& S) {
  ReveCtx& c = *S.c;
  const gorio_reve_config* cfg = S.cfg;
  const int m = S.fr->m;
  double *v_r = S.v_r, *sigma = S.sigma_v_r;
  if (S.want == ReveSolve::EVAL) {
    const int K = S.K;
    const std::vector<double>& vs = S.vs;
    std::vector<unsigned char> best_in;
    size_t nbi = 0;
    for (int k = 0; k < K; ++k) {
      const unsigned char* fl = S.flags.data() + (size_t)k * m;
      size_t ni = 0;
      for (int j = 0; j < m; ++j) ni += fl[j];
      size_t no = (size_t)m - ni;
      std::vector<unsigned char> cur_in(fl, fl + m), cur_out((size_t)m);
      for (int j = 0; j < m; ++j) cur_out[j] = !fl[j];
      if ((float)no / (float)(ni + no) > 0.05) {  // REVE:215-220
        std::fill(cur_in.begin(), cur_in.end(), 1);
        std::fill(cur_out.begin(), cur_out.end(), 0);
        ni = (size_t)m;
        no = 0;
      }
      if (ni > nbi) { best_in = cur_in; nbi = ni; }
      if (no > S.nbo) { S.best_out = cur_out; S.nbo = no; }
      v_r[0] = vs[3 * (size_t)k]; v_r[1] = vs[3 * (size_t)k + 1]; v_r[2] = vs[3 * (size_t)k + 2];
    }
    if (nbi == 0) {
      reve_solve_finish(S, false);
      return GORIO_OK;
    }
    S.sel = best_in;
    S.rows = (int)nbi;
    return reve_solve_start_sums(S);
  }
  if (S.want == ReveSolve::SUMS) {
    const int nb = (m + 255) / 256;
    double s[10];
    for (int q = 0; q < 10; ++q) s[q] = 0.0;
    for (int b = 0; b < nb; ++b)
      for (int q = 0; q < 10; ++q) s[q] += S.part[(size_t)b * 10 + q];
    if (S.pass == 0) {
      const double HTH[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]}, HTy[3] = {s[6], s[7], s[8]};
      host_ldlt3_solve(HTH, HTy, v_r);  // use_cholesky_instead_of_bdcsvd = true: (HTH).ldlt().solve(H^T y), REVE:272
      if (hipMemcpyAsync(c.d_v, v_r, sizeof(double) * 3, hipMemcpyHostToDevice, c.stream) != hipSuccess) return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: device error");
      S.pass = 1;
      return GORIO_OK;  // want stays SUMS
    }
    {  // REVE:278-290
      const double H0 = s[0], H1 = s[1], H2 = s[2], H4 = s[3], H5 = s[4], H8 = s[5];
      const double c00 = H4 * H8 - H5 * H5, c01 = H5 * H2 - H1 * H8, c02 = H1 * H5 - H4 * H2;
      const double det = H0 * c00 + H1 * c01 + H2 * c02;
      const double sc = s[9] / (double)(S.rows - 3);
      double sg[3] = {sc * (c00 / det), sc * ((H0 * H8 - H2 * H2) / det), sc * ((H0 * H4 - H1 * H1) / det)};
      sigma[0] = sg[0]; sigma[1] = sg[1]; sigma[2] = sg[2];
      if (sg[0] >= 0.0 && sg[1] >= 0.0 && sg[2] >= 0.0) {
        sigma[0] = std::sqrt(sg[0]) + cfg->sigma_offset_radar_x;
        sigma[1] = std::sqrt(sg[1]) + cfg->sigma_offset_radar_y;
        sigma[2] = std::sqrt(sg[2]) + cfg->sigma_offset_radar_z;
      }
    }
    reve_solve_finish(S, true);
  }
  return GORIO_OK;
}

int reve_solve(ReveCtx& c, const gorio_reve_config* cfg, const ReveFrame& fr, const unsigned int* sample_idx, int n_iter, double v_r[3], double sigma_v_r[3],
               unsigned char* inlier_mask, unsigned char* outlier_mask, int* zero_velocity, int* success) {
  ReveSolve S;
  S.c = &c; S.cfg = cfg; S.fr = &fr; S.sample_idx = sample_idx; S.n_iter = n_iter; S.v_r = v_r; S.sigma_v_r = sigma_v_r;
  S.inlier_mask = inlier_mask; S.outlier_mask = outlier_mask; S.zero_velocity = zero_velocity;
  int rc = reve_solve_begin(S);
  if (rc) return rc;
  const int m = fr.m, nb = (m + 255) / 256;
  while (S.want != ReveSolve::DONE) {
    if (S.want == ReveSolve::EVAL) {
      reve_eval_kernel<<<dim3(nb, S.K), 256, 0, c.stream>>>(c.d_fv, m, c.d_v, (double)cfg->inlier_thresh, c.d_flags);
      GORIO_HIP_CHECK(prep_fail, hipGetLastError());
    } else {
      reve_sums_kernel<<<nb, 256, 0, c.stream>>>(c.d_fv, m, c.d_valid, S.pass == 1 ? c.d_v.get() : nullptr, c.d_out);
    }
    rc = reve_solve_download(S);
    if (rc) return rc;
    if (hipStreamSynchronize(c.stream) != hipSuccess) return prep_fail(GORIO_ERR_NO_DEVICE, "ego_velocity: device error");
    rc = reve_solve_advance(S);
    if (rc) return rc;
  }
  if (success) *success = S.ok;
  return GORIO_OK;
}

}  // namespace

extern "C" {

void gorio_prep_reve_default_config(gorio_reve_config* c) {  // radar_ego_velocity_estimator.h:30-60
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->min_dist = 1; c->max_dist = 400; c->min_db = 0; c->elevation_thresh_deg = 22.5f; c->azimuth_thresh_deg = 56.5f; c->doppler_velocity_correction_factor = 1;
  c->thresh_zero_velocity = 0.05f; c->allowed_outlier_percentage = 0.30f; c->sigma_zero_velocity_x = 1.0e-03f; c->sigma_zero_velocity_y = 3.2e-03f; c->sigma_zero_velocity_z = 1.0e-02f;
  c->max_sigma_x = 0.2f; c->max_sigma_y = 0.2f; c->max_sigma_z = 0.2f; c->inlier_thresh = 0.5f; c->use_ransac = 1; c->n_ransac_points = 5;
  c->outlier_prob = 0.05f; c->success_prob = 0.995f;
}

int gorio_prep_reve_ransac_iterations(const gorio_reve_config* c) {  // setRansacIter, radar_ego_velocity_estimator.h:138-141
  if (!c) return 0;
  return (int)(unsigned int)((std::log(1.0 - c->success_prob)) / std::log(1.0 - std::pow(1.0 - c->outlier_prob, (float)c->n_ransac_points)));
}

int gorio_prep_ego_velocity(int device, const float* xyz, const float* intensity, const float* doppler, int n, int stride_bytes, const gorio_reve_config* cfg,
                            const unsigned int* sample_idx, int n_iter, double v_r[3], double sigma_v_r[3], unsigned char* inlier_mask, unsigned char* outlier_mask,
                            int* n_valid, int* zero_velocity, int* success) {
  if (!xyz || !intensity || !doppler || !cfg || !v_r || !sigma_v_r || n <= 0 || stride_bytes < 4 || (stride_bytes % 4) || n_iter < 0 || (n_iter > 0 && !sample_idx) || cfg->n_ransac_points < 3 || cfg->n_ransac_points > 64)
    return prep_fail(GORIO_ERR_INVALID, "ego_velocity: bad arguments");
  ReveCtx& c = g_reve;
  int rc = reve_prepare(c, device, n);
  if (rc) return rc;
  // ---- per-target features on the device
  const int st = stride_bytes / 4;
  std::vector<float> in((size_t)n * 5);
  for (int i = 0; i < n; ++i) {
    in[5 * (size_t)i] = xyz[(size_t)i * st]; in[5 * (size_t)i + 1] = xyz[(size_t)i * st + 1]; in[5 * (size_t)i + 2] = xyz[(size_t)i * st + 2];
    in[5 * (size_t)i + 3] = intensity[(size_t)i * st]; in[5 * (size_t)i + 4] = doppler[(size_t)i * st];
  }
  GORIO_HIP_CHECK(prep_fail, hipMemcpyAsync(c.d_in, in.data(), sizeof(float) * in.size(), hipMemcpyHostToDevice, c.stream));
  ReveFrame fr;
  rc = reve_features(c, c.d_in, c.d_in + 1, c.d_in + 2, c.d_in + 3, c.d_in + 4, 5, n, cfg, fr);
  if (rc) return rc;
  if (n_valid) *n_valid = fr.m;
  return reve_solve(c, cfg, fr, sample_idx, n_iter, v_r, sigma_v_r, inlier_mask, outlier_mask, zero_velocity, success);
}

}  // extern "C"
