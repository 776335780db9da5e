// apd_scan.hip -- the preprocessing nodelet's whole cloud_callback (preprocessing_nodelet_ntu.cpp:370-581, "PREP") as one device-resident
// pipeline: include/gorio_scan.h.  Kernels first, the host side below them.  Included at the end of apd_api.hip, after apd_prep.hip:
// the search stages run through the internal entry points of apd_prep.hip and apd_ground.hip that start from a cloud on the device.
//
// A cloud is five float columns (x, y, z, intensity, doppler) and one int column `map` (the index of each point in the gated cloud;
// in the gated cloud itself: in the raw message).  Every stage writes a cloud of its own, so any stage can be read back afterwards
// (gorio_scan_get_stage).  Stages that drop points produce a keep mask and share ONE order-preserving compaction.
//
// Arithmetic: the elementwise kernels must give the bits of tests/scan_pipeline_restatement.py.  Floating-point contraction is OFF for
// this file -- the library's Makefile passes -ffp-contract=off, and the pragma below repeats it for a build that does not -- so every
// * and + here is one correctly rounded operation in the order written.
#include <hip/hip_runtime.h>

#include "../../include/gorio_scan.h"

#pragma clang fp contract(off)

namespace gorio {

struct ScanColumns {  // one stage's input and output columns
  const float* s[5];
  float* d[5];
  const int* smap;  // nullptr: the identity (the source IS the gated cloud, or the raw message)
  int* dmap;
};

// ---------------------------------------------------------------------------------------------- gate and rotate (PREP:381-412)
// In place on the uploaded columns.  keep[i] = power > threshold and x, y, z finite (the reference's NAN / INFINITY comparisons drop
// nothing but +Inf; dropping NaN and -Inf too is the documented deviation).  Rotation: double, ((r0 x + r1 y) + r2 z), one rounding to
// float.  grid ceil(n / 256), block 256.
struct GateArgs {
  double R[9];
  float power_threshold;
};
// Every kernel of this file is a per-workgroup body, `block` its 256-point block, and a __global__ that hands it blockIdx.x; the job-table
// kernels of apd_scan_batch.hip hand the same bodies the block of a (job, block) entry.
__device__ __forceinline__ void scan_gate_rotate_body(float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, const float* __restrict__ power, int n, const GateArgs& a,
                                                      unsigned char* __restrict__ keep, int block) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  const float fx = x[i], fy = y[i], fz = z[i];
  const bool ok = power[i] > a.power_threshold && isfinite(fx) && isfinite(fy) && isfinite(fz);
  keep[i] = ok ? 1 : 0;
  if (!ok) return;
  const double dx = fx, dy = fy, dz = fz;
  x[i] = (float)((a.R[0] * dx + a.R[1] * dy) + a.R[2] * dz);
  y[i] = (float)((a.R[3] * dx + a.R[4] * dy) + a.R[5] * dz);
  z[i] = (float)((a.R[6] * dx + a.R[7] * dy) + a.R[8] * dz);
}
__global__ __launch_bounds__(256) void scan_gate_rotate_kernel(float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, const float* __restrict__ power, int n, GateArgs a,
                                                               unsigned char* __restrict__ keep) {
  scan_gate_rotate_body(x, y, z, power, n, a, keep, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- deskew (PREP:705-716)
// Operation order, all float unless said otherwise (w = -ang_vel rounded to float FIRST, then negated: Vector3f ang_v(...); ang_v *= -1):
//   delta_t = (scan_period * double(i)) / double(size)                         double
//   qx, qy, qz = float((delta_t / 2.0) * double(w_k))                          one rounding each; qw = 1
//   n2 = ((qx qx + qy qy) + qz qz) + qw qw                                      Quaternion::squaredNorm, scalar order
//   inverse = conjugate / n2:  ix = -qx / n2, iy = -qy / n2, iz = -qz / n2, iw = qw / n2
//   uv = i.vec x v   (cross: a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);  uv = uv + uv
//   out = (v + iw * uv) + i.vec x uv                                            Eigen's QuaternionBase::_transformVector
// intensity, doppler and map pass through.  grid ceil(n / 256), block 256.
__device__ __forceinline__ void scan_deskew_body(const ScanColumns& c, int n, double scan_period, float wx, float wy, float wz, int block) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  const double delta_t = scan_period * (double)i / (double)n;
  const double half = delta_t / 2.0;
  const float qx = (float)(half * (double)wx), qy = (float)(half * (double)wy), qz = (float)(half * (double)wz), qw = 1.0f;
  const float n2 = ((qx * qx + qy * qy) + qz * qz) + qw * qw;
  const float ix = -qx / n2, iy = -qy / n2, iz = -qz / n2, iw = qw / n2;
  const float vx = c.s[0][i], vy = c.s[1][i], vz = c.s[2][i];
  float ux = iy * vz - iz * vy, uy = iz * vx - ix * vz, uz = ix * vy - iy * vx;
  ux = ux + ux;
  uy = uy + uy;
  uz = uz + uz;
  const float cx = iy * uz - iz * uy, cy = iz * ux - ix * uz, cz = ix * uy - iy * ux;
  c.d[0][i] = (vx + iw * ux) + cx;
  c.d[1][i] = (vy + iw * uy) + cy;
  c.d[2][i] = (vz + iw * uz) + cz;
  c.d[3][i] = c.s[3][i];
  c.d[4][i] = c.s[4][i];
  c.dmap[i] = c.smap ? c.smap[i] : i;
}
__global__ __launch_bounds__(256) void scan_deskew_kernel(ScanColumns c, int n, double scan_period, float wx, float wy, float wz) {
  scan_deskew_body(c, n, scan_period, wx, wy, wz, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- distance filter (PREP:643-647)
// d = double(sqrtf((x x + y y) + z z)) (getVector3fMap().norm()), z widened to double; all four inequalities strict.
struct DistanceArgs {
  double near_, far_, z_low, z_high;
};
__device__ __forceinline__ void scan_distance_body(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, const DistanceArgs& a,
                                                   unsigned char* __restrict__ keep, int block) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  const float fx = x[i], fy = y[i], fz = z[i];
  const double d = (double)sqrtf((fx * fx + fy * fy) + fz * fz), zd = (double)fz;
  keep[i] = (d > a.near_ && d < a.far_ && zd < a.z_high && zd > a.z_low) ? 1 : 0;
}
__global__ __launch_bounds__(256) void scan_distance_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z, int n, DistanceArgs a,
                                                            unsigned char* __restrict__ keep) {
  scan_distance_body(x, y, z, n, a, keep, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- order-preserving compaction
// Three launches, no workgroup ever waits for another: (1) per workgroup the number of kept points, from one ballot + popcount per wave;
// (2) ONE workgroup scans the workgroup counts (exclusive, in place) and leaves the total behind them; (3) every workgroup repeats its
// ballots and scatters: position = workgroup offset + kept points of the lower waves + kept lanes below this one.
// `out`: where this workgroup's count goes
__device__ __forceinline__ void compact_count_body(const unsigned char* __restrict__ keep, int n, int* __restrict__ out, int block) {
  const int i = block * 256 + threadIdx.x;
  const bool k = i < n && keep[i];
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) *out = (w[0] + w[1]) + (w[2] + w[3]);
}
__global__ __launch_bounds__(256) void compact_count_kernel(const unsigned char* __restrict__ keep, int n, int* __restrict__ bcnt) {
  compact_count_body(keep, n, bcnt + blockIdx.x, blockIdx.x);
}

// (2) is block_scan_kernel of apd_voxel_group.hip, which the cell groupings share.

// `boff`: the position of this workgroup's first kept point in the output
__device__ __forceinline__ void compact_scatter_body(const ScanColumns& c, const unsigned char* __restrict__ keep, int n, int boff, int block) {
  const int i = block * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool k = i < n && keep[i];
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if (lane == 0) w[wave] = __popcll(b);
  __syncthreads();
  if (!k) return;
  int pos = boff + __popcll(b & ((1ull << lane) - 1ull));
  for (int q = 0; q < wave; ++q) pos += w[q];
#pragma unroll
  for (int q = 0; q < 5; ++q) c.d[q][pos] = c.s[q][i];
  c.dmap[pos] = c.smap ? c.smap[i] : i;
}
__global__ __launch_bounds__(256) void compact_scatter_kernel(ScanColumns c, const unsigned char* __restrict__ keep, int n, const int* __restrict__ boffs) {
  compact_scatter_body(c, keep, n, boffs[blockIdx.x], blockIdx.x);
}

// ---------------------------------------------------------------------------------------------- ground + nonground order (PREP:518)
// out[j] = in[order[j]], every column.  grid ceil(m / 256), block 256; order[j] < the source size (checked on the host before the upload).
__device__ __forceinline__ void scan_permute_body(const ScanColumns& c, const int* __restrict__ order, int m, int block) {
  const int j = block * 256 + threadIdx.x;
  if (j >= m) return;
  const int i = order[j];
#pragma unroll
  for (int q = 0; q < 5; ++q) c.d[q][j] = c.s[q][i];
  c.dmap[j] = c.smap ? c.smap[i] : i;
}
__global__ __launch_bounds__(256) void scan_permute_kernel(ScanColumns c, const int* __restrict__ order, int m) { scan_permute_body(c, order, m, blockIdx.x); }

// the labels of the DBSCAN stage into the registration cloud the stage indexed (label column and the w of the packed points)
__device__ __forceinline__ void scan_set_labels_body(const float* __restrict__ lab, int n, float* __restrict__ label, float4* __restrict__ p4, int block) {
  const int i = block * 256 + threadIdx.x;
  if (i >= n) return;
  label[i] = lab[i];
  p4[i].w = lab[i];
}
__global__ __launch_bounds__(256) void scan_set_labels_kernel(const float* __restrict__ lab, int n, float* __restrict__ label, float4* __restrict__ p4) {
  scan_set_labels_body(lab, n, label, p4, blockIdx.x);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_scan.h)
namespace {
thread_local std::string g_scan_err;
int scan_fail(int code, const std::string& m) {
  g_scan_err = m;
  return code;
}

struct ScanCloud {
  DevBuf<float> f;  // five columns of `cap` floats
  DevBuf<int> map;
  size_t cap = 0;
  int n = 0;
  bool identity = false;  // the upload: a point's index is its position
  bool is_gated = false;  // the gated cloud: its map holds RAW indices; for the stages after it a point's index is its position
  float* col(int q) const { return f.get() + (size_t)q * cap; }
};

enum { kScanRaw = 0, kScanClouds = 1 + GORIO_SCAN_STAGE_COUNT };  // cloud 0: the upload, gated in place; cloud 1 + s: what stage s put out
struct ScanBatchLead;  // apd_scan_batch.hip: what the lead handle of a batch holds for it
}  // namespace

struct gorio_scan {
  int device = 0;
  hipStream_t stream = nullptr;
  gorio_scan_params p;
  gorio_ground* ground = nullptr;
  PrepCtx prep;    // the registration handle whose source is the cloud a search stage indexes
  ReveCtx reve;
  ReveFrame frame;
  ScanCloud cl[kScanClouds];
  const ScanCloud* stage_cloud[GORIO_SCAN_STAGE_COUNT];  // nullptr: not reached; a stage that changes nothing names its input
  DevBuf<unsigned char> d_keep;  // d_keep, d_bcnt, d_order, d_lab: one group of capacity aux_cap (points)
  DevBuf<int> d_bcnt, d_order;
  DevBuf<float> d_lab;
  size_t aux_cap = 0;
  DevBuf<int> d_members, d_coffs;  // cluster members (CSR) and the sums kernel's output
  DevBuf<float> d_sums;
  int n_raw = 0;
  bool on_device = false;  // stream, segmenter and registration handle exist (made by the first load)
  bool loaded = false, have_output = false;
  int n_out = 0;
  long long point_uploads = 0, index_builds = 0, point_downloads = 0;
  std::string run_err;                  // the text of the last run when it ended REFUSED, "" otherwise (gorio_scan_handle_error)
  std::shared_ptr<ScanBatchLead> batch;  // made by the first batch call that names this handle first
};

namespace {

int scan_reserve(gorio_scan* h, int n) {
  const size_t need = (size_t)std::max(n, 1), cap = need + need / 8 + 64;
  for (ScanCloud& c : h->cl) GORIO_HIP_CHECK(scan_fail, reserve_group(c.cap, need, cap, c.f, 5 * cap, c.map, cap));
  GORIO_HIP_CHECK(scan_fail, reserve_group(h->aux_cap, need, cap, h->d_keep, cap, h->d_bcnt, cap / 256 + 4, h->d_order, cap, h->d_lab, cap));
  return GORIO_OK;
}

gorio::ScanColumns scan_columns(const ScanCloud& src, ScanCloud& dst) {
  gorio::ScanColumns c;
  for (int q = 0; q < 5; ++q) {
    c.s[q] = src.col(q);
    c.d[q] = dst.col(q);
  }
  c.smap = (src.identity || src.is_gated) ? nullptr : src.map.get();
  c.dmap = dst.map;
  return c;
}

// dst = the points of src whose keep byte (h->d_keep) is set, in order; dst.n from the device
int scan_compact(gorio_scan* h, const ScanCloud& src, ScanCloud& dst) {
  const int n = src.n, nb = (n + 255) / 256;
  gorio::compact_count_kernel<<<nb, 256, 0, h->stream>>>(h->d_keep, n, h->d_bcnt);
  gorio::block_scan_kernel<<<1, 1024, 0, h->stream>>>(h->d_bcnt, nb);
  gorio::compact_scatter_kernel<<<nb, 256, 0, h->stream>>>(scan_columns(src, dst), h->d_keep, n, h->d_bcnt);
  GORIO_HIP_CHECK(scan_fail, hipGetLastError());
  int total = 0;
  GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(&total, h->d_bcnt.get() + nb, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));
  dst.n = total;
  dst.identity = false;
  return GORIO_OK;
}

int scan_upload_keep(gorio_scan* h, const std::vector<unsigned char>& keep) {
  GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_keep, keep.data(), keep.size(), hipMemcpyHostToDevice, h->stream));
  GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));  // keep is pageable and dies with the caller's scope
  return GORIO_OK;
}

int scan_check_params(const gorio_scan_params& p) {
  for (double r : p.rotation)
    if (!std::isfinite(r)) return scan_fail(GORIO_ERR_INVALID, "create: rotation must be finite");
  if (!std::isfinite(p.distance_near) || !std::isfinite(p.distance_far) || !std::isfinite(p.z_low) || !std::isfinite(p.z_high))
    return scan_fail(GORIO_ERR_INVALID, "create: the distance filter's thresholds must be finite");
  if (!std::isfinite(p.scan_period)) return scan_fail(GORIO_ERR_INVALID, "create: scan_period must be finite");
  if (p.outlier_method < GORIO_SCAN_OUTLIER_NONE || p.outlier_method > GORIO_SCAN_OUTLIER_RADIUS) return scan_fail(GORIO_ERR_INVALID, "create: unknown outlier_method");
  if (p.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL && (p.mean_k < 1 || p.mean_k > 31)) return scan_fail(GORIO_ERR_INVALID, "create: mean_k must lie in [1, 31]");
  if (p.outlier_method == GORIO_SCAN_OUTLIER_RADIUS && (!(p.radius > 0.0) || p.min_neighbors < 0)) return scan_fail(GORIO_ERR_INVALID, "create: bad radius / min_neighbors");
  if (p.reve.n_ransac_points < 3 || p.reve.n_ransac_points > 64) return scan_fail(GORIO_ERR_INVALID, "create: reve.n_ransac_points must lie in [3, 64]");
  return GORIO_OK;
}

// the device side of a handle: made by the first load, so that create, and the argument and state checks of every call, need no device
int scan_ensure_device(gorio_scan* h) {
  if (h->on_device) return GORIO_OK;
  int ndev = 0, rc = GORIO_OK;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return scan_fail(GORIO_ERR_NO_DEVICE, "load: no usable HIP device (there is no CPU fallback)");
  if (h->device >= ndev) return scan_fail(GORIO_ERR_INVALID, "load: bad device ordinal");
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
  h->stream = device_stream(h->device);
  if (!h->stream) return scan_fail(GORIO_ERR_NO_DEVICE, "load: no stream");
  if (h->p.ground && !h->ground) {
    rc = gorio_ground_create(&h->ground, h->device, &h->p.ground_params);
    if (rc) return scan_fail(rc, std::string("load: ground segmenter: ") + gorio_ground_last_error());
  }
  if (!prep_context(h->prep, h->device, "scan", rc)) return scan_fail(rc, gorio_prep_last_error());
  h->on_device = true;
  return GORIO_OK;
}

// run() ended in `stage` with EMPTY / REFUSED
int scan_end(gorio_scan_result* r, int status, int stage, int rc) {
  r->status = status;
  r->stage = stage;
  return rc;
}

}  // namespace

extern "C" {

const char* gorio_scan_last_error(void) { return g_scan_err.c_str(); }

void gorio_scan_default_params(gorio_scan_params* p) {  // the second argument of each private_nh.param, PREP:97-181, 526-529, 705
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->power_threshold = 0.0f;
  p->rotation[0] = p->rotation[4] = p->rotation[8] = 1.0;
  p->enable_dynamic_object_removal = 0;
  p->deskew = 1;
  p->scan_period = 0.1;
  p->distance_near = 1.0;
  p->distance_far = 100.0;
  p->z_low = -5.0;
  p->z_high = 20.0;
  p->outlier_method = GORIO_SCAN_OUTLIER_STATISTICAL;
  p->mean_k = 20;
  p->stddev_mul = 1.0;
  p->radius = 2.0;
  p->min_neighbors = 2;
  p->ground = 1;
  gorio_ground_default_params(&p->ground_params);
  p->dbscan_core_min_pts = 10;
  p->dbscan_eps = 0.9;
  p->dbscan_min_cluster_size = 20;
  p->dbscan_max_cluster_size = 25000;
  gorio_prep_reve_default_config(&p->reve);
}

int gorio_scan_create(gorio_scan_t** out, int device, const gorio_scan_params* p) {
  if (!out || !p) return scan_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  int rc = scan_check_params(*p);
  if (rc) return rc;
  if (device < 0) return scan_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  std::unique_ptr<gorio_scan> h(new (std::nothrow) gorio_scan());
  if (!h) return scan_fail(GORIO_ERR_ALLOC, "create: out of memory");
  h->device = device;
  h->p = *p;
  for (auto& s : h->stage_cloud) s = nullptr;
  h->cl[kScanRaw].identity = true;
  h->cl[1 + GORIO_SCAN_STAGE_GATE].is_gated = true;
  *out = h.release();
  return GORIO_OK;
}

void gorio_scan_destroy(gorio_scan_t* h) {
  if (!h) return;
  if (h->on_device) {
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
  }
  if (h->ground) gorio_ground_destroy(h->ground);
  delete h;  // prep frees its registration handle, the buffers free themselves
}

int gorio_scan_load(gorio_scan_t* h, const float* xyz, const float* power, const float* doppler, int n, int stride_bytes, int* n_gated, int* n_valid) {
  if (!h) return scan_fail(GORIO_ERR_INVALID, "load: null handle");
  if (n < 0 || (n > 0 && (!xyz || !power || !doppler)) || stride_bytes < 4 || (stride_bytes % 4) || !n_gated || !n_valid) return scan_fail(GORIO_ERR_INVALID, "load: bad arguments");
  h->loaded = false;
  h->have_output = false;
  for (auto& s : h->stage_cloud) s = nullptr;
  *n_gated = *n_valid = 0;
  int rc = scan_ensure_device(h);
  if (rc) return rc;
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
  rc = scan_reserve(h, n);
  if (rc) return rc;
  ScanCloud &raw = h->cl[kScanRaw], &gated = h->cl[1 + GORIO_SCAN_STAGE_GATE];
  h->n_raw = n;
  raw.n = n;
  gated.n = 0;
  h->frame = ReveFrame();
  if (n > 0) {
    // ---- the one upload of the frame: the five message columns in one copy
    const size_t st = stride_bytes / 4, cap = raw.cap;
    std::vector<float> cols(4 * cap + (size_t)n);
    for (int i = 0; i < n; ++i) {
      const float* pt = xyz + st * i;
      cols[i] = pt[0];
      cols[cap + i] = pt[1];
      cols[2 * cap + i] = pt[2];
      cols[3 * cap + i] = power[st * i];
      cols[4 * cap + i] = doppler[st * i];
    }
    GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(raw.f, cols.data(), sizeof(float) * cols.size(), hipMemcpyHostToDevice, h->stream));
    ++h->point_uploads;
    gorio::GateArgs ga;
    std::memcpy(ga.R, h->p.rotation, sizeof(ga.R));
    ga.power_threshold = h->p.power_threshold;
    gorio::scan_gate_rotate_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(raw.col(0), raw.col(1), raw.col(2), raw.col(3), n, ga, h->d_keep);
    GORIO_HIP_CHECK(scan_fail, hipGetLastError());
    rc = scan_compact(h, raw, gated);  // synchronises: cols may die
    if (rc) return rc;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_GATE] = &gated;
  *n_gated = gated.n;
  if (gated.n > 0) {  // REVE:75-90 on the gated cloud (radarcloud_raw, PREP:397-409)
    rc = reve_prepare(h->reve, h->device, gated.n);
    if (!rc) rc = reve_features(h->reve, gated.col(0), gated.col(1), gated.col(2), gated.col(3), gated.col(4), 1, gated.n, &h->p.reve, h->frame);
    if (rc) return scan_fail(rc, gorio_prep_last_error());
  }
  *n_valid = h->frame.m;
  h->loaded = true;
  return GORIO_OK;
}

static int scan_run_stages(gorio_scan_t* h, const unsigned int* sample_idx, int n_iter, const double* ang_vel, gorio_scan_result* result);

int gorio_scan_run(gorio_scan_t* h, const unsigned int* sample_idx, int n_iter, const double* ang_vel, gorio_scan_result* result) {
  if (!h || !result) return scan_fail(GORIO_ERR_INVALID, "run: null argument");
  std::memset(result, 0, sizeof(*result));
  result->stage = -1;
  if (n_iter < 0 || (n_iter > 0 && !sample_idx)) return scan_fail(GORIO_ERR_INVALID, "run: bad sample arguments");
  if (!h->loaded) return scan_fail(GORIO_ERR_STATE, "run: no scan loaded (gorio_scan_load comes first, once per run)");
  h->run_err.clear();
  const int rc = scan_run_stages(h, sample_idx, n_iter, ang_vel, result);
  if (result->status == GORIO_SCAN_REFUSED) h->run_err = g_scan_err;
  return rc;
}

static int scan_run_stages(gorio_scan_t* h, const unsigned int* sample_idx, int n_iter, const double* ang_vel, gorio_scan_result* result) {
  h->loaded = false;
  h->have_output = false;
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
  const gorio_scan_params& P = h->p;
  const ScanCloud* cur = &h->cl[1 + GORIO_SCAN_STAGE_GATE];
  if (cur->n == 0) return scan_end(result, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_GATE, GORIO_OK);  // REVE fails on no targets, src_cloud is empty (PREP:480)
  // ---- 1. REVE (PREP:421-449)
  std::vector<unsigned char> inlier((size_t)cur->n);
  int zero = 0, ok = 0;
  int rc = reve_solve(h->reve, &P.reve, h->frame, sample_idx, n_iter, result->v_r, result->sigma_v_r, inlier.data(), nullptr, &zero, &ok);
  if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GATE, scan_fail(rc, gorio_prep_last_error()));
  result->reve_success = ok;
  if (ok) {
    const double* v = result->v_r;
    if (std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) < 0.05) return scan_end(result, GORIO_SCAN_ZERO_VELOCITY, -1, GORIO_OK);  // PREP:427-430
  } else {
    for (int q = 0; q < 3; ++q) result->v_r[q] = result->sigma_v_r[q] = 0.0;
  }
  // ---- 2. dynamic-object removal (PREP:464-478): the inlier cloud of the estimate, which is empty when it failed
  if (P.enable_dynamic_object_removal) {
    if (!ok) std::fill(inlier.begin(), inlier.end(), 0);
    rc = scan_upload_keep(h, inlier);
    ScanCloud& dst = h->cl[1 + GORIO_SCAN_STAGE_DYNAMIC];
    if (!rc) rc = scan_compact(h, *cur, dst);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_DYNAMIC, rc);
    cur = &dst;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_DYNAMIC] = cur;
  if (cur->n == 0) return scan_end(result, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_DYNAMIC, GORIO_OK);  // PREP:480-482
  // ---- 3. deskew (PREP:484, 658-719)
  if (P.deskew && ang_vel) {
    ScanCloud& dst = h->cl[1 + GORIO_SCAN_STAGE_DESKEW];
    const float wx = -(float)ang_vel[0], wy = -(float)ang_vel[1], wz = -(float)ang_vel[2];  // PREP:695-696
    gorio::scan_deskew_kernel<<<(cur->n + 255) / 256, 256, 0, h->stream>>>(scan_columns(*cur, dst), cur->n, P.scan_period, wx, wy, wz);
    GORIO_HIP_CHECK(scan_fail, hipGetLastError());
    dst.n = cur->n;
    dst.identity = false;
    cur = &dst;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_DESKEW] = cur;
  // ---- 4. distance filter (PREP:502, 639-656)
  {
    gorio::DistanceArgs da{P.distance_near, P.distance_far, P.z_low, P.z_high};
    gorio::scan_distance_kernel<<<(cur->n + 255) / 256, 256, 0, h->stream>>>(cur->col(0), cur->col(1), cur->col(2), cur->n, da, h->d_keep);
    GORIO_HIP_CHECK(scan_fail, hipGetLastError());
    ScanCloud& dst = h->cl[1 + GORIO_SCAN_STAGE_DISTANCE];
    rc = scan_compact(h, *cur, dst);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_DISTANCE, rc);
    cur = &dst;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_DISTANCE] = cur;
  if (cur->n == 0) return scan_end(result, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_DISTANCE, GORIO_OK);
  // ---- 5. outlier removal (PREP:503, 626-637)
  if (P.outlier_method != GORIO_SCAN_OUTLIER_NONE) {
    const int n = cur->n;
    if (P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL && n < P.mean_k + 1)
      return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_OUTLIER, scan_fail(GORIO_ERR_INVALID, kSorTooFew));
    std::vector<unsigned char> keep((size_t)n);
    rc = prep_index_cloud_device(h->prep, cur->col(0), cur->col(1), cur->col(2), n);
    if (!rc) {
      ++h->index_builds;
      rc = P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL ? prep_statistical_outlier_keep(h->prep, n, P.mean_k, P.stddev_mul, keep.data(), nullptr, nullptr)
                                                               : prep_radius_outlier_keep(h->prep, n, P.radius, P.min_neighbors, keep.data(), nullptr);
    }
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_OUTLIER, scan_fail(rc, gorio_prep_last_error()));
    rc = scan_upload_keep(h, keep);
    ScanCloud& dst = h->cl[1 + GORIO_SCAN_STAGE_OUTLIER];
    if (!rc) rc = scan_compact(h, *cur, dst);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_OUTLIER, rc);
    cur = &dst;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_OUTLIER] = cur;
  if (cur->n == 0) return scan_end(result, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_OUTLIER, GORIO_OK);
  // ---- 6. Patchwork++ and full_scan = ground + nonground (PREP:505-518)
  if (h->ground) {
    const int n = cur->n;
    std::vector<int> order((size_t)n, -1);
    int* order_ptr = order.data();
    int n_ground = 0, n_full = 0;
    const GroundDeviceScan dev{cur->col(0), cur->col(1), cur->col(2), cur->col(3)};
    gorio_ground* const hs[1] = {h->ground};
    GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));  // the segmenter launches on a stream of its own
    rc = ground_run(hs, 1, nullptr, nullptr, &n, nullptr, 1, &order_ptr, &n_ground, &n_full, &dev);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GROUND, scan_fail(rc, gorio_ground_last_error()));
    for (int j = 0; j < n_full; ++j)
      if (order[j] < 0 || order[j] >= n) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_GROUND, scan_fail(GORIO_ERR_STATE, "run: ground order outside the cloud"));
    ScanCloud& dst = h->cl[1 + GORIO_SCAN_STAGE_GROUND];
    dst.n = n_full;
    dst.identity = false;
    if (n_full > 0) {
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_order, order.data(), sizeof(int) * (size_t)n_full, hipMemcpyHostToDevice, h->stream));
      gorio::scan_permute_kernel<<<(n_full + 255) / 256, 256, 0, h->stream>>>(scan_columns(*cur, dst), h->d_order, n_full);
      GORIO_HIP_CHECK(scan_fail, hipGetLastError());
      GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));  // order is pageable
    }
    result->n_ground = n_ground;
    cur = &dst;
  }
  h->stage_cloud[GORIO_SCAN_STAGE_GROUND] = cur;
  if (cur->n == 0) return scan_end(result, GORIO_SCAN_EMPTY, GORIO_SCAN_STAGE_GROUND, GORIO_OK);
  // ---- 7. DBSCAN labels (PREP:520-568).  The cloud becomes the source of the pipeline's registration handle: that cloud and its index
  // are what gorio_apd_set_*_from_scan hands over.
  {
    const int n = cur->n;
    rc = prep_index_cloud_device(h->prep, cur->col(0), cur->col(1), cur->col(2), n);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_DBSCAN, scan_fail(rc, gorio_prep_last_error()));
    ++h->index_builds;
    std::vector<std::vector<int>> clusters;
    rc = prep_dbscan_clusters(h->prep, n, P.dbscan_eps, P.dbscan_core_min_pts, P.dbscan_min_cluster_size, P.dbscan_max_cluster_size, clusters);
    if (rc) return scan_end(result, GORIO_SCAN_REFUSED, GORIO_SCAN_STAGE_DBSCAN, scan_fail(rc, gorio_prep_last_error()));
    const int nc = (int)clusters.size();
    std::vector<float> lab((size_t)n, 0.0f);
    if (nc > 0) {  // PREP:537-568: the coordinate sums on the device, ranking and label values here
      std::vector<int> members, offs(1, 0);
      for (const std::vector<int>& m : clusters) {
        members.insert(members.end(), m.begin(), m.end());
        offs.push_back((int)members.size());
      }
      GORIO_HIP_CHECK(scan_fail, h->d_members.reserve(members.size(), members.size() + members.size() / 8));
      GORIO_HIP_CHECK(scan_fail, h->d_coffs.reserve(offs.size(), offs.size() + 64));
      GORIO_HIP_CHECK(scan_fail, h->d_sums.reserve(3 * (size_t)nc, 3 * (size_t)nc + 192));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_members, members.data(), sizeof(int) * members.size(), hipMemcpyHostToDevice, h->stream));
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_coffs, offs.data(), sizeof(int) * offs.size(), hipMemcpyHostToDevice, h->stream));
      gorio::cluster_sums_kernel<<<(nc + 63) / 64, 64, 0, h->stream>>>(cur->col(0), cur->col(1), cur->col(2), h->d_members, h->d_coffs, nc, h->d_sums);
      GORIO_HIP_CHECK(scan_fail, hipGetLastError());
      std::vector<float> sums(3 * (size_t)nc);
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(sums.data(), h->d_sums, sizeof(float) * sums.size(), hipMemcpyDeviceToHost, h->stream));
      GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));
      std::vector<int> order;
      prep_rank_clusters(clusters, sums.data(), order);
      for (int r = 0; r < nc; ++r)
        for (int idx : clusters[order[r]]) lab[idx] = (float)(r + 1);
    }
    DevCloud& out = *h->prep.h->src;
    GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(h->d_lab, lab.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    gorio::scan_set_labels_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(h->d_lab, n, out.label, out.p4);
    GORIO_HIP_CHECK(scan_fail, hipGetLastError());
    GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));  // lab is pageable
    result->n_clusters = nc;
    result->n_out = n;
    h->n_out = n;
  }
  h->have_output = true;
  result->status = GORIO_SCAN_OK;
  return GORIO_OK;
}

int gorio_scan_get_output(gorio_scan_t* h, float* xyz, float* intensity, float* doppler, float* label, int stride_bytes, int capacity) {
  if (!h || stride_bytes < 4 || (stride_bytes % 4) || (xyz && stride_bytes < 12)) return scan_fail(GORIO_ERR_INVALID, "get_output: bad arguments");
  if (!h->have_output) return scan_fail(GORIO_ERR_STATE, "get_output: the last run produced no frame");
  const int n = h->n_out;
  if (capacity < n) return scan_fail(GORIO_ERR_INVALID, "get_output: capacity too small");
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
  const ScanCloud& c = *h->stage_cloud[GORIO_SCAN_STAGE_GROUND];
  const DevCloud& out = *h->prep.h->src;
  std::vector<float> buf(6 * (size_t)n);
  for (int q = 0; q < 5; ++q) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(buf.data() + (size_t)q * n, c.col(q), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(buf.data() + 5 * (size_t)n, out.label, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));
  ++h->point_downloads;
  const size_t st = stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    if (xyz) {
      xyz[st * i] = buf[i];
      xyz[st * i + 1] = buf[(size_t)n + i];
      xyz[st * i + 2] = buf[2 * (size_t)n + i];
    }
    if (intensity) intensity[st * i] = buf[3 * (size_t)n + i];
    if (doppler) doppler[st * i] = buf[4 * (size_t)n + i];
    if (label) label[st * i] = buf[5 * (size_t)n + i];
  }
  return GORIO_OK;
}

static int scan_get_stage(gorio_scan* h, int stage, int* index_out, float* xyz_out, int capacity, int* count) {
  if (!h || !count || stage < 0 || stage >= GORIO_SCAN_STAGE_COUNT || capacity < 0) return scan_fail(GORIO_ERR_INVALID, "get_stage: bad arguments");
  const ScanCloud* c = h->stage_cloud[stage];
  *count = c ? c->n : 0;
  if (!c || c->n == 0) return GORIO_OK;
  if ((index_out || xyz_out) && capacity < c->n) return scan_fail(GORIO_ERR_INVALID, "get_stage: capacity too small (count holds the size needed)");
  GORIO_HIP_CHECK(scan_fail, hipSetDevice(h->device));
  const int n = c->n;
  if (index_out) {
    if (stage != GORIO_SCAN_STAGE_GATE && c->is_gated) {  // the gated cloud in its own order
      for (int i = 0; i < n; ++i) index_out[i] = i;
    } else {
      GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(index_out, c->map, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
      GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));
    }
  }
  if (xyz_out) {
    std::vector<float> buf(3 * (size_t)n);
    for (int q = 0; q < 3; ++q) GORIO_HIP_CHECK(scan_fail, hipMemcpyAsync(buf.data() + (size_t)q * n, c->col(q), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    GORIO_HIP_CHECK(scan_fail, hipStreamSynchronize(h->stream));
    ++h->point_downloads;
    for (int i = 0; i < n; ++i) {
      xyz_out[3 * (size_t)i] = buf[i];
      xyz_out[3 * (size_t)i + 1] = buf[(size_t)n + i];
      xyz_out[3 * (size_t)i + 2] = buf[2 * (size_t)n + i];
    }
  }
  return GORIO_OK;
}

int gorio_scan_get_stage(gorio_scan_t* h, int stage, int* index_out, int capacity, int* count) { return scan_get_stage(h, stage, index_out, nullptr, capacity, count); }
int gorio_scan_get_stage_points(gorio_scan_t* h, int stage, float* xyz_out, int capacity, int* count) { return scan_get_stage(h, stage, nullptr, xyz_out, capacity, count); }

static int scan_hand_off(gorio_apd* apd, gorio_scan* scan, bool source) {
  if (!apd) return GORIO_ERR_INVALID;
  if (!scan) return fail(apd, GORIO_ERR_INVALID, "set_input_from_scan: null pipeline");
  if (apd->device != scan->device) return fail(apd, GORIO_ERR_INVALID, "set_input_from_scan: both handles must live on one device");
  if (!scan->have_output) return fail(apd, GORIO_ERR_STATE, "set_input_from_scan: the pipeline's last run produced no frame");
  const std::shared_ptr<DevCloud>& out = scan->prep.h->src;
  if (cov_rule_differs(apd, *out))
    return fail(apd, GORIO_ERR_INVALID, "set_input_from_scan: another handle estimated this cloud's covariances with another k_correspondences / regularization");
  (source ? apd->src : apd->tgt) = out;  // points, labels, search index: one copy on the device, alive until the last handle lets go of it
  apd->corr_valid = false;
  return GORIO_OK;
}
int gorio_apd_set_source_from_scan(gorio_apd_t* apd, gorio_scan_t* scan) { return scan_hand_off(apd, scan, true); }
int gorio_apd_set_target_from_scan(gorio_apd_t* apd, gorio_scan_t* scan) { return scan_hand_off(apd, scan, false); }

// ---- the hand-offs of include/gorio_ndt.h.  They live here because this is where gorio_scan, gorio_apd and gorio_ndt are all complete
// types; the device half is ndt_adopt (csrc/apd_ndt.hip).  A hand-off is a COPY of x, y, z of the first n points -- NDT wants neither
// labels nor a search index and keeps a SoA cloud of its own -- so it moves none of the pipeline's counters.
// Order of the points: the pipeline's output is stage_cloud[GROUND], the columns gorio_scan_get_output downloads, written by
// scan_permute_kernel / compact_scatter_kernel in output order.  A registration cloud keeps x[i], y[i], z[i] == p4[i] for i < n in the
// order it was given (copy_cloud_kernel, copy_clouds_kernel, submap_store_kernel, upload_cloud); the search index sorts into arrays of
// its own (idx_sx, idx_orig), never in place.  So neither side needs a permutation.
// Streams: gorio_scan_run synchronises the pipeline's stream after the last kernel that writes the columns (the label upload, just
// before have_output is set), but gorio_apd_set_target_device / _set_clouds_device_batch return with their copy kernel in flight, so
// ndt_adopt orders its copy behind the producer's stream with one event in every case.
static int ndt_scan_hand_off(gorio_ndt* ndt, gorio_scan* scan, bool source) {
  const std::string what = source ? "set_source_from_scan" : "set_target_from_scan";
  if (!ndt) return ndt_fail(GORIO_ERR_INVALID, what + ": null handle");
  if (!scan) return ndt_fail(GORIO_ERR_INVALID, what + ": null pipeline");
  if (!scan->have_output) return ndt_fail(GORIO_ERR_STATE, what + ": the pipeline's last run produced no frame");
  if (ndt->device != scan->device) return ndt_fail(GORIO_ERR_INVALID, what + ": both handles must live on one device");
  const ScanCloud& c = *scan->stage_cloud[GORIO_SCAN_STAGE_GROUND];
  return ndt_adopt(ndt, c.col(0), c.col(1), c.col(2), scan->n_out, scan->stream, source, what);
}
int gorio_ndt_set_source_from_scan(gorio_ndt_t* ndt, gorio_scan_t* scan) { return ndt_scan_hand_off(ndt, scan, true); }
int gorio_ndt_set_target_from_scan(gorio_ndt_t* ndt, gorio_scan_t* scan) { return ndt_scan_hand_off(ndt, scan, false); }

int gorio_ndt_set_target_from_apd(gorio_ndt_t* ndt, gorio_apd_t* apd) {
  const std::string what = "set_target_from_apd";
  if (!ndt) return ndt_fail(GORIO_ERR_INVALID, what + ": null handle");
  if (!apd) return ndt_fail(GORIO_ERR_INVALID, what + ": null registration handle");
  if (ndt->device != apd->device) return ndt_fail(GORIO_ERR_INVALID, what + ": both handles must live on one device");
  const DevCloud& t = *apd->tgt;
  if (!t.present) return ndt_fail(GORIO_ERR_STATE, what + ": the registration handle has no input target");
  return ndt_adopt(ndt, t.x, t.y, t.z, t.n, apd->stream, false, what);
}

int gorio_scan_get_counters(const gorio_scan_t* h, long long* point_uploads, long long* index_builds, long long* point_downloads) {
  if (!h) return scan_fail(GORIO_ERR_INVALID, "get_counters: null handle");
  if (point_uploads) *point_uploads = h->point_uploads;
  if (index_builds) *index_builds = h->index_builds;
  if (point_downloads) *point_downloads = h->point_downloads;
  return GORIO_OK;
}

}  // extern "C"

#include "apd_scan_batch.hip"
