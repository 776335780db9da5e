// apd_keyframes.hip -- the keyframe store and its consumers: include/gorio_keyframes.h.  Kernels first, the host side below them.
// Included at the end of apd_api.hip, after apd_scan.hip: this is where gorio_apd, gorio_scan, gorio_ndt and gorio_sc are all complete
// types, and the ordered compaction's block scan (block_scan_kernel, apd_voxel_group.hip) is reused from there.
//
// SMO = apps/scan_matching_odometry_nodelet.cpp, RGS = apps/radar_graph_slam_nodelet.cpp, LD = src/radar_graph_slam/loop_detector.cpp
// of the Go-RIO sources.
//
// Arithmetic: kf_submap_scatter_kernel must give the bits of submap_transform_kernel (apd_submap.hip).  Floating-point contraction is OFF
// for this file as for that one -- the library's Makefile passes -ffp-contract=off, and the pragma below repeats it for a build that does
// not -- so the four products of a row are rounded one by one and summed left to right in double, then rounded to float once.
#include <hip/hip_runtime.h>

#include "../../include/gorio_keyframes.h"
#include "edge_information.h"

#pragma clang fp contract(off)

namespace gorio {

// ---------------------------------------------------------------------------------------------- submap from resident keyframes
// What the host loop of gorio_apd_set_target_submap does serially (skip non-finite points, pack the frames one behind the other, then
// submap_transform_kernel) in three launches, none of which waits for another workgroup:
//   kf_submap_count_kernel     per 256-point block of every frame: the finite points, one ballot + popcount per wave
//   block_scan_kernel          ONE workgroup scans all block counts (exclusive, in place; any number of blocks) and leaves the total behind
//   kf_submap_scatter_kernel   every block repeats its ballots and writes each finite point, transformed, at its rank
// Blocks are numbered frame by frame (KfFrame::blk0), so ranks ascend in frame order and, inside a frame, in point order.
// grid: (max blocks of one frame, frames), block 256; a block beyond its frame's last one leaves at once (uniform per block).
struct KfFrame {
  const float4* p4;  // the keyframe's packed points (x, y, z, label); null when n == 0
  int n;
  int blk0;          // index of this frame's first block in the count array
  double T[12];      // rows 0..2 of rel_pose, row-major
};

__device__ __forceinline__ bool kf_finite(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__global__ __launch_bounds__(256) void kf_submap_count_kernel(const KfFrame* __restrict__ frames, int* __restrict__ bcnt) {
  const int n = frames[blockIdx.y].n;
  if ((int)blockIdx.x * 256 >= n) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool k = i < n && kf_finite(frames[blockIdx.y].p4[i]);
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) bcnt[frames[blockIdx.y].blk0 + blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

__global__ __launch_bounds__(256) void kf_submap_scatter_kernel(const KfFrame* __restrict__ frames, const int* __restrict__ boffs, float4* __restrict__ out) {
  const KfFrame& f = frames[blockIdx.y];
  const int n = f.n;
  if ((int)blockIdx.x * 256 >= n) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) p = f.p4[i];
  const bool k = i < n && kf_finite(p);
  const unsigned long long b = __ballot(k);
  __shared__ int w[4];
  if (lane == 0) w[wave] = __popcll(b);
  __syncthreads();
  if (!k) return;
  int pos = boffs[f.blk0 + blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int q = 0; q < wave; ++q) pos += w[q];
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  float4 q;
  q.x = (float)(f.T[0] * x + f.T[1] * y + f.T[2] * z + f.T[3]);
  q.y = (float)(f.T[4] * x + f.T[5] * y + f.T[6] * z + f.T[7]);
  q.z = (float)(f.T[8] * x + f.T[9] * y + f.T[10] * z + f.T[11]);
  q.w = p.w;
  out[pos] = q;
}

// ---------------------------------------------------------------------------------------------- Scan Context from resident keyframes
// pts[off + i] = (x, y, intensity, 0) of every listed keyframe, and the scan offsets offs[0 .. count]: the blob gorio_sc_add_scans uploads.
// grid: (max(1, max blocks of one keyframe), keyframes), block 256.
struct KfScJob {
  const float4* p4;
  const float* intensity;
  int n, off;
};
__global__ __launch_bounds__(256) void kf_sc_pack_kernel(const KfScJob* __restrict__ jobs, int count, int total, float4* __restrict__ pts, int* __restrict__ offs) {
  const KfScJob j = jobs[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    offs[blockIdx.y] = j.off;
    if (blockIdx.y == 0) offs[count] = total;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= j.n) return;
  const float4 p = j.p4[i];
  pts[j.off + i] = make_float4(p.x, p.y, j.intensity[i], 0.0f);
}

// ---------------------------------------------------------------------------------------------- pose-graph edges between keyframes
// The reduction of gorio_kf_edge_fitness (include/gorio_kf_edges.h) over the packed keys the pruned search left: per 256 source points
// of every edge the sum of the squared distances within max_range_sq and their number.  The partition, the wave_sum tree and the
// combination of the four wave sums are those of fitness_kernel (apd_kernels.hip), so an edge's partials are bit for bit the ones a
// single gorio_apd_fitness_score computes.  Edges differ in size by orders of magnitude, so the partials are not a [edges][max blocks]
// rectangle: every edge's descriptor names its own slice (PairDesc::partials = out + 2 * first block of the edge) and the host reads
// back exactly the blocks that exist.  grid: (max blocks of one edge, edges), block 256; a block past its edge's last one leaves at once.
__global__ __launch_bounds__(256) void kf_edge_reduce_kernel(const PairDesc* __restrict__ descs, double max_range_sq) {
  const PairDesc& pd = descs[blockIdx.y];
  const int n = pd.src.n;
  if ((int)blockIdx.x * 256 >= n) return;  // uniform over the block
  const int i = blockIdx.x * 256 + threadIdx.x;
  double s = 0.0, c = 0.0;
  if (i < n) {
    const unsigned long long key = pd.best_key[i];
    if (key != ~0ull) {
      const double d = (double)__uint_as_float((unsigned int)(key >> 32));
      if (d <= max_range_sq) {
        s = d;
        c = 1.0;
      }
    }
  }
  s = wave_sum(s);
  c = wave_sum(c);
  __shared__ double sw[4][2];
  if ((threadIdx.x & 63) == 0) {
    sw[threadIdx.x >> 6][0] = s;
    sw[threadIdx.x >> 6][1] = c;
  }
  __syncthreads();
  if (threadIdx.x < 2) pd.partials[(size_t)blockIdx.x * 2 + threadIdx.x] = (sw[0][threadIdx.x] + sw[1][threadIdx.x]) + (sw[2][threadIdx.x] + sw[3][threadIdx.x]);
}

}  // namespace gorio

// ================================================================================================= host (include/gorio_keyframes.h)
namespace {
thread_local std::string g_kf_err;
int kf_fail(int code, const std::string& m) {
  g_kf_err = m;
  return code;
}

struct KfEntry {
  std::shared_ptr<DevCloud> cloud;  // null after gorio_kf_release
  DevBuf<float> intensity;          // n floats when has_intensity
  bool has_intensity = false;
  int n = 0;
};
}  // namespace

struct gorio_kf {
  int device = 0;
  gorio_apd* up = nullptr;  // made by the first call that needs the device: its stream (the device's launch stream) and upload_cloud run through it
  std::vector<KfEntry> kfs;
  long long point_uploads = 0, point_downloads = 0, device_copies = 0;
  // gorio_kf_edge_fitness (include/gorio_kf_edges.h).  The search scratch of ALL edges of a call, one slice per edge: packed keys by
  // source point, seeds by sorted source position, the measured work and the plan of the query waves.  A registration handle keeps
  // these per handle, which is why two of its pairs cannot share a source; here they belong to the edge.  They grow, never shrink.
  DevBuf<unsigned long long> e_keys;
  DevBuf<int> e_seed;
  DevBuf<unsigned int> e_work, e_plan;
  DevBuf<void> e_tab;    // the edge table: [edges] PairDesc, then [edges] PairState; staged in e_pin (free again once a call has synchronised)
  DevBuf<double> e_fit;  // [blocks of all edges][2] partial sums and counts, read back into e_out
  PinnedBuf e_pin, e_out;
  long long edge_calls = 0, edge_edges = 0, edge_index_builds = 0, edge_syncs = 0;
};

namespace {

int kf_ensure_device(gorio_kf* kf, const char* who) {
  if (kf->up) return GORIO_OK;
  const int rc = gorio_apd_create(&kf->up, kf->device);
  if (rc == GORIO_ERR_INVALID) return kf_fail(rc, std::string(who) + ": bad device ordinal");
  if (rc) return kf_fail(rc, std::string(who) + ": no usable HIP device (there is no CPU fallback)");
  return GORIO_OK;
}

// the entry of `id`, or null with *rc set: GORIO_ERR_INVALID for an id never added, GORIO_ERR_STATE for a released one
const KfEntry* kf_entry(const gorio_kf* kf, int id, int* rc, std::string* why) {
  if (id < 0 || id >= (int)kf->kfs.size()) {
    *rc = GORIO_ERR_INVALID;
    *why = "keyframe " + std::to_string(id) + " has not been added (" + std::to_string(kf->kfs.size()) + " keyframes)";
    return nullptr;
  }
  if (!kf->kfs[id].cloud) {
    *rc = GORIO_ERR_STATE;
    *why = "keyframe " + std::to_string(id) + " has been released";
    return nullptr;
  }
  return &kf->kfs[id];
}

int kf_push(gorio_kf* kf, KfEntry&& e, int* id) {
  try {
    kf->kfs.push_back(std::move(e));
  } catch (const std::bad_alloc&) {
    return kf_fail(GORIO_ERR_ALLOC, "add: out of memory");
  }
  *id = (int)kf->kfs.size() - 1;
  return GORIO_OK;
}

}  // namespace

extern "C" {

const char* gorio_kf_last_error(void) { return g_kf_err.c_str(); }

int gorio_kf_create(gorio_kf_t** out, int device) {
  if (!out) return kf_fail(GORIO_ERR_INVALID, "create: null argument");
  *out = nullptr;
  if (device < 0) return kf_fail(GORIO_ERR_INVALID, "create: bad device ordinal");
  gorio_kf* kf = new (std::nothrow) gorio_kf();
  if (!kf) return kf_fail(GORIO_ERR_ALLOC, "create: out of memory");
  kf->device = device;
  *out = kf;
  return GORIO_OK;
}

void gorio_kf_destroy(gorio_kf_t* kf) {
  if (!kf) return;
  if (kf->up) {
    hipSetDevice(kf->device);
    hipStreamSynchronize(kf->up->stream);
    kf->kfs.clear();  // the store's shares and the intensity columns, with the device current
    gorio_apd_destroy(kf->up);
  }
  delete kf;
}

int gorio_kf_add(gorio_kf_t* kf, const float* xyz, const float* intensity, const float* label, int n, int stride_bytes, int* id) {
  if (!kf || !id) return kf_fail(GORIO_ERR_INVALID, "add: null argument");
  if (n < 0 || (n > 0 && !xyz) || stride_bytes < 12 || (stride_bytes % 4) != 0) return kf_fail(GORIO_ERR_INVALID, "add: bad cloud arguments");
  int rc = kf_ensure_device(kf, "add");
  if (rc) return rc;
  GORIO_HIP_CHECK(kf_fail, hipSetDevice(kf->device));
  KfEntry e;
  e.cloud = std::make_shared<DevCloud>();
  e.cloud->device = kf->device;
  e.n = n;
  if (n > 0) {
    rc = upload_cloud(kf->up, *e.cloud, xyz, label, n, stride_bytes);  // the routine of gorio_apd_set_source; synchronises
    if (rc) return kf_fail(rc, "add: " + kf->up->err);
    if (intensity) {
      GORIO_HIP_CHECK(kf_fail, e.intensity.reserve(n));
      std::vector<float> col((size_t)n);
      const size_t st = stride_bytes / 4;
      for (int i = 0; i < n; ++i) col[i] = intensity[st * i];
      GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(e.intensity, col.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, kf->up->stream));
      GORIO_HIP_CHECK(kf_fail, hipStreamSynchronize(kf->up->stream));  // col is pageable
    }
  }
  e.has_intensity = intensity != nullptr;
  rc = kf_push(kf, std::move(e), id);
  if (rc) return rc;
  ++kf->point_uploads;
  return GORIO_OK;
}

int gorio_kf_add_from_scan(gorio_kf_t* kf, gorio_scan_t* scan, int* id) {
  if (!kf || !scan || !id) return kf_fail(GORIO_ERR_INVALID, "add_from_scan: null argument");
  if (kf->device != scan->device) return kf_fail(GORIO_ERR_INVALID, "add_from_scan: the store and the pipeline must live on one device");
  if (!scan->have_output) return kf_fail(GORIO_ERR_STATE, "add_from_scan: the pipeline's last run produced no frame");
  int rc = kf_ensure_device(kf, "add_from_scan");
  if (rc) return rc;
  GORIO_HIP_CHECK(kf_fail, hipSetDevice(kf->device));
  KfEntry e;
  e.cloud = scan->prep.h->src;  // the cloud gorio_apd_set_source_from_scan shares: the pipeline starts its next frame in fresh buffers
  e.n = scan->n_out;
  if (!e.cloud->present || e.cloud->n != e.n) return kf_fail(GORIO_ERR_STATE, "add_from_scan: the pipeline's output cloud does not match its last run");
  const ScanCloud& c = *scan->stage_cloud[GORIO_SCAN_STAGE_GROUND];
  GORIO_HIP_CHECK(kf_fail, e.intensity.reserve(std::max(e.n, 1)));
  // behind the pipeline's stream, and complete on return: the pipeline reuses its stage buffers for the next frame
  GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(e.intensity, c.col(3), sizeof(float) * (size_t)e.n, hipMemcpyDeviceToDevice, scan->stream));
  GORIO_HIP_CHECK(kf_fail, hipStreamSynchronize(scan->stream));
  e.has_intensity = true;
  rc = kf_push(kf, std::move(e), id);
  if (rc) return rc;
  ++kf->device_copies;
  return GORIO_OK;
}

int gorio_kf_add_from_apd(gorio_kf_t* kf, gorio_apd_t* apd, int which, const float* intensity, int intensity_stride_bytes, int* id) {
  if (!kf || !apd || !id) return kf_fail(GORIO_ERR_INVALID, "add_from_apd: null argument");
  if (which != 0 && which != 1) return kf_fail(GORIO_ERR_INVALID, "add_from_apd: which must be 0 (source) or 1 (target)");
  if (intensity && (intensity_stride_bytes < 4 || (intensity_stride_bytes % 4) != 0)) return kf_fail(GORIO_ERR_INVALID, "add_from_apd: bad intensity stride");
  if (kf->device != apd->device) return kf_fail(GORIO_ERR_INVALID, "add_from_apd: the store and the registration handle must live on one device");
  const std::shared_ptr<DevCloud>& c = which == 0 ? apd->src : apd->tgt;
  if (!c->present) return kf_fail(GORIO_ERR_STATE, which == 0 ? "add_from_apd: the registration handle has no input source" : "add_from_apd: the registration handle has no input target");
  int rc = kf_ensure_device(kf, "add_from_apd");
  if (rc) return rc;
  GORIO_HIP_CHECK(kf_fail, hipSetDevice(kf->device));
  KfEntry e;
  e.cloud = c;  // points, labels, covariances with their (k, regularization), search index, voxel map: one copy on the device
  e.n = c->n;
  if (intensity) {
    GORIO_HIP_CHECK(kf_fail, e.intensity.reserve(e.n));
    std::vector<float> col((size_t)e.n);
    const size_t st = intensity_stride_bytes / 4;
    for (int i = 0; i < e.n; ++i) col[i] = intensity[st * i];
    GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(e.intensity, col.data(), sizeof(float) * (size_t)e.n, hipMemcpyHostToDevice, kf->up->stream));
    GORIO_HIP_CHECK(kf_fail, hipStreamSynchronize(kf->up->stream));  // col is pageable
    e.has_intensity = true;
  }
  return kf_push(kf, std::move(e), id);
}

int gorio_kf_release(gorio_kf_t* kf, int id) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "release: null handle");
  int rc = GORIO_OK;
  std::string why;
  if (!kf_entry(kf, id, &rc, &why)) return kf_fail(rc, "release: " + why);
  hipSetDevice(kf->device);
  hipStreamSynchronize(kf->up->stream);  // nothing in flight reads the buffers about to be freed
  KfEntry& e = kf->kfs[id];
  e.cloud.reset();
  e.intensity.reset();
  e.has_intensity = false;
  e.n = 0;
  return GORIO_OK;
}

int gorio_kf_count(const gorio_kf_t* kf, int* n_added, int* n_resident) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "count: null handle");
  if (n_added) *n_added = (int)kf->kfs.size();
  if (n_resident) {
    int r = 0;
    for (const KfEntry& e : kf->kfs) r += e.cloud ? 1 : 0;
    *n_resident = r;
  }
  return GORIO_OK;
}

int gorio_kf_info(const gorio_kf_t* kf, int id, gorio_kf_info_t* out) {
  if (!kf || !out) return kf_fail(GORIO_ERR_INVALID, "info: null argument");
  if (id < 0 || id >= (int)kf->kfs.size()) return kf_fail(GORIO_ERR_INVALID, "info: keyframe " + std::to_string(id) + " has not been added");
  std::memset(out, 0, sizeof(*out));
  const KfEntry& e = kf->kfs[id];
  if (!e.cloud) return GORIO_OK;
  const DevCloud& c = *e.cloud;
  out->n = e.n;
  out->resident = 1;
  out->has_intensity = e.has_intensity ? 1 : 0;
  out->cov_count = (e.n > 0 && c.cov_count == c.n) ? c.cov_count : 0;
  out->cov_k = out->cov_count ? c.cov_k : 0;
  out->cov_reg = out->cov_count ? c.cov_reg : 0;
  out->index_built = (e.n > 0 && c.idx_valid) ? 1 : 0;
  out->sharers = (int)e.cloud.use_count() - 1;
  return GORIO_OK;
}

int gorio_kf_get(gorio_kf_t* kf, int id, float* xyz, float* intensity, float* label, int stride_bytes, int capacity) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "get: null handle");
  if (stride_bytes < 4 || (stride_bytes % 4) != 0 || (xyz && stride_bytes < 12) || capacity < 0) return kf_fail(GORIO_ERR_INVALID, "get: bad arguments");
  int rc = GORIO_OK;
  std::string why;
  const KfEntry* e = kf_entry(kf, id, &rc, &why);
  if (!e) return kf_fail(rc, "get: " + why);
  if (capacity < e->n) return kf_fail(GORIO_ERR_INVALID, "get: capacity too small");
  if (intensity && !e->has_intensity) return kf_fail(GORIO_ERR_STATE, "get: keyframe " + std::to_string(id) + " has no intensity column");
  const int n = e->n;
  ++kf->point_downloads;
  if (n == 0) return GORIO_OK;
  GORIO_HIP_CHECK(kf_fail, hipSetDevice(kf->device));
  std::vector<float4> pts((size_t)n);
  std::vector<float> col(intensity ? (size_t)n : 0);
  hipStream_t st = kf->up->stream;
  GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(pts.data(), e->cloud->p4, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
  if (intensity) GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(col.data(), e->intensity, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(kf_fail, hipStreamSynchronize(st));
  const size_t s = stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    if (xyz) {
      xyz[s * i] = pts[i].x;
      xyz[s * i + 1] = pts[i].y;
      xyz[s * i + 2] = pts[i].z;
    }
    if (intensity) intensity[s * i] = col[i];
    if (label) label[s * i] = pts[i].w;
  }
  return GORIO_OK;
}

int gorio_kf_get_counters(const gorio_kf_t* kf, long long* point_uploads, long long* point_downloads, long long* device_copies) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "get_counters: null handle");
  if (point_uploads) *point_uploads = kf->point_uploads;
  if (point_downloads) *point_downloads = kf->point_downloads;
  if (device_copies) *device_copies = kf->device_copies;
  return GORIO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ consumers

// SMO:588, LD:222, LD:391: a pointer share with the checks of gorio_apd_set_target_shared
static int kf_hand_off(gorio_apd* apd, gorio_kf* kf, int id, bool source) {
  if (!apd) return GORIO_ERR_INVALID;
  const std::string what = source ? "set_source_from_keyframe: " : "set_target_from_keyframe: ";
  if (!kf) return fail(apd, GORIO_ERR_INVALID, what + "null keyframe store");
  if (apd->device != kf->device) return fail(apd, GORIO_ERR_INVALID, what + "the handle and the store must live on one device");
  int rc = GORIO_OK;
  std::string why;
  const KfEntry* e = kf_entry(kf, id, &rc, &why);
  if (!e) return fail(apd, rc, what + why);
  if (e->n <= 0) return fail(apd, GORIO_ERR_INVALID, what + "bad cloud arguments (the keyframe is empty)");
  const DevCloud& c = *e->cloud;
  if (cov_rule_differs(apd, c))
    return fail(apd, GORIO_ERR_INVALID, what + "the keyframe's covariances were estimated with another k_correspondences / regularization than this handle's");
  if (!source && apd->method == GORIO_METHOD_VGICP && c.vm_valid && (c.vm.res != apd->voxel_resolution || c.vm_mult != (apd->voxel_mode == GORIO_VOXEL_MULTIPLICATIVE)))
    return fail(apd, GORIO_ERR_INVALID, what + "the keyframe's voxel map was built with another voxel_resolution / voxel_mode than this handle's");
  (source ? apd->src : apd->tgt) = e->cloud;  // points, covariances, search index, voxel map: one copy on the device, alive until the last holder lets go of it
  apd->corr_valid = false;
  return GORIO_OK;
}
int gorio_apd_set_source_from_keyframe(gorio_apd_t* apd, gorio_kf_t* kf, int id) { return kf_hand_off(apd, kf, id, true); }
int gorio_apd_set_target_from_keyframe(gorio_apd_t* apd, gorio_kf_t* kf, int id) { return kf_hand_off(apd, kf, id, false); }

// LD:222, LD:391 with NDT_OMP: a copy of x, y, z through ndt_adopt, ordered behind the stream the keyframe was last written on
static int kf_ndt_hand_off(gorio_ndt* ndt, gorio_kf* kf, int id, bool source) {
  const std::string what = source ? "set_source_from_keyframe" : "set_target_from_keyframe";
  if (!ndt) return ndt_fail(GORIO_ERR_INVALID, what + ": null handle");
  if (!kf) return ndt_fail(GORIO_ERR_INVALID, what + ": null keyframe store");
  if (ndt->device != kf->device) return ndt_fail(GORIO_ERR_INVALID, what + ": the handle and the store must live on one device");
  int rc = GORIO_OK;
  std::string why;
  const KfEntry* e = kf_entry(kf, id, &rc, &why);
  if (!e) return ndt_fail(rc, what + ": " + why);
  const DevCloud& c = *e->cloud;
  rc = ndt_adopt(ndt, c.x, c.y, c.z, e->n, kf->up->stream, source, what);
  if (rc == GORIO_OK) ++kf->device_copies;
  return rc;
}
int gorio_ndt_set_source_from_keyframe(gorio_ndt_t* ndt, gorio_kf_t* kf, int id) { return kf_ndt_hand_off(ndt, kf, id, true); }
int gorio_ndt_set_target_from_keyframe(gorio_ndt_t* ndt, gorio_kf_t* kf, int id) { return kf_ndt_hand_off(ndt, kf, id, false); }

// SMO:602-618
int gorio_apd_set_target_submap_keyframes(gorio_apd_t* h, gorio_kf_t* kf, const int* ids, const double* rel_poses, int count, double voxel_leaf, int* n_target) {
  if (!h) return GORIO_ERR_INVALID;
  const std::string what = "set_target_submap_keyframes: ";
  if (!kf || !ids || !rel_poses || count <= 0) return fail(h, GORIO_ERR_INVALID, what + "null argument or count <= 0");
  if (h->device != kf->device) return fail(h, GORIO_ERR_INVALID, what + "the handle and the store must live on one device");
  std::vector<gorio::KfFrame> fr(count);
  long long total = 0, nblocks = 0;
  int max_blocks = 0;
  for (int k = 0; k < count; ++k) {
    int rc = GORIO_OK;
    std::string why;
    const KfEntry* e = kf_entry(kf, ids[k], &rc, &why);
    if (!e) return fail(h, rc, what + why);
    const int nb = (e->n + 255) / 256;
    fr[k].p4 = e->n > 0 ? e->cloud->p4.get() : nullptr;
    fr[k].n = e->n;
    fr[k].blk0 = (int)nblocks;
    for (int q = 0; q < 12; ++q) fr[k].T[q] = rel_poses[(size_t)k * 16 + q];
    total += e->n;
    nblocks += nb;
    max_blocks = std::max(max_blocks, nb);
  }
  if (total > (long long)INT_MAX / 2) return fail(h, GORIO_ERR_INVALID, what + "too many points");
  if (total == 0) return fail(h, GORIO_ERR_INVALID, "set_target_submap: no finite point in any keyframe");
  HIP_TRY(h, hipSetDevice(h->device));
  {
    const size_t cap = (size_t)total + (size_t)total / 8;  // at most `total` points survive
    HIP_TRY(h, reserve_group(h->sub_cap, (size_t)total, cap, h->d_sub_in, cap, h->d_sub_out, cap, h->d_sub_vox, cap));
  }
  const size_t fbytes = sizeof(gorio::KfFrame) * (size_t)count;
  HIP_TRY(h, h->d_sub_kframes.reserve(fbytes, fbytes + fbytes / 2));
  HIP_TRY(h, h->d_sub_kcnt.reserve((size_t)nblocks + 1, (size_t)nblocks + 1 + (size_t)nblocks / 8));
  HIP_TRY(h, h->d_sub_bb.reserve(8));
  const gorio::KfFrame* d_fr = static_cast<const gorio::KfFrame*>(h->d_sub_kframes.get());
  HIP_TRY(h, hipMemcpyAsync(h->d_sub_kframes, fr.data(), fbytes, hipMemcpyHostToDevice, h->stream));
  const dim3 grid(max_blocks, count);
  gorio::kf_submap_count_kernel<<<grid, 256, 0, h->stream>>>(d_fr, h->d_sub_kcnt);
  gorio::block_scan_kernel<<<1, 1024, 0, h->stream>>>(h->d_sub_kcnt, (int)nblocks);
  gorio::kf_submap_scatter_kernel<<<grid, 256, 0, h->stream>>>(d_fr, h->d_sub_kcnt, h->d_sub_out);
  HIP_TRY(h, hipGetLastError());
  int m = 0;
  HIP_TRY(h, hipMemcpyAsync(&m, h->d_sub_kcnt.get() + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // also covers the pageable frame table
  if (m <= 0) return fail(h, GORIO_ERR_INVALID, "set_target_submap: no finite point in any keyframe");
  return submap_finish(h, m, voxel_leaf, n_target);
}

// RGS:727-731
int gorio_sc_add_keyframes(gorio_sc_t* h, gorio_kf_t* kf, const int* ids, int count, int* first_index_out) {
  if (!h) return sc_fail(GORIO_ERR_INVALID, "add_keyframes: null handle");
  if (!kf || !ids || count <= 0) return sc_fail(GORIO_ERR_INVALID, "add_keyframes: null argument or count <= 0");
  if (h->device != kf->device) return sc_fail(GORIO_ERR_INVALID, "add_keyframes: the handle and the store must live on one device");
  std::vector<gorio::KfScJob> jobs(count);
  size_t ntot = 0;
  int max_blocks = 1;
  for (int s = 0; s < count; ++s) {
    int rc = GORIO_OK;
    std::string why;
    const KfEntry* e = kf_entry(kf, ids[s], &rc, &why);
    if (!e) return sc_fail(rc, "add_keyframes: " + why);
    if (e->n > 0 && !e->has_intensity) return sc_fail(GORIO_ERR_STATE, "add_keyframes: keyframe " + std::to_string(ids[s]) + " has no intensity column");
    jobs[s].p4 = e->n > 0 ? e->cloud->p4.get() : nullptr;
    jobs[s].intensity = e->n > 0 ? e->intensity.get() : nullptr;
    jobs[s].n = e->n;
    jobs[s].off = (int)ntot;
    ntot += e->n;
    if (ntot > (size_t)INT_MAX / 2) return sc_fail(GORIO_ERR_INVALID, "add_keyframes: too many points or scans");
    max_blocks = std::max(max_blocks, (e->n + 255) / 256);
  }
  if ((size_t)h->n + count > (size_t)INT_MAX / 2) return sc_fail(GORIO_ERR_INVALID, "add_keyframes: too many points or scans");
  const size_t b_pts = sizeof(float4) * ntot, b_off = sizeof(int) * ((size_t)count + 1), b_jobs = sizeof(gorio::KfScJob) * (size_t)count;
  GORIO_HIP_CHECK(sc_fail, hipSetDevice(h->device));
  if (sc_grow_db(h, (size_t)h->n + count)) return GORIO_ERR_NO_DEVICE;
  GORIO_HIP_CHECK(sc_fail, h->d_in.reserve(b_pts + b_off, (b_pts + b_off) + (b_pts + b_off) / 2));
  GORIO_HIP_CHECK(sc_fail, h->d_kfjobs.reserve(b_jobs, b_jobs + b_jobs / 2));
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(kf->up->stream));  // the keyframes were written on the device's launch stream, this handle has its own
  float4* d_pts = (float4*)h->d_in.get();
  int* d_off = (int*)((char*)h->d_in.get() + b_pts);
  GORIO_HIP_CHECK(sc_fail, hipMemcpyAsync(h->d_kfjobs, jobs.data(), b_jobs, hipMemcpyHostToDevice, h->stream));
  gorio::kf_sc_pack_kernel<<<dim3(max_blocks, count), 256, 0, h->stream>>>(static_cast<const gorio::KfScJob*>(h->d_kfjobs.get()), count, (int)ntot, d_pts, d_off);
  hipLaunchKernelGGL(gorio::sc_descriptor_kernel, dim3(count), dim3(gorio::kScThreads), 0, h->stream, (const float4*)d_pts, (const int*)d_off, h->n, h->p.azimuth_range, h->db());
  GORIO_HIP_CHECK(sc_fail, hipGetLastError());
  GORIO_HIP_CHECK(sc_fail, hipStreamSynchronize(h->stream));  // also covers the pageable job table
  if (first_index_out) *first_index_out = h->n;
  h->n += count;
  ++kf->device_copies;
  return GORIO_OK;
}

// ------------------------------------------------------------------------------------------------- pose-graph edges (include/gorio_kf_edges.h)

// IMC:55-86 for `count` edges.  who: the entry point's name for the error text.
static int kf_edge_fitness_impl(gorio_kf* kf, const char* who, const gorio_kf_edge* edges, int count, double max_range, double* score, long long* n_in_range) {
  const std::string what = std::string(who) + ": ";
  if (count > 65535) return kf_fail(GORIO_ERR_UNSUPPORTED, what + std::to_string(count) + " edges in one call (at most 65535: one edge is one grid row)");
  if (std::isnan(max_range)) return kf_fail(GORIO_ERR_INVALID, what + "max_range is NaN");
  // every check, then the sizes: nothing below this block can refuse an argument
  struct Slice {
    int e;  // index into edges[]
    size_t key_off, seed_off, work_off, plan_off, blk0;
  };
  std::vector<Slice> live;  // the edges with points on both sides, in the caller's order
  std::vector<std::pair<gorio_apd*, DevCloud*>> clouds;
  size_t n_keys = 0, n_seed = 0, n_work = 0, n_plan = 0, n_blk = 0;
  long long total_src = 0, total_waves = 0;
  int max_n = 1, max_nbx = 1, max_spad = 512;
  try {
    for (int e = 0; e < count; ++e) {
      const std::string at = what + "edges[" + std::to_string(e) + "]: ";
      int rc = GORIO_OK;
      std::string why;
      const KfEntry* t = kf_entry(kf, edges[e].target_id, &rc, &why);
      if (!t) return kf_fail(rc, at + "target: " + why);
      const KfEntry* s = kf_entry(kf, edges[e].source_id, &rc, &why);
      if (!s) return kf_fail(rc, at + "source: " + why);
      for (int q = 0; q < 16; ++q)
        if (!std::isfinite(edges[e].relpose[q])) return kf_fail(GORIO_ERR_INVALID, at + "relpose[" + std::to_string(q) + "] is not finite");
      total_src += s->n;
      if (total_src > (long long)INT_MAX) return kf_fail(GORIO_ERR_UNSUPPORTED, at + "more than 2^31 - 1 source points over the edges of one call");
      if (s->n <= 0 || t->n <= 0) continue;  // scores DBL_MAX below, takes no part in the launches
      const int spad = roundup(s->n, 512), wcap = spad / 64;
      live.push_back(Slice{e, n_keys, n_seed, n_work, n_plan, n_blk});
      n_keys += (size_t)s->n;
      n_seed += (size_t)spad;
      n_work += 2 * (size_t)wcap;
      n_plan += 1 + 16 * (size_t)wcap;
      n_blk += (size_t)((s->n + 255) / 256);
      total_waves += (s->n + 63) / 64;
      max_n = std::max(max_n, s->n);
      max_nbx = std::max(max_nbx, (s->n + 255) / 256);
      max_spad = std::max(max_spad, spad);
      clouds.emplace_back(kf->up, s->cloud.get());
      clouds.emplace_back(kf->up, t->cloud.get());
    }
  } catch (const std::bad_alloc&) {
    return kf_fail(GORIO_ERR_ALLOC, what + "out of memory");
  }
  int rc = kf_ensure_device(kf, who);  // (a store that holds a keyframe has its device side already)
  if (rc) return rc;
  for (int e = 0; e < count; ++e) {
    score[e] = DBL_MAX;  // IMC:85
    if (n_in_range) n_in_range[e] = 0;
  }
  const int m = (int)live.size();
  if (m == 0) {  // nothing but empty keyframes: nothing to launch, nothing to wait for
    ++kf->edge_calls;
    kf->edge_edges += count;
    return GORIO_OK;
  }
  GORIO_HIP_CHECK(kf_fail, hipSetDevice(kf->device));
  gorio_apd* up = kf->up;
  hipStream_t st = up->stream;
  {  // ONE index build for the keyframes that lack one; a keyframe named by many edges is one cloud
    std::unordered_set<DevCloud*> lacking;
    for (auto& c : clouds)
      if (!c.second->idx_valid) lacking.insert(c.second);
    rc = run_index_build(up, clouds);
    if (rc) return kf_fail(rc, what + up->err);
    kf->edge_index_builds += (long long)lacking.size();
  }
  const size_t b_desc = sizeof(PairDesc) * (size_t)m, b_tab = b_desc + sizeof(PairState) * (size_t)m, b_out = sizeof(double) * 2 * n_blk;
  GORIO_HIP_CHECK(kf_fail, kf->e_keys.reserve(n_keys, n_keys + n_keys / 8));
  GORIO_HIP_CHECK(kf_fail, kf->e_seed.reserve(n_seed, n_seed + n_seed / 8));
  GORIO_HIP_CHECK(kf_fail, kf->e_work.reserve(n_work, n_work + n_work / 8));
  GORIO_HIP_CHECK(kf_fail, kf->e_plan.reserve(n_plan, n_plan + n_plan / 8));
  GORIO_HIP_CHECK(kf_fail, kf->e_fit.reserve(2 * n_blk, 2 * n_blk + n_blk / 4));
  GORIO_HIP_CHECK(kf_fail, kf->e_tab.reserve(b_tab, b_tab + b_tab / 2));
  GORIO_HIP_CHECK(kf_fail, kf->e_pin.reserve(b_tab, b_tab + b_tab / 2));
  GORIO_HIP_CHECK(kf_fail, kf->e_out.reserve(b_out, b_out + b_out / 2));
  static_assert(sizeof(PairDesc) % 8 == 0, "the states follow the descriptors in one table");
  PairDesc* h_desc = static_cast<PairDesc*>(kf->e_pin.get());
  PairState* h_state = reinterpret_cast<PairState*>(static_cast<char*>(kf->e_pin.get()) + b_desc);
  PairDesc* d_desc = static_cast<PairDesc*>(kf->e_tab.get());
  PairState* d_state = reinterpret_cast<PairState*>(static_cast<char*>(kf->e_tab.get()) + b_desc);
  for (int k = 0; k < m; ++k) {
    const Slice& sl = live[k];
    const gorio_kf_edge& ed = edges[sl.e];
    const DevCloud& src = *kf->kfs[ed.source_id].cloud;
    const DevCloud& tgt = *kf->kfs[ed.target_id].cloud;
    PairDesc& d = h_desc[k];
    std::memset(&d, 0, sizeof(d));
    d.src = src.view();
    d.tgt = tgt.view();
    d.best_key = kf->e_keys.get() + sl.key_off;
    d.seed = kf->e_seed.get() + sl.seed_off;
    d.nn_work = kf->e_work.get() + sl.work_off;
    d.nn_plan = kf->e_plan.get() + sl.plan_off;
    d.nn_wcap = roundup(src.n, 512) / 64;
    d.partials = kf->e_fit.get() + 2 * sl.blk0;  // this edge's slice of the block partials (kf_edge_reduce_kernel)
    d.state = d_state + k;
    d.nblk = (src.n + 255) / 256;
    d.nn_splits = 1;  // (the exhaustive search's split of the target: not launched here)
    d.nn_chunk = std::max(512, roundup(tgt.n_pad, kPad));
    d.shard_lo = 0;
    d.shard_hi = INT_MAX;
    // relpose.cast<float>() (IMC:63), then exactly what gorio_apd_fitness_score makes of a float pose
    float Tf[16];
    double Td[16];
    for (int q = 0; q < 16; ++q) {
      Tf[q] = (float)ed.relpose[q];
      Td[q] = (double)Tf[q];
    }
    init_state(h_state[k], Td);
    for (int q = 0; q < 12; ++q) h_state[k].Tf[q] = Tf[q];
  }
  GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(kf->e_tab.get(), kf->e_pin.get(), b_tab, hipMemcpyHostToDevice, st));
  arm_keys_kernel<<<dim3(std::min(64, (max_n + 255) / 256), m), 256, 0, st>>>(d_desc);
  launch_pruned(dim3(max_spad / 256, fitness_splits((long)total_waves), m), st, d_desc, fitness_bound(max_range, 0.0), 0);
  gorio::kf_edge_reduce_kernel<<<dim3(max_nbx, m), 256, 0, st>>>(d_desc, max_range);
  GORIO_HIP_CHECK(kf_fail, hipGetLastError());
  GORIO_HIP_CHECK(kf_fail, hipMemcpyAsync(kf->e_out.get(), kf->e_fit.get(), b_out, hipMemcpyDeviceToHost, st));
  GORIO_HIP_CHECK(kf_fail, hipStreamSynchronize(st));
  ++kf->edge_syncs;
  ++kf->edge_calls;
  kf->edge_edges += count;
  const double* part = static_cast<const double*>(kf->e_out.get());
  for (int k = 0; k < m; ++k) {
    const Slice& sl = live[k];
    const int nbx = h_desc[k].nblk;
    double sum = 0.0, cnt = 0.0;
    for (int bk = 0; bk < nbx; ++bk) {  // block order, as gorio_apd_fitness_score adds them
      sum += part[2 * (sl.blk0 + bk)];
      cnt += part[2 * (sl.blk0 + bk) + 1];
    }
    score[sl.e] = cnt > 0 ? sum / cnt : DBL_MAX;
    if (n_in_range) n_in_range[sl.e] = (long long)cnt;
  }
  return GORIO_OK;
}

int gorio_kf_edge_fitness(gorio_kf_t* kf, const gorio_kf_edge* edges, int count, double max_range, double* score, long long* n_in_range) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "edge_fitness: null handle");
  if (count < 0) return kf_fail(GORIO_ERR_INVALID, "edge_fitness: count < 0");
  if (count == 0) return GORIO_OK;
  if (!edges || !score) return kf_fail(GORIO_ERR_INVALID, "edge_fitness: null argument");
  return kf_edge_fitness_impl(kf, "edge_fitness", edges, count, max_range, score, n_in_range);
}

void gorio_kf_default_inf_params(gorio_inf_params* p) {
  if (!p) return;
  p->use_const_inf_matrix = 0;  // IMC:15-24
  p->const_stddev_x = 0.5;
  p->const_stddev_q = 0.1;
  p->var_gain_a = 20.0;
  p->min_stddev_x = 0.1;
  p->max_stddev_x = 5.0;
  p->min_stddev_q = 0.05;
  p->max_stddev_q = 0.2;
  p->fitness_score_thresh = 0.5;
}

int gorio_kf_edge_information(gorio_kf_t* kf, const gorio_inf_params* p, const gorio_kf_edge* edges, int count, double* inf_diag, double* score) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "edge_information: null handle");
  if (!p) return kf_fail(GORIO_ERR_INVALID, "edge_information: null parameters");
  if (count < 0) return kf_fail(GORIO_ERR_INVALID, "edge_information: count < 0");
  if (count == 0) return GORIO_OK;
  if (!inf_diag) return kf_fail(GORIO_ERR_INVALID, "edge_information: null argument");
  if (p->use_const_inf_matrix) {  // IMC:30-35: neither cloud is looked at
    for (int e = 0; e < count; ++e) gorio::edge_information_from_score(*p, 0.0, inf_diag + 2 * (size_t)e);
    return GORIO_OK;
  }
  if (!edges) return kf_fail(GORIO_ERR_INVALID, "edge_information: null argument");
  std::vector<double> own;
  if (!score) {
    try {
      own.resize((size_t)count);
    } catch (const std::bad_alloc&) {
      return kf_fail(GORIO_ERR_ALLOC, "edge_information: out of memory");
    }
    score = own.data();
  }
  const int rc = kf_edge_fitness_impl(kf, "edge_information", edges, count, DBL_MAX, score, nullptr);  // IMC:37: max_range at its default
  if (rc) return rc;
  for (int e = 0; e < count; ++e) gorio::edge_information_from_score(*p, score[e], inf_diag + 2 * (size_t)e);
  return GORIO_OK;
}

int gorio_kf_edge_counters(const gorio_kf_t* kf, long long* calls, long long* edges_scored, long long* index_builds, long long* synchronisations) {
  if (!kf) return kf_fail(GORIO_ERR_INVALID, "edge_counters: null handle");
  if (calls) *calls = kf->edge_calls;
  if (edges_scored) *edges_scored = kf->edge_edges;
  if (index_builds) *index_builds = kf->edge_index_builds;
  if (synchronisations) *synchronisations = kf->edge_syncs;
  return GORIO_OK;
}

}  // extern "C"
