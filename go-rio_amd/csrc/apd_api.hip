// apd_api.hip -- host side of the APD-GICP C ABI declared in include/gorio_apd.h.
//
// One gorio_apd handle == one fast_gicp::FastAPDGICP object (APDH:20-122): it owns the device copies of the two clouds,
// their covariances, the per-source-point correspondence state and the device-resident optimiser state, and it drives
// the kernels of apd_kernels.hip.  No CPU compute path exists here: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/gorio_apd.h"
#include "dev_buffer.h"

// THE check of a HIP call in every host module of this translation unit: on an error, return through the module's fail function
// (`fail_fn` is anything callable as fail_fn(code, message)) with "<expression>: <hipGetErrorString>".
#define GORIO_HIP_CHECK(fail_fn, expr)                                                                             \
  do {                                                                                                           \
    hipError_t e_ = (expr);                                                                                      \
    if (e_ != hipSuccess) return fail_fn(GORIO_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

#include "apd_kernels.hip"
#include "apd_index.hip"
#include "apd_voxel_group.hip"
#include "apd_submap.hip"
#include "apd_approx_voxel.hip"
#include "apd_voxel.hip"
#include "apd_ndt_cuda.hip"
#include "apd_vgicp_cuda.hip"
#include "apd_ground.hip"
#include "../../include/gorio_sc.h"
#include "apd_sc.hip"
#include "apd_sc_pairs.hip"
#include "apd_sc_cross.hip"
#include "../../include/gorio_ndt.h"
#include "apd_ndt.hip"

using namespace gorio;

namespace {

constexpr int kPad = 16;
constexpr float kFar = 1e30f;

// One Gaussian voxel map on the device (VoxMapView<Real> is its kernel-visible view): the occupied voxels in ascending id order, and the
// box of occupied coordinates that the ids are linear in.  What it is valid FOR (settings, the state of the cloud) is its owner's business.
template <typename Real>
struct VoxMap {
  DevBuf<unsigned long long> vkey;  // these four hold `cap` voxels
  DevBuf<Real> mean, cov6;
  DevBuf<int> num;
  int cap = 0, nv = 0;
  int min[3] = {0, 0, 0}, dim[3] = {0, 0, 0};
  Real res = 0;
  hipError_t reserve(int n_voxels) {
    const size_t c = n_voxels + n_voxels / 8 + 64;
    return reserve_group(cap, n_voxels, c, vkey, c, mean, 3 * c, cov6, 6 * c, num, c);
  }
  void set_geometry(const CellBox<Real>& g, int n_voxels) {
    nv = n_voxels;
    for (int a = 0; a < 3; ++a) {
      min[a] = g.min_c[a];
      dim[a] = g.dim[a];
    }
    res = g.res;
  }
  VoxMapView<Real> view() const { return VoxMapView<Real>{vkey, mean, cov6, num, nv, {min[0], min[1], min[2]}, {dim[0], dim[1], dim[2]}, res}; }
  // host: (cx, cy, cz) of the nv linear ids `ids` (a download of vkey) -> coords [nv][3]
  void decode_coords(const unsigned long long* ids, int* coords) const {
    const unsigned long long d1 = (unsigned long long)dim[1], d2 = (unsigned long long)dim[2];
    for (int v = 0; v < nv; ++v) {
      const unsigned long long id = ids[v];
      coords[3 * (size_t)v + 2] = (int)(id % d2) + min[2];
      coords[3 * (size_t)v + 1] = (int)((id / d2) % d1) + min[1];
      coords[3 * (size_t)v] = (int)(id / (d2 * d1)) + min[0];
    }
  }
};

// scratch of a cell grouping (voxel_cell_starts): the three maps of a cloud are built one after the other on one stream and share it
struct VoxScratch {
  DevBuf<unsigned long long> keys;  // linear voxel id << 31 | point index, sorted
  DevBuf<int> counts;               // voxel starts per 256 keys, scanned; [blocks] is the voxel count
  DevBuf<int> bb;                   // [8] bounding box of the occupied coordinates + range flag
};

struct DevCloud {
  int device = 0;          // first member: ~DevCloud selects it before the buffers below free themselves
  DevBuf<float> x, y, z, label;  // the point group: these, p4, cov6 and geo_w share `cap`
  DevBuf<float4> p4;
  DevBuf<double> cov6, geo_w;
  DevBuf<int> knn;         // [cap][knn_k] neighbour indices of the last covariance computation (parity hook, params.keep_knn_indices)
  DevBuf<int> redo;        // per query wave: redo flags of knn_collect_kernel
  DevBuf<float> kth;       // per sorted position: k-th distance (knn_kth_kernel)
  int redo_cap = 0;        // query waves redo / kth hold
  DevBuf<float> part_d;    // k-NN partial lists
  DevBuf<int> part_i;
  size_t part_cap = 0;     // elements of part_d / part_i
  int knn_k = 0;
  bool knn_valid = false;  // knn holds the lists of the current covariances
  int n = 0, n_pad = 0, cap = 0;
  bool present = false;
  int cov_count = 0;       // == source_covs_.size(): n when valid, 0 when stale
  int cov_k = -1, cov_reg = -1;  // k_correspondences / regularization the covariances were ESTIMATED with; -1: supplied by set_*_covariances
  double cov_eps = 0.0;    // gicp_epsilon of covariances estimated by the GICP_OMP rule (cov_reg == kRegGicpOmp), 0 otherwise
  // exact search accelerator (GORIO_SEARCH_PRUNED)
  DevBuf<float> idx_sx, idx_sy, idx_sz, idx_tbox, idx_sbox, idx_bbox;  // the arrays behind index_view(): one group of capacity idx_cap
  DevBuf<int> idx_orig;
  DevBuf<float4> idx_s4;
  int idx_cap = 0;
  int idx_n = 0, idx_spad = 0;  // sizes of the index held (SearchIndex::n / n_spad)
  DevBuf<unsigned long long> keys;
  DevBuf<unsigned int> bb;
  bool idx_valid = false;
  int idx_chunk = 0;       // kd chunk size the index was built with (gorio_apd_debug_get_index)
  // Gaussian voxel map of this cloud as a FastVGICP target (voxelmap_, fast_vgicp.hpp:85): lives with the cloud, so the handles that share a
  // target share its map.  Valid for (vm.res, vm_mult) until the points or the covariances change.
  VoxScratch vox_scratch;
  VoxMap<double> vm;
  bool vm_mult = false;                   // MultiplicativeGaussianVoxel (ADDITIVE and ADDITIVE_WEIGHTED build the same voxels, VOX:138-141)
  bool vm_valid = false;
  // float Gaussian voxel map of this cloud for fast_gicp::NDTCuda (apd_ndt_cuda.hip; source_voxelmap / target_voxelmap, ndt_cuda.cu:120-140):
  // lives with the cloud, so a swap moves it and the sharers of a target share it.  Built from the points alone; valid for nc.res until the points change.
  VoxMap<float> nc;                    // cov6: the regularised covariance
  DevBuf<float> nc_raw;                // [nc.cap][9] the covariance before the regularisation (GV:188), row-major
  bool nc_valid = false;
  // fast_gicp::FastVGICPCuda (apd_vgicp_cuda.hip): three stages, each valid for the settings recorded beside it until the points change.
  //   raw   float covariances of ALL points (source_covariances / target_covariances, VC:183-219) from the k-NN lists (vc_knn) or the RBF pass
  //   kept  the points the regularisation keeps, in input order, with their regularised covariances (CR:91-117)
  //   map   the voxel map of the kept points that averages their covariances (GV:229-252); built for a target only
  // They live with the cloud: a swap moves them, the sharers of a cloud share them.
  DevBuf<float> vc_raw6, vc_reg6;      // the point group of this method: these, vc_keep, vc_p4, vc_cov6, vc_index hold vc_cap points
  DevBuf<unsigned char> vc_keep;
  DevBuf<float4> vc_p4;                // kept points
  DevBuf<float> vc_cov6;               // [vc_nkept][6]
  DevBuf<int> vc_index;                // [vc_nkept] input index of a kept point
  int vc_cap = 0, vc_nkept = 0;
  DevBuf<int> vc_knn, vc_bcnt;         // [n][k] lists; kept points per 256, scanned
  DevBuf<double> vc_scratch;           // [n][7] the double covariances and weights the k-NN kernels make on their way to the lists
  DevBuf<float> vc_part;               // RBF block partials [blocks][10][n]
  bool vc_raw_valid = false, vc_kept_valid = false, vc_map_valid = false;
  int vc_rbf = 0, vc_k = 0, vc_reg = -1;  // what raw / kept were made with: RBF or lists, k (lists), kernel_width and max_dist (RBF), regularization
  double vc_width = 0.0, vc_maxd = 0.0;
  VoxMap<float> vc_map;                // the map
  // fast_gicp::FastGICPMultiPoints (apd_gicp_mp.hip): every point with its float covariance as a record of three float4, made from the k-NN
  // lists mp_knn (mp_scratch: what the k-NN kernels write on their way to the lists).  Valid for (mp_k, mp_reg) until the points change;
  // lives with the cloud, so a swap moves it and the sharers of a cloud share it.
  DevBuf<float4> mp_rec;               // [n][3]
  DevBuf<int> mp_knn;                  // [n][k]
  DevBuf<double> mp_scratch;           // [n][7]
  bool mp_valid = false;
  int mp_k = 0, mp_reg = -1;
  // What is derived from what: covariances, search index, voxel map and k-NN lists from the points; the voxel map and the k-NN lists from
  // the covariances too.  New points leave all four stale, new covariances the last two.  These members are the ONLY code that writes
  // present, cov_count, cov_k, cov_reg, idx_valid, idx_chunk, vm_valid, nc_valid, knn_valid, the three vc_*_valid and mp_valid; everybody else reads them.
  void covs_dropped() { cov_count = 0; vm_valid = false; knn_valid = false; }
  void points_replaced() { present = true; idx_valid = false; nc_valid = false; vgc_raw_dropped(); mp_dropped(); covs_dropped(); }
  void cleared() { present = false; n = 0; idx_valid = false; nc_valid = false; vgc_raw_dropped(); mp_dropped(); covs_dropped(); }
  void mp_dropped() { mp_valid = false; }
  void mp_built(int k, int reg) { mp_valid = true; mp_k = k; mp_reg = reg; }
  void vgc_raw_dropped() { vc_raw_valid = false; vgc_kept_dropped(); }
  void vgc_kept_dropped() { vc_kept_valid = false; vc_map_valid = false; }
  void vgc_map_dropped() { vc_map_valid = false; }
  void vgc_raw_built(bool rbf, int k, double width, double maxd) { vc_raw_valid = true; vc_rbf = rbf ? 1 : 0; vc_k = k; vc_width = width; vc_maxd = maxd; }
  void vgc_kept_built(int reg, int nkept) { vc_kept_valid = true; vc_reg = reg; vc_nkept = nkept; }
  void vgc_map_built() { vc_map_valid = true; }
  void ndtc_map_dropped() { nc_valid = false; }
  void ndtc_map_built() { nc_valid = true; }
  void covs_estimated(int k, int reg, bool keep_knn, double eps = 0.0) { cov_count = n; cov_k = k; cov_reg = reg; cov_eps = eps; vm_valid = false; knn_valid = keep_knn; }
  void covs_supplied() { covs_estimated(-1, -1, false); }  // not from a k-NN search of this library: no lists, no (k, reg) to compare
  void index_built(int chunk) { idx_valid = true; idx_chunk = chunk; }
  void voxelmap_dropped() { vm_valid = false; }
  void voxelmap_built() { vm_valid = true; }
  // the kernel-visible view of the search index (the buffers above own the memory)
  SearchIndex index_view() const { return SearchIndex{idx_sx, idx_sy, idx_sz, idx_orig, idx_s4, idx_tbox, idx_sbox, idx_bbox, idx_n, idx_spad, idx_spad / 32, idx_spad / 512}; }
  CloudView view() const { return CloudView{x, y, z, label, p4, cov6, geo_w, n, n_pad, index_view()}; }
  DevCloud() = default;
  DevCloud(const DevCloud&) = delete;
  DevCloud& operator=(const DevCloud&) = delete;
  // A cloud may be shared by several handles (gorio_apd_set_target_shared) and lives until the last one lets go.  The buffers free
  // themselves as members, AFTER this body: the device has to be current by then.
  ~DevCloud() { hipSetDevice(device); }
};

}  // namespace

struct GicpMpState;  // apd_gicp_mp.hip

struct gorio_apd {
  int device = 0;
  hipStream_t stream = nullptr;
  gorio_apd_params params;
  std::shared_ptr<DevCloud> src, tgt;  // never null; tgt may be shared with other handles of the device
  // per-source-point state: one group of capacity pt_cap (ensure_points)
  DevBuf<unsigned long long> best_key;
  DevBuf<int> seed;        // warm start of the pruned search, by sorted source position (PairDesc::seed)
  DevBuf<unsigned int> nn_work, nn_plan;  // PairDesc::nn_work / nn_plan (measured work of the query waves, plan of the next searches)
  int nn_wcap = 0;
  int align_budget = 0;    // loop iterations the previous batch led by this handle needed (0 = none yet): enqueued before the first look at the done flags
  DevBuf<int> corr;
  DevBuf<float> sqd;
  DevBuf<double> omega6, partials;
  int pt_cap = 0;
  bool corr_valid = false;
  // registration method (gorio_apd_set_method): which fast_gicp class this handle stands for, and the FastVGICP members
  // voxel_resolution_ / search_method_ / voxel_mode_ (fast_vgicp.hpp:79-81)
  int method = GORIO_METHOD_APDGICP;
  double voxel_resolution = 1.0;
  int voxel_search = GORIO_VOXEL_DIRECT1;
  int voxel_mode = GORIO_VOXEL_ADDITIVE;
  // FastVGICP pair state: slot table, weighted Mahalanobis blocks, block partials (VoxPair); corr_valid / omega_valid describe them in that mode
  DevBuf<int> v_slots;       // these three: one group of capacity v_cap
  DevBuf<double> v_omega6, v_partials;
  size_t v_cap = 0;          // slots
  int v_n_off = 0;           // offsets per source point of the slot table held
  DevBuf<VoxPair> d_vox;     // batch array (owned by the handle that leads a batch)
  bool omega_valid = false;  // omega6 holds the Mahalanobis matrices of the last linearisation (not after a Gauss-Newton align)
  // GICP_OMP (GORIO_METHOD_GICP_OMP, apd_gicp_omp.hip): gicp_epsilon_ / max_inner_iterations_ (GOH:117-121), the `output` cloud of GO:402 in
  // original order (x, y, z) and in the source's search-index order, mahalanobis_ as 9 floats per source point, the functor's partials
  double gomp_eps = 0.001;
  int gomp_max_inner = 20;
  DevBuf<float> gomp_out, gomp_maha;  // these five: one group of capacity gomp_cap (source points)
  DevBuf<float4> gomp_s4;
  DevBuf<double> gomp_part;
  DevBuf<int> gomp_cnt;
  int gomp_cap = 0;
  DevBuf<double> gomp_res;            // [16] sums of the last functor evaluation
  DevBuf<unsigned int> gomp_arrive;   // ticket counter of gomp_functor_kernel
  float gomp_guess[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // guess of the `output` cloud held
  int gomp_pairs = -1;                // pairs of the last update (-1: none held)
  int gomp_outer = 0, gomp_inner = 0, gomp_evals = 0, gomp_status = -1;  // gorio_apd_gicp_omp_diag
  int gomp_b_rounds = 0, gomp_b_launches = 0;  // gorio_apd_gicp_omp_batch_diag: of the last batch this handle led
  // ICP (GORIO_METHOD_ICP, apd_icp.hip): use_reciprocal_correspondences_, euclidean_fitness_epsilon_ and transformation_rotation_epsilon_ of
  // pcl::IterativeClosestPoint, the moved working copy in original order (x, y, z) and in the source's search-index order, the reciprocal flags
  int icp_reciprocal = 0;
  double icp_fit_eps = -DBL_MAX, icp_rot_eps = 0.0;
  DevBuf<float> icp_w;                // these three: one group of capacity icp_cap (source points)
  DevBuf<float4> icp_s4;
  DevBuf<int> icp_rflag;
  int icp_cap = 0;
  int icp_iterations = 0, icp_state = 0, icp_pairs = -1, icp_passes = 0;  // gorio_apd_icp_diag
  double icp_mse = 0.0;
  int icp_b_rounds = 0, icp_b_launches = 0;  // gorio_apd_icp_batch_diag: of the last batch this handle led
  // fast_gicp::NDTCuda (GORIO_METHOD_NDT_CUDA, apd_ndt_cuda.hip): distance_mode and the DIRECT_RADIUS radius (ndt_cuda.cu:21-35), the offset
  // table on the device and the (search, radius) it was made for, the slot table, linearized_x and the block partials
  int ndtc_mode = GORIO_NDT_CUDA_D2D;
  double ndtc_radius = -1.0;
  DevBuf<int> ndtc_off;
  int ndtc_n_off = 0, ndtc_off_search = -1;
  double ndtc_off_radius = 0.0;
  std::vector<int> ndtc_off_host;
  DevBuf<int> ndtc_slots;      // these two: one group of capacity ndtc_cap (slots)
  DevBuf<double> ndtc_partials;
  size_t ndtc_cap = 0;
  DevBuf<float> ndtc_tlin;     // [12]
  int ndtc_items = 0, ndtc_slot_off = 0, ndtc_slot_d2d = 0;  // shape of the slot table held (items, offsets, distance mode)
  DevBuf<NdtcPair> d_ndtc;     // batch array (owned by the handle that leads a batch)
  // fast_gicp::FastVGICPCuda (GORIO_METHOD_VGICP_CUDA, apd_vgicp_cuda.hip): neighbor_method_, kernel_width_, kernel_max_dist_ (VI:27-31).  Its
  // offset table, slot table, linearized_x and partials are the NDTCuda members above (ndtc_slot_d2d == 2).
  int vgc_nn = GORIO_VGICP_CUDA_NN_CPU_PARALLEL_KDTREE;
  double vgc_width = 0.5, vgc_maxd = 3.0;
  // fast_gicp::FastGICPMultiPoints (GORIO_METHOD_GICP_MP, apd_gicp_mp.hip): neighbor_search_radius_ (MPI:35), the per-pass state (the radius
  // search's buffers and CSR, the transformed source, the merged distributions, the partials) and whether it holds a pass
  double mp_radius = 0.5;
  std::shared_ptr<GicpMpState> mp;
  bool mp_pass_valid = false;
  DevBuf<PairState> d_state;
  DevBuf<PairDesc> d_desc;   // batch descriptor array and states (owned by the handle that leads a batch): one group of capacity desc_cap
  DevBuf<PairState> d_states_batch;
  int desc_cap = 0;
  DevBuf<KnnJob> d_jobs;
  DevBuf<unsigned int> d_redo_list;  // run_covariances: [0] count, then (job, group) of the 64-position groups knn_collect_kernel gave up on
  DevBuf<void> d_copy_jobs;  // gorio_apd_set_clouds_device_batch
  DevBuf<IndexJob> d_ijobs;
  DevBuf<double> d_fit;      // block partials of a fitness score
  // scan-to-submap assembly scratch (gorio_apd_set_target_submap)
  DevBuf<float4> d_sub_in, d_sub_out, d_sub_vox;  // one group of capacity sub_cap
  size_t sub_cap = 0;
  DevBuf<unsigned long long> d_sub_keys;
  DevBuf<int> d_sub_counts;
  DevBuf<SubmapFrame> d_sub_frames;
  DevBuf<unsigned int> d_sub_bb;
  DevBuf<void> d_sub_kframes;  // gorio_apd_set_target_submap_keyframes (apd_keyframes.hip): frame table, and the finite points per 256-point block
  DevBuf<int> d_sub_kcnt;
  int sub_downsample = GORIO_DOWNSAMPLE_VOXELGRID;  // gorio_apd_set_submap_downsample: what a voxel_leaf > 0 runs (SMO:140-154)
  AvgScratch avg;  // pcl::ApproximateVoxelGrid (apd_approx_voxel.hip): the submap mode above and gorio_prep_approx_voxel_downsample
  // sharded-source mode (gorio_apd_comm_init): RCCL communicator over the ranks that share one source cloud
  ncclComm_t comm = nullptr;
  int comm_world = 1, comm_rank = 0;
  bool shard_only = false;  // gorio_apd_debug_set_shard: the source partition of a rank without the collectives (test hook)
  bool fuse_supported = false;  // gorio_apd_create: the device is one the fence-free hand-over of the fused step was validated on
  bool fuse_step = true, plan_search = true;  // gorio_apd_debug_set_schedule
  DevBuf<double> d_red;     // [32] all-reduce buffer: 28 sums of a linearisation, [28] trial error, [29] scratch
  long long allreduce_count = 0;  // ncclAllReduce calls enqueued through this handle's communicator (gorio_apd_comm_info)
  // pinned host staging of the small descriptor arrays a call uploads (index jobs, k-NN jobs, pair descriptors / states, copy jobs): a
  // copy from pageable memory needs a stream drain before the vector it came from may die; a pinned buffer of the handle's own needs none
  struct Pinned {
    PinnedBuf buf;
    hipEvent_t ev = nullptr;  // recorded behind the last upload from this buffer: the next writer waits for it
    bool pending = false;
    ~Pinned() {
      if (ev) hipEventDestroy(ev);
    }
  };
  Pinned pin_ijobs, pin_jobs, pin_desc, pin_states, pin_copy, pin_vox, pin_ndtc;
  // The lock-step batched aligns (run_rounds, apd_batch_rounds.hip), used by the handle that leads the rounds: job records and round table,
  // block partials and block counts, the jobs' folded sums on the device and pinned on the host, the staging of the table.  One set for
  // all methods: a handle leads one batch at a time and every call reserves what it needs; pin's event guards the staging's reuse.
  struct RoundScratch {
    DevBuf<unsigned char> tab;
    DevBuf<double> part;
    DevBuf<int> cnt;
    DevBuf<void> out;  // sums (and counts) of the jobs, h_out the same on the host
    PinnedBuf h_out;
    Pinned pin;
  };
  RoundScratch round;
  PinnedBuf pin_looks;  // where the align loop's looks at the pair states land (a download into pageable memory is staged by the runtime)
  std::string err;
  // profiling
  bool profiling = false;
  double stage_s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int stage_n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  struct EvPair { hipEvent_t start, stop; int stage; int prev; };  // prev >= 0: the span starts at ev_pool[prev].stop (StageChain)
  std::vector<EvPair> ev_pool;
  size_t ev_used = 0;
  // gorio_apd_set_method: correspondences, Mahalanobis matrices, pair counts and passes of another method (or another neighbourhood) mean
  // nothing to the new one
  void method_switched() { corr_valid = false; omega_valid = false; gomp_pairs = -1; icp_pairs = -1; mp_pass_valid = false; }
  // gorio_apd_destroy makes the device current and drains the stream first; the buffers then free themselves as members
  ~gorio_apd() {
    for (auto& e : ev_pool) { hipEventDestroy(e.start); hipEventDestroy(e.stop); }
  }
};

namespace {

// All handles of one device share ONE launch stream: setInput* copies, index builds and align batches of different handles are
// then ordered by the stream itself and a batch needs no cross-stream synchronisation.  (UGPM uses its own stream and overlaps.)
hipStream_t device_stream(int device) {
  static std::mutex mu;
  static std::vector<hipStream_t> streams;
  std::lock_guard<std::mutex> lock(mu);
  if ((int)streams.size() <= device) streams.resize(device + 1, nullptr);
  if (!streams[device]) {
    if (hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking) != hipSuccess) return nullptr;
  }
  return streams[device];
}

int fail(gorio_apd* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

struct HandleFail {  // fail() bound to a handle, for GORIO_HIP_CHECK
  gorio_apd* h;
  int operator()(int code, const std::string& msg) const { return fail(h, code, msg); }
};
#define HIP_TRY(h, expr) GORIO_HIP_CHECK(HandleFail{h}, expr)

int roundup(int v, int m) { return (v + m - 1) / m * m; }

// GICP_OMP (apd_gicp_omp.hip, included at the end of this file)
constexpr int kRegGicpOmp = 100;  // DevCloud::cov_reg of covariances estimated by the rule of GO:50-122: one more "regularization" for sharing
constexpr int kRegMpBase = 200;   // DevCloud::mp_reg = kRegMpBase + regularization: the covariance rule of FastGICPMultiPoints is one more "regularization" for sharing
int gomp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize);
int gomp_covariances(gorio_apd* lead, std::vector<std::pair<gorio_apd*, DevCloud*>>& todo);
// ICP (apd_icp.hip, included at the end of this file)
int icp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize);
// FastGICPMultiPoints (apd_gicp_mp.hip, included at the end of this file)
int mp_align(gorio_apd* h, const float* guess, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize);
bool is_mp(const gorio_apd* h) { return h->method == GORIO_METHOD_GICP_MP; }
// the rule a handle estimates covariances by, and whether covariances estimated with (k, reg, eps) are the ones it would estimate
int cov_rule(const gorio_apd* h) { return h->method == GORIO_METHOD_GICP_OMP ? kRegGicpOmp : h->params.regularization; }
bool cov_rule_differs(const gorio_apd* h, const DevCloud& c) {
  return c.cov_count == c.n && c.cov_k >= 0 && (c.cov_k != h->params.k_correspondences || c.cov_reg != cov_rule(h) || (c.cov_reg == kRegGicpOmp && c.cov_eps != h->gomp_eps));
}

// Upload `bytes` of a short-lived host array through the handle's pinned staging buffer `b`: no stream drain, the caller's array may die
// right away.  A buffer that still feeds an earlier upload is waited for first (its event), never overwritten under it.
int upload_staged(gorio_apd* h, gorio_apd::Pinned& b, void* dst, const void* src, size_t bytes) {
  if (b.pending) {
    HIP_TRY(h, hipEventSynchronize(b.ev));
    b.pending = false;
  }
  HIP_TRY(h, b.buf.reserve(bytes, bytes + bytes / 2 + 256));
  if (!b.ev) HIP_TRY(h, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
  std::memcpy(b.buf, src, bytes);
  HIP_TRY(h, hipMemcpyAsync(dst, b.buf, bytes, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipEventRecord(b.ev, h->stream));
  b.pending = true;
  return GORIO_OK;
}

// RCCL is loaded on first use (dlopen): a process that never shards a source never needs librccl, and one that already has a copy
// mapped (PyTorch ships its own) keeps using that copy.
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;
};
Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (!r.lib) return;
    r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
    r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
    r.CommCount = reinterpret_cast<decltype(r.CommCount)>(dlsym(r.lib, "ncclCommCount"));
    r.CommUserRank = reinterpret_cast<decltype(r.CommUserRank)>(dlsym(r.lib, "ncclCommUserRank"));
    r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
    r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllReduce && r.GetErrorString;
  });
  return r;
}

#define NCCL_TRY(h, expr)                                                                                              \
  do {                                                                                                                 \
    ncclResult_t e_ = (expr);                                                                                          \
    if (e_ != ncclSuccess) return fail(h, GORIO_ERR_NO_DEVICE, std::string(#expr) + ": " + rccl().GetErrorString(e_)); \
  } while (0)


// a cloud about to be overwritten must not be one other handles still look at (gorio_apd_set_target_shared): detach first
void make_private(gorio_apd* h, std::shared_ptr<DevCloud>& c) {
  if (c.use_count() > 1) {
    c = std::make_shared<DevCloud>();
    c->device = h->device;
  }
}

int ensure_cloud(gorio_apd* h, DevCloud& c, int n) {
  const int n_pad = roundup(n, kPad) + kPad;
  if (n_pad > c.cap) {
    c.knn.reset();  // sized by cap * k: reallocated by the next covariance computation that keeps the lists
    c.knn_k = 0;
    const size_t cap = n_pad + n_pad / 8;
    HIP_TRY(h, reserve_group(c.cap, n_pad, cap, c.x, cap, c.y, cap, c.z, cap, c.label, cap, c.p4, cap, c.cov6, 6 * cap, c.geo_w, cap));
  }
  c.n = n;
  c.n_pad = n_pad;
  return GORIO_OK;
}

int ensure_points(gorio_apd* h, int n) {
  if (n > h->pt_cap) {
    const size_t cap = n + n / 8 + 256;
    const size_t wcap = (cap + 512) / 64 + 1;
    HIP_TRY(h, reserve_group(h->pt_cap, n, cap, h->best_key, cap, h->seed, cap + 512 /* indexed by sorted position < roundup(n, 512) */, h->nn_work, 2 * wcap,
                             h->nn_plan, 1 + 16 * wcap, h->corr, cap, h->sqd, cap, h->omega6, 6 * cap, h->partials, 28 * (cap / 256 + 2)));
    h->nn_wcap = (int)wcap;
    HIP_TRY(h, hipMemsetAsync(h->nn_work, 0, sizeof(unsigned int) * 2 * wcap, h->stream));
    HIP_TRY(h, hipMemsetAsync(h->nn_plan, 0, sizeof(unsigned int) * (1 + 16 * wcap), h->stream));
  }
  return GORIO_OK;
}

// host strided AoS -> device SoA (+ padding)
int upload_cloud(gorio_apd* h, DevCloud& c, const float* xyz, const float* label, int n, int stride_bytes) {
  if (!xyz || n <= 0 || stride_bytes < 12 || (stride_bytes % 4) != 0) return fail(h, GORIO_ERR_INVALID, "set_input: bad cloud arguments");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = ensure_cloud(h, c, n);
  if (rc) return rc;
  const int np = c.n_pad;
  std::vector<float> buf((size_t)np * 8);
  float *bx = buf.data(), *by = bx + np, *bz = by + np, *bl = bz + np, *b4 = bl + np;
  const int st = stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + (size_t)i * st;
    bx[i] = p[0]; by[i] = p[1]; bz[i] = p[2];
    bl[i] = label ? label[(size_t)i * st] : 0.0f;
  }
  for (int i = n; i < np; ++i) { bx[i] = kFar; by[i] = kFar; bz[i] = kFar; bl[i] = 0.0f; }
  for (int i = 0; i < np; ++i) { b4[4 * (size_t)i] = bx[i]; b4[4 * (size_t)i + 1] = by[i]; b4[4 * (size_t)i + 2] = bz[i]; b4[4 * (size_t)i + 3] = bl[i]; }
  HIP_TRY(h, hipMemcpyAsync(c.x, bx, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c.y, by, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c.z, bz, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c.label, bl, sizeof(float) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c.p4, b4, sizeof(float4) * np, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  c.points_replaced();
  return GORIO_OK;
}

// setInput* from device-resident SoA buffers: one launch copies the four arrays and writes the padding
__global__ __launch_bounds__(256) void copy_cloud_kernel(const float* __restrict__ sx, const float* __restrict__ sy, const float* __restrict__ sz, const float* __restrict__ sl,
                                                         float* __restrict__ x, float* __restrict__ y, float* __restrict__ z, float* __restrict__ label, float4* __restrict__ p4, int n, int n_pad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_pad) return;
  const bool in = i < n;
  const float4 v = make_float4(in ? sx[i] : 1e30f, in ? sy[i] : 1e30f, in ? sz[i] : 1e30f, (in && sl) ? sl[i] : 0.0f);
  x[i] = v.x;
  y[i] = v.y;
  z[i] = v.z;
  label[i] = v.w;
  p4[i] = v;
}

int upload_cloud_device(gorio_apd* h, DevCloud& c, const float* dx, const float* dy, const float* dz, const float* dl, int n) {
  if (!dx || !dy || !dz || n <= 0) return fail(h, GORIO_ERR_INVALID, "set_input_device: bad cloud arguments");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = ensure_cloud(h, c, n);
  if (rc) return rc;
  copy_cloud_kernel<<<(c.n_pad + 255) / 256, 256, 0, h->stream>>>(dx, dy, dz, dl, c.x, c.y, c.z, c.label, c.p4, n, c.n_pad);
  HIP_TRY(h, hipGetLastError());
  c.points_replaced();
  return GORIO_OK;
}

// the same for many clouds in ONE launch (grid.y = cloud): a step of the batched pipeline re-targets 2 x pairs clouds, and 128
// five-microsecond launches in a row are 0.7 ms of stream time
struct CopyJob {
  const float* sx; const float* sy; const float* sz; const float* sl;
  float* x; float* y; float* z; float* label;
  float4* p4;
  int n, n_pad;
};
__global__ __launch_bounds__(256) void copy_clouds_kernel(const CopyJob* __restrict__ jobs) {
  const CopyJob jb = jobs[blockIdx.y];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < jb.n_pad; i += gridDim.x * 256) {
    const bool in = i < jb.n;
    const float4 v = make_float4(in ? jb.sx[i] : 1e30f, in ? jb.sy[i] : 1e30f, in ? jb.sz[i] : 1e30f, (in && jb.sl) ? jb.sl[i] : 0.0f);
    jb.x[i] = v.x;
    jb.y[i] = v.y;
    jb.z[i] = v.z;
    jb.label[i] = v.w;
    jb.p4[i] = v;
  }
}

ApdConsts make_consts(const gorio_apd_params& p) {  // inv_n_scale is patched per launch set by cl_scale()
  ApdConsts c;
  c.thr2 = p.corr_dist_threshold * p.corr_dist_threshold;
  c.dist_var = p.dist_var;
  c.sin_az = std::sin(p.azimuth_var / 180 * M_PI);
  c.sin_el = std::sin(p.elevation_var / 180 * M_PI);
  c.rot_eps = p.rotation_epsilon;
  c.trans_eps = p.transformation_epsilon;
  c.lm_init_lambda_factor = p.lm_init_lambda_factor;
  c.inv_n_scale = 1.0;
  c.optimizer = p.optimizer;
  c.lm_max_iterations = p.lm_max_iterations;
  c.max_iterations = p.max_iterations;
  c.pad_ = 0;
  return c;
}

// Stage timing with HIP events on the launch stream.  Events are only RECORDED while kernels are being enqueued (no host
// synchronisation inside the loop); resolve_stage_events() turns them into seconds after the stream has drained.
struct StageTimer {
  gorio_apd* h;
  bool on;
  size_t slot;
  StageTimer(gorio_apd* h_, int s) : h(h_), on(h_->profiling), slot(0) {
    if (!on) return;
    if (h->ev_used == h->ev_pool.size()) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
      h->ev_pool.push_back({a, b, s, -1});
    }
    slot = h->ev_used++;
    h->ev_pool[slot].stage = s;
    h->ev_pool[slot].prev = -1;
    hipEventRecord(h->ev_pool[slot].start, h->stream);
  }
  ~StageTimer() {
    if (on) hipEventRecord(h->ev_pool[slot].stop, h->stream);
  }
};

// Back-to-back kernels of the optimiser loop: ONE event between two kernels closes the span of the first and opens the span of the
// second (two records per kernel cost the loop about 10 % in launch gaps).  A span then includes the launch gap before its kernel.
struct StageChain {
  gorio_apd* h;
  bool on;
  int last = -1;
  int take(int stage) {
    if (h->ev_used == h->ev_pool.size()) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return -1; }
      h->ev_pool.push_back({a, b, stage, -1});
    }
    const int q = (int)h->ev_used++;
    h->ev_pool[q].stage = stage;
    h->ev_pool[q].prev = -1;
    return q;
  }
  explicit StageChain(gorio_apd* h_) : h(h_), on(h_->profiling) {
    if (!on) return;
    last = take(-1);  // boundary only, no span
    if (on) hipEventRecord(h->ev_pool[last].stop, h->stream);
  }
  void mark(int stage) {  // call right after the launch(es) of `stage`
    if (!on) return;
    const int q = take(stage);
    if (!on) return;
    h->ev_pool[q].prev = last;
    hipEventRecord(h->ev_pool[q].stop, h->stream);
    last = q;
  }
};

void resolve_stage_events(gorio_apd* h) {
  if (!h->profiling) return;
  for (size_t q = 0; q < h->ev_used; ++q) {
    float ms = 0.f;
    if (h->ev_pool[q].stage < 0) continue;
    const hipEvent_t from = h->ev_pool[q].prev >= 0 ? h->ev_pool[h->ev_pool[q].prev].stop : h->ev_pool[q].start;
    if (hipEventSynchronize(h->ev_pool[q].stop) == hipSuccess && hipEventElapsedTime(&ms, from, h->ev_pool[q].stop) == hipSuccess) {
      h->stage_s[h->ev_pool[q].stage] += ms * 1e-3;
      h->stage_n[h->ev_pool[q].stage] += 1;
    }
  }
  h->ev_used = 0;
}

// Build the search accelerator of every listed cloud that lacks one (batched: every launch covers all clouds).  The launches, in order:
//   bbox_morton_sort_kernel                   clouds of at most kLdsSortMax points: bounding box, Morton keys and their sort in one launch
//   for the bigger clouds of the call, each routed by its own size (the jobs are ordered small first, the launches take their part):
//     bbox_morton_kernel                      bounding box + Morton keys (bbox_init / bbox / morton_kernel when a cloud exceeds kBboxFusedMax)
//     enqueue_tiled_sort                      bitonic_tile_sort_kernel, then per merge size above the sort tile bitonic_global_kernel per stride +
//                                             bitonic_tile_merge_kernel (apd_index.hip; the voxel-map and submap sorts enqueue the same)
//   kd_refine_kernel                          gather in Morton order, median splits, sx / sy / sz / orig / s4, tile and super-tile boxes
//   box_block_kernel                          block boxes
// 3 launches for 16 384-point scans (9 while their sort went through global memory between its stages).
thread_local int g_index_build_launches = 0;  // kernel launches of this thread's last run_index_build (the scan batch's diagnostics add them up)
int run_index_build(gorio_apd* lead, std::vector<std::pair<gorio_apd*, DevCloud*>>& clouds) {
  g_index_build_launches = 0;
  std::vector<std::pair<gorio_apd*, DevCloud*>> todo;
  bool small_call = true;  // every cloud named in the call (built now or not) is a scan-sized one: kd chunks of 2048 points (kd_refine_kernel)
  {
    std::unordered_set<DevCloud*> seen;
    for (auto& c : clouds) {
      if (c.second->n > kKdSmallCloud) small_call = false;
      if (!c.second->idx_valid && seen.insert(c.second).second) todo.push_back(c);
    }
  }
  if (todo.empty()) return GORIO_OK;
  const int nj = (int)todo.size();
  // clouds whose keys one workgroup sorts in LDS come first in the job list, the others behind them
  const int ns = (int)(std::stable_partition(todo.begin(), todo.end(), [](const std::pair<gorio_apd*, DevCloud*>& c) { return c.second->n <= kLdsSortMax; }) - todo.begin());
  std::vector<IndexJob> jobs(nj);
  int max_pow2 = kSortTile, max_spad = 512, max_n = 1;  // max_pow2 / max_n: over the clouds that take the tiled sort
  for (int q = 0; q < nj; ++q) {
    gorio_apd* h = todo[q].first;
    DevCloud& c = *todo[q].second;
    const int n_spad = roundup(c.n, 512);
    const int npow2 = sort_padded_size(c.n);
    const size_t cap = n_spad + roundup(n_spad / 8, 512);
    HIP_TRY(h, reserve_group(c.idx_cap, n_spad, cap, c.idx_sx, cap, c.idx_sy, cap, c.idx_sz, cap, c.idx_orig, cap, c.idx_s4, cap, c.idx_tbox, 8 * (cap / 32),
                             c.idx_sbox, 8 * (cap / 512), c.idx_bbox, 8 * (cap / 32768 + 1)));
    HIP_TRY(h, c.keys.reserve(npow2));
    HIP_TRY(h, c.bb.reserve(6));
    c.idx_n = c.n;
    c.idx_spad = n_spad;
    IndexJob& j = jobs[q];
    j.x = c.x; j.y = c.y; j.z = c.z; j.n = c.n; j.npow2 = npow2; j.keys = c.keys; j.bb = c.bb; j.idx = c.index_view();
    max_spad = std::max(max_spad, n_spad);
    if (q >= ns) {
      max_pow2 = std::max(max_pow2, npow2);
      max_n = std::max(max_n, c.n);
    }
  }
  HIP_TRY(lead, lead->d_ijobs.reserve(nj));
  if (int rc = upload_staged(lead, lead->pin_ijobs, lead->d_ijobs, jobs.data(), sizeof(IndexJob) * nj)) return rc;
  {
    StageTimer t(lead, 4);
    const IndexJob* dj = lead->d_ijobs;
    if (ns > 0) bbox_morton_sort_kernel<<<ns, 1024, 0, lead->stream>>>(dj);
    if (nj > ns) {
      const IndexJob* bj = dj + ns;
      const int nb = nj - ns;
      if (max_n <= kBboxFusedMax) {
        bbox_morton_kernel<<<nb, 1024, 0, lead->stream>>>(bj);
      } else {
        bbox_init_kernel<<<(nb + 63) / 64, 64, 0, lead->stream>>>(bj, nb);
        bbox_kernel<<<dim3(std::min(64, (max_n + 255) / 256), nb), 256, 0, lead->stream>>>(bj);
        morton_kernel<<<dim3((max_pow2 + 255) / 256, nb), 256, 0, lead->stream>>>(bj);
      }
      enqueue_tiled_sort(lead->stream, IndexJobKeys{bj}, nb, max_pow2);
    }
    if (small_call) kd_refine_kernel<2048><<<dim3((max_spad + 2047) / 2048, nj), 512, 0, lead->stream>>>(dj);
    else kd_refine_kernel<4096><<<dim3((max_spad + 4095) / 4096, nj), 1024, 0, lead->stream>>>(dj);
    box_block_kernel<<<dim3((max_spad / 32768 + 64) / 64, nj), 64, 0, lead->stream>>>(dj);
  }
  HIP_TRY(lead, hipGetLastError());
  g_index_build_launches = (ns > 0 ? 1 : 0) + 2;
  if (nj > ns) {
    g_index_build_launches += (max_n <= kBboxFusedMax ? 1 : 3) + 1;
    for (int k = 2 * kSortTile; k <= max_pow2; k <<= 1) {
      for (int j = k >> 1; j >= kSortTile; j >>= 1) ++g_index_build_launches;
      ++g_index_build_launches;
    }
  }
  for (auto& t : todo) t.second->index_built(small_call ? 2048 : 4096);
  return GORIO_OK;
}

// run_covariances for its k-NN lists alone (FastVGICPCuda's float covariances are made from them, apd_vgicp_cuda.hip): the lists go to
// knn_out, the double covariances and weights the kernels make on the way go to scratch, and the clouds' own covariances, lists and state
// stay as they are
struct KnnListsOnly {
  int* knn_out;    // [n][k]
  double* cov6;    // [n][6] scratch
  double* geo_w;   // [n] scratch
};

// covariance estimation for a list of clouds on lead's stream
int run_covariances(gorio_apd* lead, std::vector<std::pair<gorio_apd*, DevCloud*>>& todo, const KnnListsOnly* only = nullptr) {
  if (todo.empty()) return GORIO_OK;
  const int njobs = (int)todo.size();
  const int k = lead->params.k_correspondences;
  const int K = k <= 20 ? 20 : 32;
  const bool pruned = lead->params.search == GORIO_SEARCH_PRUNED;
  const bool select = pruned && K == 20;  // knn_kth_kernel + knn_collect_kernel (LDS buffer sized for K = 20); K = 32 keeps the insertion kernel
  if (pruned) {
    int rc = run_index_build(lead, todo);
    if (rc) return rc;
  }
  long total_waves = 0;
  int max_n = 0;
  for (auto& t : todo) {
    total_waves += (t.second->n + 63) / 64;
    if (t.second->n > max_n) max_n = t.second->n;
  }
  int splits = (int)((8192 + total_waves - 1) / total_waves);
  if (splits < 1) splits = 1;
  if (splits > 32) splits = 32;
  if (pruned) splits = 1;
  std::vector<KnnJob> jobs(njobs);
  int max_splits = 1;
  for (int q = 0; q < njobs; ++q) {
    gorio_apd* h = todo[q].first;
    DevCloud& c = *todo[q].second;
    int chunk = roundup((c.n_pad + splits - 1) / splits, kPad);
    if (chunk < 256) chunk = 256;
    const int s = pruned ? 1 : (c.n_pad + chunk - 1) / chunk;
    if (s > max_splits) max_splits = s;
    const size_t need = pruned ? 0 : (size_t)s * K * c.n;
    HIP_TRY(h, reserve_group(c.part_cap, need, need, c.part_d, need, c.part_i, need));
    const bool keep = h->params.keep_knn_indices != 0 || lead->method == GORIO_METHOD_GICP_OMP;  // GICP_OMP estimates from the lists
    if (!only && keep && (c.knn_k != k || !c.knn)) {
      c.knn_k = 0;
      HIP_TRY(h, c.knn.realloc((size_t)c.cap * k));
      c.knn_k = k;
    }
    if (select) {
      const size_t nw = roundup(c.n, 512) / 64, cap = nw + nw / 8;
      HIP_TRY(h, reserve_group(c.redo_cap, nw, cap, c.redo, cap, c.kth, 64 * cap));
    }
    KnnJob& j = jobs[q];
    j.cloud = c.view();
    if (only) {
      j.cloud.cov6 = only->cov6;
      j.cloud.geo_w = only->geo_w;
    }
    j.part_d = c.part_d;
    j.part_i = c.part_i;
    j.knn_out = only ? only->knn_out : keep ? c.knn.get() : nullptr;
    j.redo = select ? c.redo.get() : nullptr;
    j.kth = select ? c.kth.get() : nullptr;
    j.k = k;
    j.regularization = h->params.regularization;
    j.splits = s;
    j.chunk_len = chunk;
    j.qpw = 64;
    j.pad0_ = 0;
  }
  // queries per wave of the selection kernels: halved while the call has fewer waves than the chip has SIMDs (1024)
  int qpw = 64;
  {
    long w64 = 0;
    for (int q = 0; q < njobs; ++q) w64 += (jobs[q].cloud.idx.n + 63) / 64;
    while (qpw > 8 && w64 * (64 / qpw) < 1024) qpw /= 2;
    if (const char* e = std::getenv("GORIO_KNN_QPW")) {  // experiments (profiles/r03/experiments.md)
      const int v = std::atoi(e);
      if (v == 8 || v == 16 || v == 32 || v == 64) qpw = v;
    }
    for (int q = 0; q < njobs; ++q) jobs[q].qpw = qpw;
  }
  HIP_TRY(lead, lead->d_jobs.reserve(njobs));
  if (int rc = upload_staged(lead, lead->pin_jobs, lead->d_jobs, jobs.data(), sizeof(KnnJob) * njobs)) return rc;
  if (select) {  // the call's redo list: room for every 64-position group that has a query
    size_t groups = 0;
    for (auto& t : todo) groups += ((size_t)t.second->n + 63) / 64;
    HIP_TRY(lead, lead->d_redo_list.reserve(2 + 2 * groups, 2 + 2 * (groups + groups / 8)));
  }
  {
    StageTimer t(lead, 0);
    dim3 g1((max_n + 255) / 256, max_splits, njobs), g2((max_n + 255) / 256, 1, njobs);
    dim3 gp((roundup(max_n, 512) + 255) / 256, 1, njobs);
    if (K == 20) {
      if (pruned) {
        const dim3 gs(gp.x * (256 / qpw), 1, njobs);
        HIP_TRY(lead, hipMemsetAsync(lead->d_redo_list, 0, sizeof(unsigned int), lead->stream));
        knn_kth_kernel<20><<<gs, kKnnBlock, 0, lead->stream>>>(lead->d_jobs);
        knn_collect_kernel<20><<<gs, kKnnBlock, 0, lead->stream>>>(lead->d_jobs, lead->d_redo_list);
        knn_redo_kernel<20><<<kKnnRedoBlocks, 256, 0, lead->stream>>>(lead->d_jobs, lead->d_redo_list);  // the groups knn_collect_kernel listed (massive ties)
      } else {
        knn_partial_kernel<20><<<g1, 256, 0, lead->stream>>>(lead->d_jobs);
        cov_finalize_kernel<20><<<g2, 256, 0, lead->stream>>>(lead->d_jobs);
      }
    } else {
      if (pruned) knn_pruned_kernel<32><<<gp, 256, 0, lead->stream>>>(lead->d_jobs);
      else {
        knn_partial_kernel<32><<<g1, 256, 0, lead->stream>>>(lead->d_jobs);
        cov_finalize_kernel<32><<<g2, 256, 0, lead->stream>>>(lead->d_jobs);
      }
    }
  }
  HIP_TRY(lead, hipGetLastError());
  if (only) return GORIO_OK;
  if (lead->method == GORIO_METHOD_GICP_OMP) {
    if (int rc = gomp_covariances(lead, todo)) return rc;
    for (auto& t : todo) t.second->covs_estimated(k, kRegGicpOmp, true, lead->gomp_eps);
    return GORIO_OK;
  }
  for (auto& t : todo) t.second->covs_estimated(k, lead->params.regularization, t.first->params.keep_knn_indices != 0);
  return GORIO_OK;
}

// largest float f with (double)f < thr2: candidates beyond it can never pass the gate of APD:183.  inclusive: with (double)f <= thr2, for
// the gate of pcl::CorrespondenceEstimation (a pair is dropped when its distance is GREATER than the threshold)
float gate_bound(double thr2, bool inclusive = false) {
  if (!(thr2 < (double)FLT_MAX)) return FLT_MAX;
  float f = (float)thr2;
  while (!(inclusive ? (double)f <= thr2 : (double)f < thr2)) f = std::nextafterf(f, 0.0f);
  return f;
}

// mode: bit 0 = which half of nn_work this launch accumulates into, bit 1 = take the work list of nn_plan_kernel instead of the grid position
void launch_pruned(dim3 grid, hipStream_t stream, const PairDesc* d_desc, float bound, int mode) {
  nn_search_pruned_kernel<<<dim3(grid.x * (256 / kNnBlock), grid.y, grid.z), kNnBlock, 0, stream>>>(d_desc, bound, mode);
}

// launch_index: position of this search inside its align (0 = the unseeded one), or -1 for a search outside an align loop.  From the third
// search of an align on, the work measured in the second one (the first seeded one) decides which query waves are cut into parts and
// which run first (nn_plan_kernel); the first two use the grid position, with the groups of every wave dealt over `splits` workgroups.
void launch_nn(gorio_apd* lead, const PairDesc* d_desc, dim3 g_nn, int max_src_spad, int count, int max_tgt_n, int launch_index = -1, bool inclusive_gate = false) {
  if (lead->params.search == GORIO_SEARCH_PRUNED) {
    const double thr = lead->params.corr_dist_threshold;
    const long waves = (long)count * ((max_src_spad + 63) / 64);
    const bool no_plan = !lead->plan_search;  // gorio_apd_debug_set_schedule
    const bool planned = launch_index >= 2 && !lead->comm && !lead->shard_only && !no_plan;
    // entries of the work list == workgroups of a planned launch: twice the query waves for a batch that fills the chip anyway, more for
    // a few pairs (a lone 16k scan has 256 query waves: 16 parts each are 4096 workgroups), never more than 16 parts per wave
    const int nw_max = (max_src_spad + 63) / 64;
    // part budget = all work / plan_div (10240 = two parts per wave slot of the chip) and at most capmul parts per query wave on average.
    // Finer cutting pays only where the work has a heavy tail -- the far returns of a scan against a big, dense map: measured on 64 scans
    // x 1 M-point map 11.5 -> 10.3 ms per 20 searches with (4, 20480), on 64 pairs of 16 k points 2.01 -> 2.14 ms.
    const bool big = max_tgt_n >= 131072;
    const int capmul = big ? 4 : 2, plan_div = big ? 20480 : 10240;
    const int plan_cap = std::min(16 * nw_max, std::max(capmul * nw_max, 8192 / std::max(1, count)));
    if (planned) {
      launch_pruned(dim3((plan_cap + 3) / 4, 1, count), lead->stream, d_desc, gate_bound(thr * thr, inclusive_gate), 2 | (launch_index & 1));
      return;
    }
    int splits = (int)(4096 / (waves > 0 ? waves : 1));  // a lone 16k scan has 256 query waves: deal the tile groups over more workgroups
    if (splits < 1) splits = 1;
    if (splits > 16) splits = 16;
    // A big, dense target has query waves that need hundreds of tiles (a far radar return whose nearest map point is a metre away
    // sits in a ball full of map points) next to waves that need two: dealing the tile groups of every wave over several workgroups
    // shortens that tail until the plan takes over.
    if (max_tgt_n >= 131072 && splits < 8) splits = 8;
    while (splits & (splits - 1)) splits &= splits - 1;  // the kernel deals groups by their low bits: a power of two
    launch_pruned(dim3((max_src_spad + 255) / 256, splits, count), lead->stream, d_desc, gate_bound(thr * thr, inclusive_gate), launch_index >= 0 ? (launch_index & 1) : 0);
    if (launch_index == 1 && !lead->comm && !lead->shard_only && !no_plan) nn_plan_kernel<<<count, 256, 0, lead->stream>>>(d_desc, 1, count, plan_cap, plan_div);
  } else {
    nn_search_kernel<<<g_nn, 256, 0, lead->stream>>>(d_desc);
  }
}

// a target shared with other handles carries ONE set of covariances: a sharer whose k_correspondences / regularization differ from the ones
// they were estimated with would silently register with another object's covariances (the reference estimates them per object, APD:149-154)
bool shared_cov_mismatch(const gorio_apd* h) {
  const DevCloud& t = *h->tgt;
  return h->tgt.use_count() > 1 && cov_rule_differs(h, t);
}

// the same for a source that other handles hold too (a scan output handed over by gorio_apd_set_source_from_scan, include/gorio_scan.h)
bool shared_source_cov_mismatch(const gorio_apd* h) {
  const DevCloud& s = *h->src;
  return h->src.use_count() > 1 && cov_rule_differs(h, s);
}

// ---- FastVGICP plumbing

int voxel_offsets(int search) { return search == GORIO_VOXEL_DIRECT1 ? 1 : search == GORIO_VOXEL_DIRECT7 ? 7 : 27; }  // neighbor_offsets, VOX:16-43

// sharers of a target share ONE voxel map: a sharer whose resolution / accumulation differ from the ones it was built with would register
// against another object's map (or rebuild it under the other sharers)
bool shared_voxel_mismatch(const gorio_apd* h) {
  const DevCloud& t = *h->tgt;
  return h->method == GORIO_METHOD_VGICP && h->tgt.use_count() > 1 && t.vm_valid &&
         (t.vm.res != h->voxel_resolution || t.vm_mult != (h->voxel_mode == GORIO_VOXEL_MULTIPLICATIVE));
}

// The first half of every map build with the floor(x / res - 0.5) rule (apd_voxel_group.hip), in double or in float: the voxel starts of
// the `n` points `pts` in scratch s (sorted keys, scanned block counts), the box g of the occupied coordinates and the voxel count nv.
// Two small read-backs (the box, the count).  what / whose: the caller's words in the error texts.
template <typename Real>
int voxel_cell_starts(gorio_apd* h, VoxScratch& s, const float4* pts, int n, Real res, const std::string& what, const char* whose, CellBox<Real>& g, int& nv) {
  HIP_TRY(h, s.bb.reserve(8));
  cell_bbox_init_kernel<<<1, 64, 0, h->stream>>>(s.bb);
  cell_coord_bbox_kernel<Real><<<std::min(256, (n + 255) / 256), 256, 0, h->stream>>>(pts, n, res, s.bb);
  int bb[8];
  HIP_TRY(h, hipMemcpyAsync(bb, s.bb, sizeof(int) * 7, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (bb[6]) return fail(h, GORIO_ERR_UNSUPPORTED, what + ": " + whose + " is not finite or its voxel coordinate does not fit 31 bits");
  double cells = 1.0;
  for (int a = 0; a < 3; ++a) {
    g.min_c[a] = bb[a];
    const long long d = (long long)bb[3 + a] - (long long)bb[a] + 1;
    g.dim[a] = (int)d;
    cells *= (double)d;
  }
  g.res = res;
  if (cells >= 8589934592.0) return fail(h, GORIO_ERR_UNSUPPORTED, what + ": the bounding box of the occupied voxels has 2^33 cells or more (the voxel id is packed into 33 bits of the sort key)");
  const int npow2 = sort_padded_size(n);
  const int nblocks = (n + 255) / 256;
  HIP_TRY(h, s.keys.reserve(npow2));
  HIP_TRY(h, s.counts.reserve(nblocks + 1));
  cell_key_kernel<Real><<<(npow2 + 255) / 256, 256, 0, h->stream>>>(pts, n, npow2, g, s.keys);
  enqueue_tiled_sort(h->stream, SortKeys{s.keys, npow2}, 1, npow2);
  cell_count_kernel<31><<<nblocks, 256, 0, h->stream>>>(s.keys, n, s.counts);
  block_scan_kernel<<<1, 1024, 0, h->stream>>>(s.counts, nblocks);
  nv = 0;
  HIP_TRY(h, hipMemcpyAsync(&nv, s.counts + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (nv <= 0 || nv > n) return fail(h, GORIO_ERR_NO_DEVICE, what + ": inconsistent voxel count");
  return GORIO_OK;
}

// create_voxelmap (VOX:129-156) of target cloud t, whose covariances are valid: the voxel starts, one accumulation pass; nothing to do when
// the map held matches.
int build_voxelmap(gorio_apd* h, DevCloud& t, double res, int mode) {
  const bool mult = mode == GORIO_VOXEL_MULTIPLICATIVE;
  if (t.vm_valid && t.vm.res == res && t.vm_mult == mult) return GORIO_OK;
  t.voxelmap_dropped();
  const int n = t.n;
  VoxScratch& s = t.vox_scratch;
  VoxBox g;
  int nv = 0;
  if (int rc = voxel_cell_starts(h, s, t.p4, n, res, "voxel map", "a target coordinate", g, nv)) return rc;
  HIP_TRY(h, t.vm.reserve(nv));
  vg_accum_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(s.keys, t.p4, t.cov6, n, s.counts, mult ? 2 : 0, t.vm.vkey, t.vm.mean, t.vm.cov6, t.vm.num);
  HIP_TRY(h, hipGetLastError());
  t.vm.set_geometry(g, nv);
  t.vm_mult = mult;
  t.voxelmap_built();
  return GORIO_OK;
}

// slot table, Mahalanobis blocks and block partials of this handle's (source point, offset) slots
int ensure_voxel_pair(gorio_apd* h) {
  const int n_off = voxel_offsets(h->voxel_search);
  const size_t total = (size_t)h->src->n * n_off;
  const size_t cap = total + total / 8 + 256;
  HIP_TRY(h, reserve_group(h->v_cap, total, cap, h->v_slots, cap, h->v_omega6, 6 * cap, h->v_partials, 28 * (cap / 256 + 2)));
  h->v_n_off = n_off;
  return GORIO_OK;
}

VoxPair make_vox_pair(const gorio_apd* h, int write_omega) {
  VoxPair v;
  v.map = h->tgt->vm.view();
  v.slots = h->v_slots;
  v.omega6 = h->v_omega6;
  v.n_off = h->v_n_off;
  v.write_omega = write_omega;
  return v;
}

// ---- fast_gicp::NDTCuda plumbing (apd_ndt_cuda.hip)

bool is_ndtc(const gorio_apd* h) { return h->method == GORIO_METHOD_NDT_CUDA; }

// 0 < radius <= 3 (at most 123 offsets); ndt_cuda.cu:70-84 would build an empty table for radius <= 0
int ndtc_check_radius(gorio_apd* h, double radius) {
  if (!(radius > 0.0) || !std::isfinite(radius)) return fail(h, GORIO_ERR_INVALID, "NDTCuda: the DIRECT_RADIUS radius must be positive and finite (gorio_apd_set_ndt_cuda_params)");
  if (radius > 3.0) return fail(h, GORIO_ERR_UNSUPPORTED, "NDTCuda: a DIRECT_RADIUS radius above 3 voxels is not supported");
  return GORIO_OK;
}

// set_neighbor_search_method, ndt_cuda.cu:35-88, in table order
std::vector<int> ndtc_offset_table(int search, double radius) {
  std::vector<int> o;
  auto push = [&o](int i, int j, int k) { o.push_back(i); o.push_back(j); o.push_back(k); };
  if (search == GORIO_VOXEL_DIRECT1) {
    push(0, 0, 0);
  } else if (search == GORIO_VOXEL_DIRECT7) {
    push(0, 0, 0); push(1, 0, 0); push(-1, 0, 0); push(0, 1, 0); push(0, -1, 0); push(0, 0, 1); push(0, 0, -1);
  } else if (search == GORIO_VOXEL_DIRECT27) {
    for (int i = -1; i <= 1; ++i)
      for (int j = -1; j <= 1; ++j)
        for (int k = -1; k <= 1; ++k) push(i, j, k);
  } else {
    const int range = (int)std::ceil(radius);
    for (int i = -range; i <= range; ++i)
      for (int j = -range; j <= range; ++j)
        for (int k = -range; k <= range; ++k)
          if (std::sqrt((double)(i * i + j * j + k * k)) <= radius + 1e-3) push(i, j, k);
  }
  return o;
}

bool ndtc_same_settings(const gorio_apd* a, const gorio_apd* b) {
  return a->voxel_resolution == b->voxel_resolution && a->voxel_search == b->voxel_search && a->ndtc_mode == b->ndtc_mode &&
         (a->voxel_search != GORIO_VOXEL_DIRECT_RADIUS || a->ndtc_radius == b->ndtc_radius);
}

// a cloud shared with other handles carries ONE map: a sharer with another resolution would rebuild it under the others
bool ndtc_shared_mismatch(const gorio_apd* h, const std::shared_ptr<DevCloud>& c) {
  return c.use_count() > 1 && c->nc_valid && c->nc.res != (float)h->voxel_resolution;
}

int ndtc_ready(gorio_apd* h) {
  if (!h->src->present) return fail(h, GORIO_ERR_STATE, "no input source set (setInputSource)");
  if (!h->tgt->present) return fail(h, GORIO_ERR_STATE, "no input target set (setInputTarget)");
  if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "NDTCuda has no sharded-source mode (gorio_apd_comm_init / gorio_apd_debug_set_shard): use an unsharded handle");
  if (ndtc_shared_mismatch(h, h->tgt)) return fail(h, GORIO_ERR_INVALID, "the shared target's NDTCuda voxel map was built with another resolution: give this handle a target of its own (setInputTarget)");
  if (h->ndtc_mode == GORIO_NDT_CUDA_D2D && ndtc_shared_mismatch(h, h->src)) return fail(h, GORIO_ERR_INVALID, "the shared source's NDTCuda voxel map was built with another resolution: give this handle a source of its own (setInputSource)");
  if (h->voxel_search == GORIO_VOXEL_DIRECT_RADIUS) return ndtc_check_radius(h, h->ndtc_radius);
  return GORIO_OK;
}

// create_voxelmap + covariance_regularization (ndt_cuda.cu:120-140) of cloud c: the voxel starts, one accumulation pass; nothing to do
// when the map held matches.  Deviation from the reference: a changed resolution rebuilds the map (ndt_cuda.cu:122, 133 keep the old one).
int build_ndtc_map(gorio_apd* h, DevCloud& c, double resolution) {
  const float res = (float)resolution;
  if (c.nc_valid && c.nc.res == res) return GORIO_OK;
  c.ndtc_map_dropped();
  const int n = c.n;
  VoxScratch& s = c.vox_scratch;
  NdtcBox g;
  int nv = 0;
  if (int rc = voxel_cell_starts(h, s, c.p4, n, res, "NDTCuda voxel map", "a coordinate", g, nv)) return rc;
  HIP_TRY(h, c.nc.reserve(nv));
  HIP_TRY(h, c.nc_raw.reserve(9 * (size_t)nv, 9 * (size_t)c.nc.cap));
  ndtc_accum_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(s.keys, c.p4, n, s.counts, c.nc.vkey, c.nc.mean, c.nc_raw, c.nc.cov6, c.nc.num);
  HIP_TRY(h, hipGetLastError());
  c.nc.set_geometry(g, nv);
  c.ndtc_map_built();
  return GORIO_OK;
}

int ensure_ndtc_slots(gorio_apd* h, int items, int mode);
// the maps a linearisation needs (create_voxelmaps, ndt_cuda.cu:115-140: P2D builds no source map), the offset table, the slot table and
// the block partials of this handle's (offset, item) slots
int ensure_ndtc_pair(gorio_apd* h) {
  int rc = build_ndtc_map(h, *h->tgt, h->voxel_resolution);
  if (rc) return rc;
  const bool d2d = h->ndtc_mode == GORIO_NDT_CUDA_D2D;
  if (d2d) {
    rc = build_ndtc_map(h, *h->src, h->voxel_resolution);
    if (rc) return rc;
  }
  return ensure_ndtc_slots(h, d2d ? h->src->nc.nv : h->src->n, d2d ? 1 : 0);
}

// the offset table on the device, and the slot table and block partials of `items` items (mode: NdtcPair::d2d)
int ensure_ndtc_slots(gorio_apd* h, int items, int mode) {
  if (h->ndtc_off_search != h->voxel_search || (h->voxel_search == GORIO_VOXEL_DIRECT_RADIUS && h->ndtc_off_radius != h->ndtc_radius)) {
    h->ndtc_off_host = ndtc_offset_table(h->voxel_search, h->ndtc_radius);
    HIP_TRY(h, h->ndtc_off.reserve(h->ndtc_off_host.size()));
    HIP_TRY(h, hipMemcpyAsync(h->ndtc_off, h->ndtc_off_host.data(), sizeof(int) * h->ndtc_off_host.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ndtc_n_off = (int)(h->ndtc_off_host.size() / 3);
    h->ndtc_off_search = h->voxel_search;
    h->ndtc_off_radius = h->ndtc_radius;
  }
  const size_t total = (size_t)items * h->ndtc_n_off;
  if (total >= (size_t)INT_MAX) return fail(h, GORIO_ERR_UNSUPPORTED, "NDTCuda: items x offsets does not fit 31 bits");
  const size_t cap = total + total / 8 + 256;
  HIP_TRY(h, reserve_group(h->ndtc_cap, total, cap, h->ndtc_slots, cap, h->ndtc_partials, 28 * (cap / 256 + 2)));
  HIP_TRY(h, h->ndtc_tlin.reserve(12));
  h->ndtc_items = items;
  h->ndtc_slot_off = h->ndtc_n_off;
  h->ndtc_slot_d2d = mode;
  return GORIO_OK;
}

// over the slot table HELD (compute_error reads the stale pairs of the last linearise, ndt_cuda.cu:162-177)
NdtcPair make_ndtc_pair(const gorio_apd* h) {
  NdtcPair p;
  if (h->ndtc_slot_d2d == 2) {  // FastVGICPCuda: the kept source points and their covariances against the map of the kept target points
    p.map = h->tgt->vc_map.view();
    p.item = reinterpret_cast<const float*>(h->src->vc_p4.get());
    p.item_cov6 = h->src->vc_cov6;
    p.offsets = h->ndtc_off;
    p.slots = h->ndtc_slots;
    p.tlin = h->ndtc_tlin;
    p.item_stride = 4;
    p.n_items = h->ndtc_items;
    p.n_off = h->ndtc_slot_off;
    p.d2d = 2;
    return p;
  }
  p.map = h->tgt->nc.view();
  const bool d2d = h->ndtc_slot_d2d != 0;
  p.item = d2d ? h->src->nc.mean.get() : reinterpret_cast<const float*>(h->src->p4.get());
  p.item_cov6 = d2d ? h->src->nc.cov6.get() : nullptr;
  p.offsets = h->ndtc_off;
  p.slots = h->ndtc_slots;
  p.tlin = h->ndtc_tlin;
  p.item_stride = d2d ? 3 : 4;
  p.n_items = h->ndtc_items;
  p.n_off = h->ndtc_slot_off;
  p.d2d = d2d ? 1 : 0;
  return p;
}

void launch_ndtc_linearize(bool d2d, dim3 grid, hipStream_t stream, const PairDesc* d_desc, const NdtcPair* d_pairs) {
  if (d2d) ndtc_linearize_kernel<true><<<grid, 256, 0, stream>>>(d_desc, d_pairs);
  else ndtc_linearize_kernel<false><<<grid, 256, 0, stream>>>(d_desc, d_pairs);
}

// ---- fast_gicp::FastVGICPCuda plumbing (apd_vgicp_cuda.hip)

bool is_vgc(const gorio_apd* h) { return h->method == GORIO_METHOD_VGICP_CUDA; }
bool is_voxf(const gorio_apd* h) { return is_ndtc(h) || is_vgc(h); }  // the two methods of the reference's CUDA back end: float voxel maps, no per-point search state
std::string voxf_name(const gorio_apd* h) { return is_vgc(h) ? "FastVGICPCuda" : "NDTCuda"; }

bool vgc_rbf(const gorio_apd* h) { return h->vgc_nn == GORIO_VGICP_CUDA_NN_GPU_RBF_KERNEL; }
double vgc_max_dist(const gorio_apd* h) { return h->vgc_maxd > 0.0 ? h->vgc_maxd : 5.0 * h->vgc_width; }  // VI:46-50

// does the stage held by cloud c equal the one this handle would make (each stage rests on the one before it)
bool vgc_raw_matches(const gorio_apd* h, const DevCloud& c) {
  if (!c.vc_raw_valid) return false;
  if (vgc_rbf(h)) return c.vc_rbf && c.vc_width == h->vgc_width && c.vc_maxd == vgc_max_dist(h);
  return !c.vc_rbf && c.vc_k == h->params.k_correspondences;  // CPU_PARALLEL_KDTREE and GPU_BRUTEFORCE are one path
}
bool vgc_kept_matches(const gorio_apd* h, const DevCloud& c) { return vgc_raw_matches(h, c) && c.vc_kept_valid && c.vc_reg == h->params.regularization; }
bool vgc_map_matches(const gorio_apd* h, const DevCloud& c) { return vgc_kept_matches(h, c) && c.vc_map_valid && c.vc_map.res == (float)h->voxel_resolution; }

// a cloud other handles hold too carries ONE set of covariances, kept points and map: a sharer that would make any stage HELD
// differently would rebuild it under the others
bool vgc_shared_mismatch(const gorio_apd* h, const std::shared_ptr<DevCloud>& cp, bool with_map) {
  const DevCloud& c = *cp;
  if (cp.use_count() <= 1) return false;
  if (c.vc_raw_valid && !vgc_raw_matches(h, c)) return true;
  if (c.vc_kept_valid && c.vc_reg != h->params.regularization) return true;
  return with_map && c.vc_map_valid && c.vc_map.res != (float)h->voxel_resolution;
}

int vgc_cloud_ready(gorio_apd* h, const DevCloud& c, const char* side) {
  const gorio_apd_params& p = h->params;
  if (p.regularization < 0 || p.regularization > 4) return fail(h, GORIO_ERR_UNSUPPORTED, "unknown regularization method");
  if (vgc_rbf(h) || vgc_raw_matches(h, c)) return GORIO_OK;
  if (p.k_correspondences < 1 || p.k_correspondences > 32) return fail(h, GORIO_ERR_UNSUPPORTED, "k_correspondences must be in [1, 32]");
  if (c.n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, std::string(side) + " cloud has fewer points than k_correspondences (the k-NN list would hold padding)");
  return GORIO_OK;
}

int vgc_ready(gorio_apd* h) {
  if (!h->src->present) return fail(h, GORIO_ERR_STATE, "no input source set (setInputSource)");
  if (!h->tgt->present) return fail(h, GORIO_ERR_STATE, "no input target set (setInputTarget)");
  if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "FastVGICPCuda has no sharded-source mode (gorio_apd_comm_init / gorio_apd_debug_set_shard): use an unsharded handle");
  if (vgc_shared_mismatch(h, h->tgt, true)) return fail(h, GORIO_ERR_INVALID, "the shared target's FastVGICPCuda covariances / kept points / voxel map were made with other settings: give this handle a target of its own (setInputTarget)");
  if (vgc_shared_mismatch(h, h->src, false)) return fail(h, GORIO_ERR_INVALID, "the shared source's FastVGICPCuda covariances / kept points were made with other settings: give this handle a source of its own (setInputSource)");
  if (int rc = vgc_cloud_ready(h, *h->src, "source")) return rc;
  if (int rc = vgc_cloud_ready(h, *h->tgt, "target")) return rc;
  if (h->voxel_search == GORIO_VOXEL_DIRECT_RADIUS) return ndtc_check_radius(h, h->ndtc_radius);
  return GORIO_OK;
}

// stage 1: the float covariance of every point (VC:183-219)
int vgc_covariances(gorio_apd* h, DevCloud& c) {
  if (vgc_raw_matches(h, c)) return GORIO_OK;
  c.vgc_raw_dropped();
  const int n = c.n;
  {
    const size_t cap = (size_t)n + n / 8 + 64;
    HIP_TRY(h, reserve_group(c.vc_cap, n, cap, c.vc_raw6, 6 * cap, c.vc_reg6, 6 * cap, c.vc_keep, cap, c.vc_p4, cap, c.vc_cov6, 6 * cap, c.vc_index, cap));
  }
  const unsigned int nblk = (unsigned int)((n + 255) / 256);
  if (vgc_rbf(h)) {  // no list, no search index: every point against every block of 512 (RB:116-151)
    const int nb = (n + kRbfBlock - 1) / kRbfBlock;
    // the partials of at most 64 M floats' worth of blocks at a time; the running sums wait in the first chunk's tail between chunks
    const int per = std::max(1, (int)std::min<size_t>((size_t)nb, ((size_t)64 << 20) / ((size_t)kRbfTerms * n)));
    HIP_TRY(h, c.vc_part.reserve((size_t)(per + 1) * kRbfTerms * n));
    float* acc = c.vc_part + (size_t)per * kRbfTerms * n;
    const float g = (float)h->vgc_width, md = (float)vgc_max_dist(h);
    for (int b0 = 0; b0 < nb; b0 += per) {
      const int cnt = std::min(per, nb - b0);
      vgc_cov_rbf_kernel<<<dim3(nblk, (unsigned int)cnt), 256, 0, h->stream>>>(c.p4, n, b0, g, md * md, c.vc_part);
      vgc_cov_rbf_fold_kernel<<<nblk, 256, 0, h->stream>>>(c.vc_part, n, cnt, acc, b0 == 0 ? 1 : 0, b0 + cnt == nb ? 1 : 0, c.vc_raw6);
    }
    HIP_TRY(h, hipGetLastError());
    c.vgc_raw_built(true, 0, h->vgc_width, vgc_max_dist(h));
    return GORIO_OK;
  }
  const int k = h->params.k_correspondences;
  HIP_TRY(h, c.vc_knn.reserve((size_t)n * k));
  HIP_TRY(h, c.vc_scratch.reserve((size_t)7 * n));
  {  // the handle's exact k-NN kernels, by params.search (pruned: the search index is built when stale)
    std::vector<std::pair<gorio_apd*, DevCloud*>> one = {{h, &c}};
    const KnnListsOnly only = {c.vc_knn, c.vc_scratch, c.vc_scratch + (size_t)6 * n};
    if (int rc = run_covariances(h, one, &only)) return rc;
  }
  vgc_cov_knn_kernel<<<nblk, 256, 0, h->stream>>>(c.p4, c.vc_knn, n, k, c.vc_raw6);
  HIP_TRY(h, hipGetLastError());
  c.vgc_raw_built(false, k, 0.0, 0.0);
  return GORIO_OK;
}

// stage 2: covariance_regularization (CR:91-117) and the ordered compaction of the points it keeps.  One small read-back (the count).
int vgc_filter(gorio_apd* h, DevCloud& c) {
  if (int rc = vgc_covariances(h, c)) return rc;
  if (vgc_kept_matches(h, c)) return GORIO_OK;
  c.vgc_kept_dropped();
  const int n = c.n;
  const int nblk = (n + 255) / 256;
  HIP_TRY(h, c.vc_bcnt.reserve(nblk + 1));
  vgc_regularize_kernel<<<nblk, 256, 0, h->stream>>>(c.vc_raw6, n, h->params.regularization, c.vc_keep, c.vc_reg6);
  compact_count_kernel<<<nblk, 256, 0, h->stream>>>(c.vc_keep, n, c.vc_bcnt);
  block_scan_kernel<<<1, 1024, 0, h->stream>>>(c.vc_bcnt, nblk);
  vgc_scatter_kernel<<<nblk, 256, 0, h->stream>>>(c.p4, c.vc_reg6, c.vc_keep, n, c.vc_bcnt, c.vc_p4, c.vc_cov6, c.vc_index);
  HIP_TRY(h, hipGetLastError());
  int nkept = 0;
  HIP_TRY(h, hipMemcpyAsync(&nkept, c.vc_bcnt + nblk, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (nkept < 0 || nkept > n) return fail(h, GORIO_ERR_NO_DEVICE, "FastVGICPCuda: inconsistent kept-point count");
  c.vgc_kept_built(h->params.regularization, nkept);
  return GORIO_OK;
}

// stage 3: the voxel map of the kept points (GV:229-252).  No kept point: an empty map, in which every lookup misses.  Deviation from
// the reference: a changed resolution rebuilds the map (VI:41-43, 145; VC:257-263).
int build_vgc_map(gorio_apd* h, DevCloud& c) {
  if (int rc = vgc_filter(h, c)) return rc;
  if (vgc_map_matches(h, c)) return GORIO_OK;
  c.vgc_map_dropped();
  const float res = (float)h->voxel_resolution;
  const int n = c.vc_nkept;
  VoxScratch& s = c.vox_scratch;
  NdtcBox g = {{0, 0, 0}, {0, 0, 0}, res};
  int nv = 0;
  if (n > 0) {
    if (int rc = voxel_cell_starts(h, s, c.vc_p4, n, res, "NDTCuda voxel map", "a coordinate", g, nv)) return rc;
    HIP_TRY(h, c.vc_map.reserve(nv));
    vgc_accum_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(s.keys, c.vc_p4, c.vc_cov6, n, s.counts, c.vc_map.vkey, c.vc_map.mean, c.vc_map.cov6, c.vc_map.num);
    HIP_TRY(h, hipGetLastError());
  }
  c.vc_map.set_geometry(g, nv);
  c.vgc_map_built();
  return GORIO_OK;
}

// everything a linearisation needs: both clouds filtered, the target's map, the offset and slot tables over the kept source points
int ensure_vgc_pair(gorio_apd* h) {
  int rc = vgc_filter(h, *h->src);
  if (!rc) rc = build_vgc_map(h, *h->tgt);
  if (rc) return rc;
  return ensure_ndtc_slots(h, h->src->vc_nkept, 2);
}

bool vgc_same_settings(const gorio_apd* a, const gorio_apd* b) {
  return a->voxel_resolution == b->voxel_resolution && a->voxel_search == b->voxel_search &&
         (a->voxel_search != GORIO_VOXEL_DIRECT_RADIUS || a->ndtc_radius == b->ndtc_radius) && a->vgc_nn == b->vgc_nn && a->vgc_width == b->vgc_width &&
         a->vgc_maxd == b->vgc_maxd;
}

int check_ready(gorio_apd* h) {
  if (!h->src->present) return fail(h, GORIO_ERR_STATE, "no input source set (setInputSource)");
  if (!h->tgt->present) return fail(h, GORIO_ERR_STATE, "no input target set (setInputTarget)");
  const gorio_apd_params& p = h->params;
  if (shared_cov_mismatch(h)) return fail(h, GORIO_ERR_INVALID, "the shared target's covariances were estimated with another k_correspondences / regularization: give this handle a target of its own (setInputTarget)");
  if (shared_source_cov_mismatch(h)) return fail(h, GORIO_ERR_INVALID, "the shared source's covariances were estimated with another k_correspondences / regularization: give this handle a source of its own (setInputSource)");
  if (shared_voxel_mismatch(h)) return fail(h, GORIO_ERR_INVALID, "the shared target's voxel map was built with another voxel_resolution / voxel_mode: give this handle a target of its own (setInputTarget)");
  if (h->method == GORIO_METHOD_VGICP && (h->comm || (h->shard_only && h->comm_world > 1)))
    return fail(h, GORIO_ERR_STATE, "FastVGICP has no sharded-source mode (gorio_apd_comm_init / gorio_apd_debug_set_shard): use an unsharded handle");
  if (p.k_correspondences < 1 || p.k_correspondences > 32) return fail(h, GORIO_ERR_UNSUPPORTED, "k_correspondences must be in [1, 32]");
  if (p.regularization < 0 || p.regularization > 4) return fail(h, GORIO_ERR_UNSUPPORTED, "unknown regularization method (the reference aborts here, APD:389-391)");
  if (h->src->cov_count != h->src->n && h->src->n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, "source cloud has fewer points than k_correspondences (undefined in the reference, APD:366-369)");
  if (h->tgt->cov_count != h->tgt->n && h->tgt->n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, "target cloud has fewer points than k_correspondences (undefined in the reference, APD:366-369)");
  return GORIO_OK;
}

void fill_desc(gorio_apd* h, PairDesc& d, PairState* state, long total_src_waves) {
  d.src = h->src->view();
  d.tgt = h->tgt->view();
  d.best_key = h->best_key;
  d.seed = h->seed;
  d.nn_work = h->nn_work;
  d.nn_plan = h->nn_plan;
  d.nn_wcap = h->nn_wcap;
  d.pad0_ = 0;
  d.corr = h->corr;
  d.sqd = h->sqd;
  d.omega6 = h->omega6;
  d.partials = h->partials;
  d.state = state;
  d.nblk = (h->src->n + 255) / 256;
  int splits = (int)((8192 + total_src_waves - 1) / total_src_waves);
  if (splits < 1) splits = 1;
  if (splits > 64) splits = 64;
  int chunk = roundup((h->tgt->n_pad + splits - 1) / splits, kPad);
  if (chunk < 512) chunk = 512;
  d.nn_chunk = chunk;
  d.nn_splits = (h->tgt->n_pad + chunk - 1) / chunk;
  d.cl_points = h->params.cl_weight_points;
  d.write_omega = 1;
  d.shard_lo = 0;
  d.shard_hi = INT_MAX;
  if ((h->comm || h->shard_only) && h->comm_world > 1) {
    // this rank's contiguous part of the query order, in units of 256 (one workgroup): sorted positions for the pruned search (a
    // spatially compact part of the scan), original indices for the exhaustive one.  Which points a rank owns changes the order of
    // the fp64 sums, never their value beyond rounding.
    const int nq = h->params.search == GORIO_SEARCH_PRUNED ? roundup(h->src->n, 512) : h->src->n;
    const long nb = (nq + 255) / 256;
    d.shard_lo = (int)(nb * h->comm_rank / h->comm_world) * 256;
    d.shard_hi = h->comm_rank == h->comm_world - 1 ? INT_MAX : (int)(nb * (h->comm_rank + 1) / h->comm_world) * 256;
  }
}

void init_state(PairState& s, const double* T16) {
  std::memset(&s, 0, sizeof(s));
  for (int i = 0; i < 16; ++i) s.x0[i] = T16[i];
  s.x0[12] = 0; s.x0[13] = 0; s.x0[14] = 0; s.x0[15] = 1;
  for (int i = 0; i < 16; ++i) s.xi[i] = s.x0[i];
  for (int i = 0; i < 12; ++i) s.Tf[i] = (float)s.x0[i];
  s.lambda = -1.0;
  for (int i = 0; i < 6; ++i) s.Hfin[i * 6 + i] = 1.0;  // final_hessian_.setIdentity(), LSQ:23
}

// batched helpers driven by the descriptor array
__global__ __launch_bounds__(256) void arm_keys_kernel(const PairDesc* __restrict__ descs) {
  const PairDesc& pd = descs[blockIdx.y];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < pd.src.n; i += gridDim.x * 256) pd.best_key[i] = ~0ull;
  if (pd.nn_work)
    for (int i = blockIdx.x * 256 + threadIdx.x; i < pd.nn_wcap; i += gridDim.x * 256) {
      pd.nn_work[i] = 0u;
      pd.nn_work[pd.nn_wcap + i] = 0u;
    }
}
__global__ __launch_bounds__(64) void gather_states_kernel(const PairDesc* __restrict__ descs, PairState* __restrict__ out) {
  const unsigned int* s = reinterpret_cast<const unsigned int*>(descs[blockIdx.x].state);
  unsigned int* d = reinterpret_cast<unsigned int*>(out + blockIdx.x);
  for (int q = threadIdx.x; q < (int)(sizeof(PairState) / 4); q += 64) d[q] = s[q];
}
__global__ __launch_bounds__(64) void scatter_states_kernel(const PairDesc* __restrict__ descs, const PairState* __restrict__ in) {
  unsigned int* d = reinterpret_cast<unsigned int*>(descs[blockIdx.x].state);
  const unsigned int* s = reinterpret_cast<const unsigned int*>(in + blockIdx.x);
  for (int q = threadIdx.x; q < (int)(sizeof(PairState) / 4); q += 64) d[q] = s[q];
}

int ensure_batch(gorio_apd* lead, int count) {
  HIP_TRY(lead, reserve_group(lead->desc_cap, count, count, lead->d_desc, count, lead->d_states_batch, count));
  return GORIO_OK;
}

// A batch member's failure is reported on the handle that leads the batch
int hand_over(gorio_apd* lead, gorio_apd* h, int rc) {
  if (rc && h != lead) lead->err = h->err;
  return rc;
}

#include "apd_lsq.hip"

// Search bound of a fitness score: nothing farther than max(max_range, inlier_dist^2) is counted by either statistic (rounded up to a float).
float fitness_bound(double max_range, double inlier_sq) {
  const double lim = std::max(max_range, inlier_sq);
  float bf = FLT_MAX;
  if (lim < (double)FLT_MAX) {
    bf = (float)lim;
    if ((double)bf < lim) bf = std::nextafterf(bf, FLT_MAX);
  }
  return bf;
}

// workgroups per query wave of a fitness score's pruned search (a power of two in [1, 16]); any value returns the same keys
int fitness_splits(long waves) {
  int splits = (int)std::min<long>(16, std::max<long>(1, 4096 / (waves > 0 ? waves : 1)));
  while (splits & (splits - 1)) splits &= splits - 1;
  return splits;
}

// the descriptor of a fitness score's search
int single_desc(gorio_apd* h) {
  int rc = ensure_batch(h, 1);
  if (rc) return rc;
  PairDesc d;
  fill_desc(h, d, h->d_state, (h->src->n + 63) / 64);
  HIP_TRY(h, hipMemcpyAsync(h->d_desc, &d, sizeof(PairDesc), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

}  // namespace

// =============================================================================================== C ABI

extern "C" {

void gorio_apd_default_params(gorio_apd_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->k_correspondences = 20;
  p->regularization = GORIO_REG_PLANE;
  p->dist_var = 0.86;
  p->azimuth_var = 0.5;
  p->elevation_var = 1.0;
  p->corr_dist_threshold = (double)FLT_MAX;
  p->max_iterations = 64;
  p->rotation_epsilon = 2e-3;
  p->transformation_epsilon = 5e-4;
  p->optimizer = GORIO_OPT_LEVENBERG_MARQUARDT;
  p->lm_max_iterations = 10;
  p->lm_init_lambda_factor = 1e-9;
  p->search = GORIO_SEARCH_BRUTE_FORCE;
  p->cl_weight_points = 0;
  p->keep_knn_indices = 0;
}

int gorio_apd_create(gorio_apd_t** out, int device) {
  if (!out) return GORIO_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GORIO_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return GORIO_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess) return GORIO_ERR_NO_DEVICE;
  gorio_apd* h = new (std::nothrow) gorio_apd();
  if (!h) return GORIO_ERR_ALLOC;
  h->device = device;
  h->src = std::make_shared<DevCloud>();
  h->tgt = std::make_shared<DevCloud>();
  h->src->device = h->tgt->device = device;
  gorio_apd_default_params(&h->params);
  h->stream = device_stream(device);
  {  // the fence-free "last workgroup runs the optimiser step" hand-over relies on how gfx950 writes through and acknowledges sc1 stores across
     // its XCD L2s: it was validated there and is switched off on anything else (the step then takes its own launch)
    hipDeviceProp_t prop;
    h->fuse_supported = hipGetDeviceProperties(&prop, device) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    h->fuse_step = h->fuse_supported;
  }
  if (!h->stream || h->d_state.reserve(1) != hipSuccess || h->d_red.reserve(32) != hipSuccess) {  // d_fit grows with its first fitness score
    delete h;
    return GORIO_ERR_NO_DEVICE;
  }
  *out = h;
  return GORIO_OK;
}

void gorio_apd_destroy(gorio_apd_t* h) {
  if (!h) return;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  if (h->comm && rccl().ok) rccl().CommDestroy(h->comm);
  delete h;  // events, clouds and buffers: ~gorio_apd and its members
}

const char* gorio_apd_last_error(const gorio_apd_t* h) { return h ? h->err.c_str() : "null handle"; }

int gorio_apd_set_params(gorio_apd_t* h, const gorio_apd_params* p) {
  if (!h || !p) return GORIO_ERR_INVALID;
  if (p->k_correspondences < 1 || p->k_correspondences > 32) return fail(h, GORIO_ERR_UNSUPPORTED, "k_correspondences must be in [1, 32]");
  if (p->regularization < 0 || p->regularization > 4) return fail(h, GORIO_ERR_UNSUPPORTED, "unknown regularization method");
  if (p->optimizer != GORIO_OPT_GAUSS_NEWTON && p->optimizer != GORIO_OPT_LEVENBERG_MARQUARDT) return fail(h, GORIO_ERR_INVALID, "unknown optimizer");
  std::memset(&h->params, 0, sizeof(h->params));  // padding bytes stay zero so whole-struct comparisons (batch validation) are meaningful
  h->params.k_correspondences = p->k_correspondences; h->params.regularization = p->regularization;
  h->params.dist_var = p->dist_var; h->params.azimuth_var = p->azimuth_var; h->params.elevation_var = p->elevation_var;
  h->params.corr_dist_threshold = p->corr_dist_threshold; h->params.max_iterations = p->max_iterations;
  h->params.rotation_epsilon = p->rotation_epsilon; h->params.transformation_epsilon = p->transformation_epsilon;
  h->params.optimizer = p->optimizer; h->params.lm_max_iterations = p->lm_max_iterations; h->params.lm_init_lambda_factor = p->lm_init_lambda_factor;
  h->params.search = p->search; h->params.cl_weight_points = p->cl_weight_points; h->params.keep_knn_indices = p->keep_knn_indices;
  return GORIO_OK;
}

int gorio_apd_get_params(const gorio_apd_t* h, gorio_apd_params* p) {
  if (!h || !p) return GORIO_ERR_INVALID;
  *p = h->params;
  return GORIO_OK;
}

int gorio_apd_set_method(gorio_apd_t* h, int method, double voxel_resolution, int voxel_search, int voxel_mode) {
  if (!h) return GORIO_ERR_INVALID;
  if (method != GORIO_METHOD_APDGICP && method != GORIO_METHOD_GICP && method != GORIO_METHOD_VGICP && method != GORIO_METHOD_GICP_OMP && method != GORIO_METHOD_ICP && method != GORIO_METHOD_NDT_CUDA && method != GORIO_METHOD_VGICP_CUDA && method != GORIO_METHOD_GICP_MP) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: unknown registration method");
  if (method == GORIO_METHOD_NDT_CUDA || method == GORIO_METHOD_VGICP_CUDA) {  // voxel_resolution = setResolution, voxel_search = setNeighborSearchMethod (DIRECT_RADIUS with the radius of gorio_apd_set_ndt_cuda_params); voxel_mode is ignored: the handle keeps the one it has
    if (voxel_search != GORIO_VOXEL_DIRECT27 && voxel_search != GORIO_VOXEL_DIRECT7 && voxel_search != GORIO_VOXEL_DIRECT1 && voxel_search != GORIO_VOXEL_DIRECT_RADIUS) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: unknown neighbour search method");
    if (!(voxel_resolution > 0.0) || !std::isfinite(voxel_resolution)) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: voxel_resolution must be positive");
    if (h->comm || (h->shard_only && h->comm_world > 1)) return fail(h, GORIO_ERR_STATE, "set_method: NDTCuda and FastVGICPCuda have no sharded-source mode");
    if (voxel_search == GORIO_VOXEL_DIRECT_RADIUS)
      if (int rc = ndtc_check_radius(h, h->ndtc_radius)) return rc;
    voxel_mode = h->voxel_mode;
  } else if (method == GORIO_METHOD_GICP_OMP || method == GORIO_METHOD_ICP || method == GORIO_METHOD_GICP_MP) {  // the voxel arguments are ignored in these modes: the handle keeps the ones it has
    if (h->comm) return fail(h, GORIO_ERR_STATE, "set_method: GICP_OMP, ICP and FastGICPMultiPoints have no sharded-source mode (the handle has a communicator)");
    if (method != GORIO_METHOD_GICP_OMP && h->shard_only && h->comm_world > 1) return fail(h, GORIO_ERR_STATE, "set_method: ICP and FastGICPMultiPoints have no sharded-source mode (gorio_apd_debug_set_shard is on)");
    voxel_resolution = h->voxel_resolution;
    voxel_search = h->voxel_search;
    voxel_mode = h->voxel_mode;
  } else {
    if (voxel_search == GORIO_VOXEL_DIRECT_RADIUS) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: DIRECT_RADIUS is not supported (the reference aborts there, VOX:13-15)");
    if (voxel_search != GORIO_VOXEL_DIRECT27 && voxel_search != GORIO_VOXEL_DIRECT7 && voxel_search != GORIO_VOXEL_DIRECT1) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: unknown neighbour search method");
    if (voxel_mode != GORIO_VOXEL_ADDITIVE && voxel_mode != GORIO_VOXEL_ADDITIVE_WEIGHTED && voxel_mode != GORIO_VOXEL_MULTIPLICATIVE) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: unknown voxel accumulation mode");
    if (!(voxel_resolution > 0.0) || !std::isfinite(voxel_resolution)) return fail(h, GORIO_ERR_UNSUPPORTED, "set_method: voxel_resolution must be positive");
    if (method == GORIO_METHOD_VGICP && h->comm) return fail(h, GORIO_ERR_STATE, "set_method: FastVGICP has no sharded-source mode (the handle has a communicator)");
  }
  h->method = method;
  h->voxel_resolution = voxel_resolution;
  h->voxel_search = voxel_search;
  h->voxel_mode = voxel_mode;
  h->method_switched();
  return GORIO_OK;
}

int gorio_apd_get_method(const gorio_apd_t* h, int* method, double* voxel_resolution, int* voxel_search, int* voxel_mode) {
  if (!h) return GORIO_ERR_INVALID;
  if (method) *method = h->method;
  if (voxel_resolution) *voxel_resolution = h->voxel_resolution;
  if (voxel_search) *voxel_search = h->voxel_search;
  if (voxel_mode) *voxel_mode = h->voxel_mode;
  return GORIO_OK;
}

int gorio_apd_get_voxelmap(gorio_apd_t* h, int* coord3, int* num_points, double* mean4, double* cov16, int capacity, int* n_voxels) {
  if (!h || !n_voxels) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_VGICP) return fail(h, GORIO_ERR_STATE, "get_voxelmap: the handle is not in FastVGICP mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  DevCloud& t = *h->tgt;  // the map depends on the target alone: no source is asked for, none is processed
  if (!t.present) return fail(h, GORIO_ERR_STATE, "get_voxelmap: no input target set (setInputTarget)");
  if (shared_cov_mismatch(h)) return fail(h, GORIO_ERR_INVALID, "the shared target's covariances were estimated with another k_correspondences / regularization");
  if (shared_voxel_mismatch(h)) return fail(h, GORIO_ERR_INVALID, "the shared target's voxel map was built with another voxel_resolution / voxel_mode");
  int rc = GORIO_OK;
  if (t.cov_count != t.n) {  // calculate_covariances (GICP:262-330) of the target only
    const gorio_apd_params& p = h->params;
    if (p.k_correspondences < 1 || p.k_correspondences > 32) return fail(h, GORIO_ERR_UNSUPPORTED, "k_correspondences must be in [1, 32]");
    if (t.n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, "target cloud has fewer points than k_correspondences (undefined in the reference, APD:366-369)");
    std::vector<std::pair<gorio_apd*, DevCloud*>> todo = {{h, &t}};
    if (p.search == GORIO_SEARCH_PRUNED) rc = run_index_build(h, todo);
    if (!rc) rc = run_covariances(h, todo);
    if (rc) return rc;
  }
  rc = build_voxelmap(h, t, h->voxel_resolution, h->voxel_mode);
  if (rc) return rc;
  const int nv = t.vm.nv;
  *n_voxels = nv;
  if (capacity < nv || (!coord3 && !num_points && !mean4 && !cov16)) return GORIO_OK;
  std::vector<unsigned long long> vkey(nv);
  std::vector<double> mean((size_t)nv * 3), c6((size_t)nv * 6);
  std::vector<int> num(nv);
  HIP_TRY(h, hipMemcpyAsync(vkey.data(), t.vm.vkey, sizeof(unsigned long long) * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(mean.data(), t.vm.mean, sizeof(double) * 3 * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c6.data(), t.vm.cov6, sizeof(double) * 6 * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(num.data(), t.vm.num, sizeof(int) * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const double c33 = t.vm_mult ? 1.0 : 0.0;  // finalize(): the multiplicative voxel inverts a matrix whose (3,3) is 1 (VOX:97-100), the additive one divides a 0
  if (coord3) t.vm.decode_coords(vkey.data(), coord3);
  for (int v = 0; v < nv; ++v) {
    if (num_points) num_points[v] = num[v];
    if (mean4) {
      double* o = mean4 + 4 * (size_t)v;
      o[0] = mean[3 * (size_t)v]; o[1] = mean[3 * (size_t)v + 1]; o[2] = mean[3 * (size_t)v + 2]; o[3] = 1.0;
    }
    if (cov16) {
      const double* q = c6.data() + 6 * (size_t)v;
      double* o = cov16 + 16 * (size_t)v;
      o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = 0;
      o[4] = q[1]; o[5] = q[3]; o[6] = q[4]; o[7] = 0;
      o[8] = q[2]; o[9] = q[4]; o[10] = q[5]; o[11] = 0;
      o[12] = 0; o[13] = 0; o[14] = 0; o[15] = c33;
    }
  }
  return GORIO_OK;
}

int gorio_apd_get_voxel_correspondences(gorio_apd_t* h, int* voxel_idx, int n_source_times_offsets) {
  if (!h || !voxel_idx) return GORIO_ERR_INVALID;
  if (h->method != GORIO_METHOD_VGICP) return fail(h, GORIO_ERR_STATE, "get_voxel_correspondences: the handle is not in FastVGICP mode (gorio_apd_set_method)");
  if (!h->corr_valid || !h->v_slots) return fail(h, GORIO_ERR_STATE, "no voxel correspondences held");
  if ((size_t)n_source_times_offsets != (size_t)h->src->n * h->v_n_off) return fail(h, GORIO_ERR_INVALID, "get_voxel_correspondences: size mismatch");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(voxel_idx, h->v_slots, sizeof(int) * (size_t)n_source_times_offsets, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_apd_set_ndt_cuda_params(gorio_apd_t* h, int distance_mode, double radius) {
  if (!h) return GORIO_ERR_INVALID;
  if (distance_mode != GORIO_NDT_CUDA_P2D && distance_mode != GORIO_NDT_CUDA_D2D) return fail(h, GORIO_ERR_INVALID, "set_ndt_cuda_params: distance_mode must be P2D (0) or D2D (1)");
  if (std::isnan(radius)) return fail(h, GORIO_ERR_INVALID, "set_ndt_cuda_params: radius is NaN");
  if (is_voxf(h) && h->voxel_search == GORIO_VOXEL_DIRECT_RADIUS)  // the radius is in use: it must be a usable one
    if (int rc = ndtc_check_radius(h, radius)) return rc;
  h->ndtc_mode = distance_mode;
  h->ndtc_radius = radius;
  if (is_voxf(h)) h->corr_valid = false;  // pairs of another item set or neighbourhood
  return GORIO_OK;
}

int gorio_apd_get_ndt_cuda_params(const gorio_apd_t* h, int* distance_mode, double* radius) {
  if (!h) return GORIO_ERR_INVALID;
  if (distance_mode) *distance_mode = h->ndtc_mode;
  if (radius) *radius = h->ndtc_radius;
  return GORIO_OK;
}

int gorio_apd_ndt_cuda_get_voxels(gorio_apd_t* h, int which, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov_raw, float* cov) {
  if (!h || !n_voxels || (which != 0 && which != 1)) return GORIO_ERR_INVALID;
  if (!is_ndtc(h)) return fail(h, GORIO_ERR_STATE, "ndt_cuda_get_voxels: the handle is not in NDTCuda mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  const std::shared_ptr<DevCloud>& cp = which == 0 ? h->src : h->tgt;
  DevCloud& c = *cp;
  if (!c.present) return fail(h, GORIO_ERR_STATE, "ndt_cuda_get_voxels: that cloud is not set");
  if (ndtc_shared_mismatch(h, cp)) return fail(h, GORIO_ERR_INVALID, "ndt_cuda_get_voxels: the shared cloud's map was built with another resolution");
  if (which == 0 && h->ndtc_mode == GORIO_NDT_CUDA_P2D) {  // P2D builds no source map (NC:122): report the one held, if any
    if (!c.nc_valid || c.nc.res != (float)h->voxel_resolution) {
      *n_voxels = 0;
      return GORIO_OK;
    }
  } else if (int rc = build_ndtc_map(h, c, h->voxel_resolution)) {
    return rc;
  }
  const int nv = c.nc.nv;
  *n_voxels = nv;
  if (capacity < nv || (!coords && !num_points && !mean && !cov_raw && !cov)) return GORIO_OK;
  std::vector<unsigned long long> vkey(nv);
  std::vector<float> c6((size_t)nv * 6);
  HIP_TRY(h, hipMemcpyAsync(vkey.data(), c.nc.vkey, sizeof(unsigned long long) * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipMemcpyAsync(c6.data(), c.nc.cov6, sizeof(float) * 6 * nv, hipMemcpyDeviceToHost, h->stream));
  if (num_points) HIP_TRY(h, hipMemcpyAsync(num_points, c.nc.num, sizeof(int) * nv, hipMemcpyDeviceToHost, h->stream));
  if (mean) HIP_TRY(h, hipMemcpyAsync(mean, c.nc.mean, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost, h->stream));
  if (cov_raw) HIP_TRY(h, hipMemcpyAsync(cov_raw, c.nc_raw, sizeof(float) * 9 * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (coords) c.nc.decode_coords(vkey.data(), coords);
  for (int v = 0; v < nv; ++v) {
    if (cov) {
      const float* q = c6.data() + 6 * (size_t)v;
      float* o = cov + 9 * (size_t)v;
      o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
      o[3] = q[1]; o[4] = q[3]; o[5] = q[4];
      o[6] = q[2]; o[7] = q[4]; o[8] = q[5];
    }
  }
  return GORIO_OK;
}

// the pair list of the slot table held, offset-major then item order (both float voxel methods)
static int voxf_get_pairs(gorio_apd* h, int capacity, int* n_pairs, int* item, int* voxel) {
  const size_t total = (size_t)h->ndtc_items * h->ndtc_slot_off;  // 0 when FastVGICPCuda's filter kept no source point: an empty list, no slot table
  if (!h->corr_valid || (total && !h->ndtc_slots)) return fail(h, GORIO_ERR_STATE, "get_pairs: no pairs held (gorio_apd_linearize or an align first)");
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<int> slots(total);
  if (total) {
    HIP_TRY(h, hipMemcpyAsync(slots.data(), h->ndtc_slots, sizeof(int) * total, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  int np = 0;
  for (size_t t = 0; t < total; ++t) np += slots[t] >= 0;
  *n_pairs = np;
  if (capacity < np || (!item && !voxel)) return GORIO_OK;
  int w = 0;
  for (size_t t = 0; t < total; ++t) {  // offset-major, then item order
    if (slots[t] < 0) continue;
    if (item) item[w] = (int)(t % (size_t)h->ndtc_items);
    if (voxel) voxel[w] = slots[t];
    ++w;
  }
  return GORIO_OK;
}

int gorio_apd_ndt_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel) {
  if (!h || !n_pairs) return GORIO_ERR_INVALID;
  if (!is_ndtc(h)) return fail(h, GORIO_ERR_STATE, "ndt_cuda_get_pairs: the handle is not in NDTCuda mode (gorio_apd_set_method)");
  return voxf_get_pairs(h, capacity, n_pairs, item, voxel);
}

int gorio_apd_set_vgicp_cuda_params(gorio_apd_t* h, int nn_method, double kernel_width, double kernel_max_dist) {
  if (!h) return GORIO_ERR_INVALID;
  if (nn_method != GORIO_VGICP_CUDA_NN_CPU_PARALLEL_KDTREE && nn_method != GORIO_VGICP_CUDA_NN_GPU_BRUTEFORCE && nn_method != GORIO_VGICP_CUDA_NN_GPU_RBF_KERNEL)
    return fail(h, GORIO_ERR_INVALID, "set_vgicp_cuda_params: nn_method must be CPU_PARALLEL_KDTREE (0), GPU_BRUTEFORCE (1) or GPU_RBF_KERNEL (2)");
  if (!std::isfinite(kernel_width) || !std::isfinite(kernel_max_dist)) return fail(h, GORIO_ERR_INVALID, "set_vgicp_cuda_params: kernel_width and kernel_max_dist must be finite");
  if (!(kernel_width > 0.0)) return fail(h, GORIO_ERR_INVALID, "set_vgicp_cuda_params: kernel_width must be positive");
  h->vgc_nn = nn_method;
  h->vgc_width = kernel_width;
  h->vgc_maxd = kernel_max_dist;
  if (is_vgc(h)) h->corr_valid = false;  // pairs of other kept points
  return GORIO_OK;
}

int gorio_apd_get_vgicp_cuda_params(const gorio_apd_t* h, int* nn_method, double* kernel_width, double* kernel_max_dist) {
  if (!h) return GORIO_ERR_INVALID;
  if (nn_method) *nn_method = h->vgc_nn;
  if (kernel_width) *kernel_width = h->vgc_width;
  if (kernel_max_dist) *kernel_max_dist = h->vgc_maxd;
  return GORIO_OK;
}

int gorio_apd_vgicp_cuda_get_points(gorio_apd_t* h, int which, int capacity, int* n, float* cov_raw, int* n_kept, int* kept_index, float* cov) {
  if (!h || !n || !n_kept || (which != 0 && which != 1)) return GORIO_ERR_INVALID;
  if (!is_vgc(h)) return fail(h, GORIO_ERR_STATE, "vgicp_cuda_get_points: the handle is not in FastVGICPCuda mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  const std::shared_ptr<DevCloud>& cp = which == 0 ? h->src : h->tgt;
  DevCloud& c = *cp;
  if (!c.present) return fail(h, GORIO_ERR_STATE, "vgicp_cuda_get_points: that cloud is not set");
  if (vgc_shared_mismatch(h, cp, false)) return fail(h, GORIO_ERR_INVALID, "vgicp_cuda_get_points: the shared cloud's covariances / kept points were made with other settings");
  if (int rc = vgc_cloud_ready(h, c, which == 0 ? "source" : "target")) return rc;
  if (int rc = vgc_filter(h, c)) return rc;
  *n = c.n;
  *n_kept = c.vc_nkept;
  if (capacity < c.n) return GORIO_OK;
  if (cov_raw) HIP_TRY(h, hipMemcpyAsync(cov_raw, c.vc_raw6, sizeof(float) * 6 * c.n, hipMemcpyDeviceToHost, h->stream));
  if (kept_index && c.vc_nkept) HIP_TRY(h, hipMemcpyAsync(kept_index, c.vc_index, sizeof(int) * c.vc_nkept, hipMemcpyDeviceToHost, h->stream));
  if (cov && c.vc_nkept) HIP_TRY(h, hipMemcpyAsync(cov, c.vc_cov6, sizeof(float) * 6 * c.vc_nkept, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_apd_vgicp_cuda_get_voxels(gorio_apd_t* h, int capacity, int* n_voxels, int* coords, int* num_points, float* mean, float* cov) {
  if (!h || !n_voxels) return GORIO_ERR_INVALID;
  if (!is_vgc(h)) return fail(h, GORIO_ERR_STATE, "vgicp_cuda_get_voxels: the handle is not in FastVGICPCuda mode (gorio_apd_set_method)");
  HIP_TRY(h, hipSetDevice(h->device));
  DevCloud& c = *h->tgt;  // there is no source map (VC:257-263)
  if (!c.present) return fail(h, GORIO_ERR_STATE, "vgicp_cuda_get_voxels: no input target set (setInputTarget)");
  if (vgc_shared_mismatch(h, h->tgt, true)) return fail(h, GORIO_ERR_INVALID, "vgicp_cuda_get_voxels: the shared target's covariances / kept points / voxel map were made with other settings");
  if (int rc = vgc_cloud_ready(h, c, "target")) return rc;
  if (int rc = build_vgc_map(h, c)) return rc;
  const int nv = c.vc_map.nv;
  *n_voxels = nv;
  if (capacity < nv || nv == 0 || (!coords && !num_points && !mean && !cov)) return GORIO_OK;
  std::vector<unsigned long long> vkey(nv);
  HIP_TRY(h, hipMemcpyAsync(vkey.data(), c.vc_map.vkey, sizeof(unsigned long long) * nv, hipMemcpyDeviceToHost, h->stream));
  if (num_points) HIP_TRY(h, hipMemcpyAsync(num_points, c.vc_map.num, sizeof(int) * nv, hipMemcpyDeviceToHost, h->stream));
  if (mean) HIP_TRY(h, hipMemcpyAsync(mean, c.vc_map.mean, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost, h->stream));
  if (cov) HIP_TRY(h, hipMemcpyAsync(cov, c.vc_map.cov6, sizeof(float) * 6 * nv, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (coords) c.vc_map.decode_coords(vkey.data(), coords);
  return GORIO_OK;
}

int gorio_apd_vgicp_cuda_get_pairs(gorio_apd_t* h, int capacity, int* n_pairs, int* item, int* voxel) {
  if (!h || !n_pairs) return GORIO_ERR_INVALID;
  if (!is_vgc(h)) return fail(h, GORIO_ERR_STATE, "vgicp_cuda_get_pairs: the handle is not in FastVGICPCuda mode (gorio_apd_set_method)");
  return voxf_get_pairs(h, capacity, n_pairs, item, voxel);
}

int gorio_apd_set_source(gorio_apd_t* h, const float* xyz, const float* label, int n, int stride) {
  if (!h) return GORIO_ERR_INVALID;
  h->corr_valid = false;
  make_private(h, h->src);
  return upload_cloud(h, *h->src, xyz, label, n, stride);
}
int gorio_apd_set_target(gorio_apd_t* h, const float* xyz, const float* label, int n, int stride) {
  if (!h) return GORIO_ERR_INVALID;
  h->corr_valid = false;
  make_private(h, h->tgt);
  return upload_cloud(h, *h->tgt, xyz, label, n, stride);
}
int gorio_apd_set_source_device(gorio_apd_t* h, const float* dx, const float* dy, const float* dz, const float* dl, int n) {
  if (!h) return GORIO_ERR_INVALID;
  h->corr_valid = false;
  make_private(h, h->src);
  return upload_cloud_device(h, *h->src, dx, dy, dz, dl, n);
}
int gorio_apd_set_target_device(gorio_apd_t* h, const float* dx, const float* dy, const float* dz, const float* dl, int n) {
  if (!h) return GORIO_ERR_INVALID;
  h->corr_valid = false;
  make_private(h, h->tgt);
  return upload_cloud_device(h, *h->tgt, dx, dy, dz, dl, n);
}

int gorio_apd_set_clouds_device_batch(gorio_apd_t** handles, int count, const gorio_apd_device_cloud* source, const gorio_apd_device_cloud* target) {
  if (!handles || count <= 0 || (!source && !target)) return GORIO_ERR_INVALID;
  gorio_apd* lead = handles[0];
  if (!lead) return GORIO_ERR_INVALID;
  HIP_TRY(lead, hipSetDevice(lead->device));
  std::vector<CopyJob> jobs;
  jobs.reserve(2 * (size_t)count);
  int max_pad = 0;
  for (int q = 0; q < count; ++q) {
    gorio_apd* h = handles[q];
    if (!h) return fail(lead, GORIO_ERR_INVALID, "null handle in batch");
    if (h->device != lead->device) return fail(lead, GORIO_ERR_INVALID, "all handles of a batch must live on one device");
    for (int side = 0; side < 2; ++side) {
      const gorio_apd_device_cloud* arr = side == 0 ? source : target;
      if (!arr) continue;
      const gorio_apd_device_cloud& in = arr[q];
      if (!in.x || !in.y || !in.z || in.n <= 0) return fail(lead, GORIO_ERR_INVALID, "set_clouds_device_batch: bad cloud arguments");
      make_private(h, side == 0 ? h->src : h->tgt);
      DevCloud& c = side == 0 ? *h->src : *h->tgt;
      int rc = ensure_cloud(h, c, in.n);
      if (rc) {
        if (h != lead) lead->err = h->err;
        return rc;
      }
      jobs.push_back(CopyJob{in.x, in.y, in.z, in.label, c.x, c.y, c.z, c.label, c.p4, in.n, c.n_pad});
      max_pad = std::max(max_pad, c.n_pad);
      c.points_replaced();
      h->corr_valid = false;
    }
  }
  const size_t bytes = sizeof(CopyJob) * jobs.size();
  HIP_TRY(lead, lead->d_copy_jobs.reserve(bytes));
  if (int rc = upload_staged(lead, lead->pin_copy, lead->d_copy_jobs, jobs.data(), bytes)) return rc;
  copy_clouds_kernel<<<dim3(std::min(16, (max_pad + 255) / 256), (unsigned)jobs.size()), 256, 0, lead->stream>>>(static_cast<const CopyJob*>(lead->d_copy_jobs.get()));
  HIP_TRY(lead, hipGetLastError());
  return GORIO_OK;
}

int gorio_apd_clear_source(gorio_apd_t* h) {
  if (!h) return GORIO_ERR_INVALID;
  make_private(h, h->src);
  h->src->cleared(); h->corr_valid = false;  // APD:101-105
  return GORIO_OK;
}
int gorio_apd_clear_target(gorio_apd_t* h) {
  if (!h) return GORIO_ERR_INVALID;
  make_private(h, h->tgt);
  h->tgt->cleared(); h->corr_valid = false;  // APD:107-112
  return GORIO_OK;
}
int gorio_apd_set_target_shared(gorio_apd_t* h, gorio_apd_t* owner) {
  if (!h || !owner) return GORIO_ERR_INVALID;
  if (h->device != owner->device) return fail(h, GORIO_ERR_INVALID, "set_target_shared: both handles must live on one device");
  if (!owner->tgt->present) return fail(h, GORIO_ERR_STATE, "set_target_shared: the owner has no input target");
  {
    const DevCloud& t = *owner->tgt;
    if (cov_rule_differs(h, t))
      return fail(h, GORIO_ERR_INVALID, "set_target_shared: the owner's covariances were estimated with another k_correspondences / regularization than this handle's");
  }
  {
    const DevCloud& t = *owner->tgt;
    if (h->method == GORIO_METHOD_VGICP && t.vm_valid && (t.vm.res != h->voxel_resolution || t.vm_mult != (h->voxel_mode == GORIO_VOXEL_MULTIPLICATIVE)))
      return fail(h, GORIO_ERR_INVALID, "set_target_shared: the owner's voxel map was built with another voxel_resolution / voxel_mode than this handle's");
  }
  if (is_ndtc(h) && owner->tgt->nc_valid && owner->tgt->nc.res != (float)h->voxel_resolution)
    return fail(h, GORIO_ERR_INVALID, "set_target_shared: the owner's NDTCuda voxel map was built with another resolution than this handle's");
  if (is_vgc(h)) {
    const DevCloud& t = *owner->tgt;
    if ((t.vc_raw_valid && !vgc_raw_matches(h, t)) || (t.vc_kept_valid && t.vc_reg != h->params.regularization) || (t.vc_map_valid && t.vc_map.res != (float)h->voxel_resolution))
      return fail(h, GORIO_ERR_INVALID, "set_target_shared: the owner's FastVGICPCuda covariances / kept points / voxel map were made with other settings than this handle's");
  }
  if (is_mp(h) && owner->tgt->mp_valid && (owner->tgt->mp_k != h->params.k_correspondences || owner->tgt->mp_reg != kRegMpBase + h->params.regularization))
    return fail(h, GORIO_ERR_INVALID, "set_target_shared: the owner's FastGICPMultiPoints covariances were made with another k_correspondences or regularization than this handle's");
  h->tgt = owner->tgt;  // points, covariances, search index, voxel map: one copy on the device, alive until the last handle lets go of it
  h->corr_valid = false;
  return GORIO_OK;
}

static int submap_finish(gorio_apd* h, int m, double voxel_leaf, int* n_target);

int gorio_apd_set_target_submap(gorio_apd_t* h, const gorio_apd_keyframe* frames, int count, double voxel_leaf, int* n_target) {
  if (!h || !frames || count <= 0) return GORIO_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  // ---- host staging: finite points of all frames, packed (x, y, z, label); pcl::PassThrough and pcl::VoxelGrid both skip non-finite points
  std::vector<float4> stage;
  std::vector<SubmapFrame> fr(count);
  int max_frame = 0;
  for (int k = 0; k < count; ++k) {
    const gorio_apd_keyframe& f = frames[k];
    if (f.n < 0 || (f.n > 0 && !f.xyz) || f.point_stride_bytes < 12 || (f.point_stride_bytes % 4) != 0 || !f.rel_pose) return fail(h, GORIO_ERR_INVALID, "set_target_submap: bad keyframe arguments");
    fr[k].begin = (int)stage.size();
    const int st = f.point_stride_bytes / 4;
    for (int i = 0; i < f.n; ++i) {
      const float* p = f.xyz + (size_t)i * st;
      if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) continue;
      stage.push_back(make_float4(p[0], p[1], p[2], f.label ? f.label[(size_t)i * st] : 0.0f));
    }
    fr[k].end = (int)stage.size();
    for (int q = 0; q < 12; ++q) fr[k].T[q] = f.rel_pose[q];
    max_frame = std::max(max_frame, fr[k].end - fr[k].begin);
  }
  const int m = (int)stage.size();
  if (m <= 0) return fail(h, GORIO_ERR_INVALID, "set_target_submap: no finite point in any keyframe");
  {
    const size_t cap = (size_t)m + (size_t)m / 8;
    HIP_TRY(h, reserve_group(h->sub_cap, m, cap, h->d_sub_in, cap, h->d_sub_out, cap, h->d_sub_vox, cap));
  }
  HIP_TRY(h, h->d_sub_frames.reserve(count));
  HIP_TRY(h, h->d_sub_bb.reserve(8));
  HIP_TRY(h, hipMemcpyAsync(h->d_sub_in, stage.data(), sizeof(float4) * m, hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->d_sub_frames, fr.data(), sizeof(SubmapFrame) * count, hipMemcpyHostToDevice, h->stream));
  submap_transform_kernel<<<dim3((max_frame + 255) / 256, count), 256, 0, h->stream>>>(h->d_sub_in, h->d_sub_frames, h->d_sub_out);
  HIP_TRY(h, hipGetLastError());
  return submap_finish(h, m, voxel_leaf, n_target);
}

// The second half of a submap assembly, shared by gorio_apd_set_target_submap and gorio_apd_set_target_submap_keyframes
// (csrc/apd_keyframes.hip): the m transformed points in d_sub_out (enqueued on the handle's stream) pass through downsample()
// (SMO:405-415) and become the target.  The stream is drained before a successful return: the callers' pageable tables may die then.
static int submap_finish(gorio_apd* h, int m, double voxel_leaf, int* n_target) {
  const float4* result = h->d_sub_out;
  int n_out = m;
  if (voxel_leaf > 0.0 && h->sub_downsample == GORIO_DOWNSAMPLE_APPROX_VOXELGRID) {  // pcl::ApproximateVoxelGrid (SMO:150-154), cubic, over (x, y, z, label)
    if (m > kAvgMaxPoints) return fail(h, GORIO_ERR_INVALID, "set_target_submap: too many points for the approximate voxel grid");
    const float* base = reinterpret_cast<const float*>(h->d_sub_out.get());
    float* obase = reinterpret_cast<float*>(h->d_sub_vox.get());
    AvgCols in{};
    AvgColsOut out{};
    for (int f = 0; f < 4; ++f) in.c[f] = base + f, out.c[f] = obase + f;
    in.stride = out.stride = 4;
    const float lf = (float)voxel_leaf;
    const float leaf3[3] = {lf, lf, lf};
    const int* d_n_out = nullptr;
    HIP_TRY(h, avg_enqueue(h->stream, h->avg, in, m, 4, leaf3, out, m, &d_n_out));
    HIP_TRY(h, hipMemcpyAsync(&n_out, d_n_out, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // also covers the pageable staging vectors above
    if (n_out < 0) return fail(h, GORIO_ERR_INVALID, "set_target_submap: a cell coordinate of the approximate voxel grid leaves (-2^30, 2^30); the target is unchanged");
    result = h->d_sub_vox;
  } else if (voxel_leaf > 0.0) {  // pcl::VoxelGrid (SMO:145-149)
    unsigned int bb[6];
    vox_bbox_init_kernel<<<1, 64, 0, h->stream>>>(h->d_sub_bb);
    vox_bbox_kernel<<<std::min(256, (m + 255) / 256), 256, 0, h->stream>>>(h->d_sub_out, m, h->d_sub_bb);
    HIP_TRY(h, hipMemcpyAsync(bb, h->d_sub_bb, sizeof(bb), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // also covers the pageable staging vectors above
    auto ord2f_host = [](unsigned int o) {
      const unsigned int u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
      float f;
      std::memcpy(&f, &u, 4);
      return f;
    };
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) { mn[a] = ord2f_host(bb[a]); mx[a] = ord2f_host(bb[3 + a]); }
    VoxGrid g;
    g.inv = 1.0f / (float)voxel_leaf;
    const long long dx = (long long)((mx[0] - mn[0]) * g.inv) + 1, dy = (long long)((mx[1] - mn[1]) * g.inv) + 1, dz = (long long)((mx[2] - mn[2]) * g.inv) + 1;
    // div_b = floor(max inv) - floor(min inv) + 1 can exceed d = (int64)((max - min) inv) + 1 by one per axis, so d's product can pass
    // PCL's test while div_b's overflows the int PCL multiplies it in (undefined there).  Defined here: the
    // product of div_b must fit int32 as well, as ndt_ensure_map requires of its grid; otherwise the input is returned unchanged.
    long long div_b[3] = {1, 1, 1};
    bool fits = dx * dy * dz <= (long long)INT_MAX;  // otherwise: "Leaf size is too small for the input dataset" -> PCL returns the input unchanged
    if (fits) {
      for (int a = 0; a < 3; ++a) {
        g.min_b[a] = (int)std::floor(mn[a] * g.inv);
        div_b[a] = (long long)(int)std::floor(mx[a] * g.inv) - (long long)g.min_b[a] + 1;
      }
      const long long div01 = div_b[0] * div_b[1];  // every factor is at most 2^31 + 1: each product is tested before the next is formed
      fits = div01 <= (long long)INT_MAX && div01 * div_b[2] <= (long long)INT_MAX;
    }
    if (fits) {
      g.div0 = (int)div_b[0];
      g.div01 = (int)(div_b[0] * div_b[1]);
      const int npow2 = sort_padded_size(m);
      HIP_TRY(h, h->d_sub_keys.reserve(npow2));
      const int nblocks = (m + 255) / 256;
      HIP_TRY(h, h->d_sub_counts.reserve(nblocks + 1, nblocks + 1 + nblocks / 8));
      vox_key_kernel<<<(npow2 + 255) / 256, 256, 0, h->stream>>>(h->d_sub_out, m, npow2, g, h->d_sub_keys);
      enqueue_tiled_sort(h->stream, SortKeys{h->d_sub_keys, npow2}, 1, npow2);
      cell_count_kernel<31><<<nblocks, 256, 0, h->stream>>>(h->d_sub_keys, m, h->d_sub_counts);
      block_scan_kernel<<<1, 1024, 0, h->stream>>>(h->d_sub_counts, nblocks);
      vox_centroid_kernel<<<nblocks, 256, 0, h->stream>>>(h->d_sub_keys, h->d_sub_out, m, h->d_sub_counts, h->d_sub_vox);
      HIP_TRY(h, hipGetLastError());
      HIP_TRY(h, hipMemcpyAsync(&n_out, h->d_sub_counts + nblocks, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
      result = h->d_sub_vox;
    }
  }
  make_private(h, h->tgt);
  DevCloud& c = *h->tgt;
  int rc = ensure_cloud(h, c, n_out);
  if (rc) return rc;
  submap_store_kernel<<<(c.n_pad + 255) / 256, 256, 0, h->stream>>>(result, n_out, c.n_pad, c.x, c.y, c.z, c.label, c.p4);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // the staging vectors die with this call
  c.points_replaced();
  h->corr_valid = false;
  if (n_target) *n_target = n_out;
  return GORIO_OK;
}

int gorio_apd_get_target_points(gorio_apd_t* h, float* xyz_out, float* label_out, int n, int point_stride_bytes) {
  if (!h || !xyz_out) return GORIO_ERR_INVALID;
  if (!h->tgt->present || n != h->tgt->n) return fail(h, GORIO_ERR_STATE, "get_target_points: no matching target cloud");
  if (point_stride_bytes < 12 || point_stride_bytes % 4) return fail(h, GORIO_ERR_INVALID, "get_target_points: bad stride");
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<float4> tmp((size_t)n);
  HIP_TRY(h, hipMemcpyAsync(tmp.data(), h->tgt->p4, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  const int st = point_stride_bytes / 4;
  for (int i = 0; i < n; ++i) {
    float* o = xyz_out + (size_t)i * st;
    o[0] = tmp[i].x; o[1] = tmp[i].y; o[2] = tmp[i].z;
    if (label_out) label_out[(size_t)i * st] = tmp[i].w;
  }
  return GORIO_OK;
}

int gorio_apd_set_submap_downsample(gorio_apd_t* h, int method) {
  if (!h) return GORIO_ERR_INVALID;
  if (method != GORIO_DOWNSAMPLE_VOXELGRID && method != GORIO_DOWNSAMPLE_APPROX_VOXELGRID) return fail(h, GORIO_ERR_INVALID, "set_submap_downsample: unknown method");
  h->sub_downsample = method;
  return GORIO_OK;
}
int gorio_apd_get_submap_downsample(const gorio_apd_t* h, int* method) {
  if (!h || !method) return GORIO_ERR_INVALID;
  *method = h->sub_downsample;
  return GORIO_OK;
}

int gorio_apd_swap_source_and_target(gorio_apd_t* h) {
  if (!h) return GORIO_ERR_INVALID;
  std::swap(h->src, h->tgt);  // APD:90-92: clouds, trees and covariances change sides
  h->corr_valid = false;      // APD:96-97
  return GORIO_OK;
}

static int set_covs(gorio_apd* h, DevCloud& c, const double* cov, int n) {
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "set_covariances: " + voxf_name(h) + " takes no per-point double covariances");
  if (is_mp(h)) return fail(h, GORIO_ERR_STATE, "set_covariances: FastGICPMultiPoints takes no per-point double covariances");
  if (n < 0 || (n > 0 && !cov)) return fail(h, GORIO_ERR_INVALID, "set_covariances: bad arguments");
  if (!c.present || n != c.n) {
    // the reference stores the vector whatever its size (APD:138-145) and recomputes the covariances in computeTransformation when the
    // size does not match the cloud (APD:149-154): a mismatching set is therefore the same as none
    c.covs_dropped();
    return GORIO_OK;
  }
  HIP_TRY(h, hipSetDevice(h->device));
  std::vector<double> c6((size_t)n * 6);
  for (int i = 0; i < n; ++i) {
    const double* m = cov + (size_t)i * 16;
    double* o = c6.data() + (size_t)i * 6;
    o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[5]; o[4] = m[6]; o[5] = m[10];
  }
  HIP_TRY(h, hipMemcpyAsync(c.cov6, c6.data(), sizeof(double) * 6 * n, hipMemcpyHostToDevice, h->stream));
  geo_weight_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(c.cov6, c.geo_w, n);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  c.covs_supplied();
  return GORIO_OK;
}

int gorio_apd_set_source_covariances(gorio_apd_t* h, const double* cov, int n) { return h ? set_covs(h, *h->src, cov, n) : GORIO_ERR_INVALID; }
int gorio_apd_set_target_covariances(gorio_apd_t* h, const double* cov, int n) { return h ? set_covs(h, *h->tgt, cov, n) : GORIO_ERR_INVALID; }

static int get_covs(gorio_apd* h, DevCloud& c, double* cov, int n) {
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "get_covariances: " + voxf_name(h) + " holds no per-point double covariances");
  if (is_mp(h)) return fail(h, GORIO_ERR_STATE, "get_covariances: FastGICPMultiPoints holds float covariances (gorio_apd_gicp_mp_get_covariances)");
  const int cnt = c.present ? c.cov_count : 0;
  if (!cov || cnt == 0) return cnt;
  const int m = n < cnt ? n : cnt;
  if (hipSetDevice(h->device) != hipSuccess) return fail(h, GORIO_ERR_NO_DEVICE, "hipSetDevice failed");
  std::vector<double> c6((size_t)m * 6);
  if (hipMemcpyAsync(c6.data(), c.cov6, sizeof(double) * 6 * m, hipMemcpyDeviceToHost, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess)
    return fail(h, GORIO_ERR_NO_DEVICE, "covariance download failed");
  for (int i = 0; i < m; ++i) {
    const double* s = c6.data() + (size_t)i * 6;
    double* o = cov + (size_t)i * 16;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = 0;
    o[4] = s[1]; o[5] = s[3]; o[6] = s[4]; o[7] = 0;
    o[8] = s[2]; o[9] = s[4]; o[10] = s[5]; o[11] = 0;
    o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
  }
  return cnt;
}
int gorio_apd_get_source_covariances(gorio_apd_t* h, double* cov, int n) { return h ? get_covs(h, *h->src, cov, n) : GORIO_ERR_INVALID; }
int gorio_apd_get_target_covariances(gorio_apd_t* h, double* cov, int n) { return h ? get_covs(h, *h->tgt, cov, n) : GORIO_ERR_INVALID; }

int gorio_apd_calculate_covariances(gorio_apd_t* h) {
  if (!h) return GORIO_ERR_INVALID;
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "calculate_covariances: " + voxf_name(h) + " has no per-point double covariances");
  if (is_mp(h)) return fail(h, GORIO_ERR_STATE, "calculate_covariances: FastGICPMultiPoints has no per-point double covariances (gorio_apd_gicp_mp_get_covariances makes its float ones)");
  HIP_TRY(h, hipSetDevice(h->device));
  const gorio_apd_params& p = h->params;
  std::vector<std::pair<gorio_apd*, DevCloud*>> todo;
  for (DevCloud* c : {h->src.get(), h->tgt.get()}) {
    if (c->present && c->cov_count != c->n) {
      if (c->n < p.k_correspondences) return fail(h, GORIO_ERR_INVALID, "cloud has fewer points than k_correspondences (undefined in the reference, APD:366-369)");
      todo.emplace_back(h, c);
    }
  }
  int rc = GORIO_OK;
  if (p.search == GORIO_SEARCH_PRUNED && !todo.empty()) {  // indices of both clouds in one call (kd chunk size by the pair, run_index_build)
    std::vector<std::pair<gorio_apd*, DevCloud*>> both;
    for (DevCloud* c : {h->src.get(), h->tgt.get()})
      if (c->present) both.emplace_back(h, c);
    rc = run_index_build(h, both);
    if (rc) return rc;
  }
  rc = run_covariances(h, todo);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  resolve_stage_events(h);
  return GORIO_OK;
}

int gorio_apd_get_knn_indices(gorio_apd_t* h, int which, int* idx, int n_times_k) {
  if (!h || !idx) return GORIO_ERR_INVALID;
  DevCloud& c = which == 0 ? *h->src : *h->tgt;
  if (!c.present || !c.knn || !c.knn_valid || c.cov_count != c.n) return fail(h, GORIO_ERR_STATE, "no k-NN result held for this cloud (set params.keep_knn_indices before the covariances are computed)");
  if (n_times_k != c.n * c.knn_k) return fail(h, GORIO_ERR_INVALID, "get_knn_indices: size mismatch");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(idx, c.knn, sizeof(int) * (size_t)n_times_k, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_apd_align(gorio_apd_t* h, const float guess[16], float T_out[16], double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  if (!h) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_GICP_OMP) return gomp_align(h, guess, T_out, H_out, converged, nr_iterations, n_linearize);
  if (h->method == GORIO_METHOD_ICP) return icp_align(h, guess, T_out, H_out, converged, nr_iterations, n_linearize);
  if (is_mp(h)) return mp_align(h, guess, T_out, H_out, converged, nr_iterations, n_linearize);
  gorio_apd* hs[1] = {h};
  return align_impl(hs, 1, guess, T_out, H_out, converged, nr_iterations, n_linearize);
}

int gorio_apd_align_batch(gorio_apd_t** handles, int count, const float* guesses, float* T_out, double* H_out, int* converged, int* nr_iterations, int* n_linearize) {
  return align_impl(handles, count, guesses, T_out, H_out, converged, nr_iterations, n_linearize);
}

int gorio_apd_linearize(gorio_apd_t* h, const double T[16], double* H, double* b, double* error) {
  if (!h || !T) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_GICP_OMP) return fail(h, GORIO_ERR_UNSUPPORTED, "linearize: GICP_OMP has no Gauss-Newton linearisation (gorio_apd_gicp_omp_update / _evaluate)");
  if (h->method == GORIO_METHOD_ICP) return fail(h, GORIO_ERR_UNSUPPORTED, "linearize: ICP has no Gauss-Newton linearisation (gorio_apd_icp_step)");
  if (is_mp(h)) return fail(h, GORIO_ERR_UNSUPPORTED, "linearize: FastGICPMultiPoints linearises at a float pose through gorio_apd_gicp_mp_pass");
  return lsq_linearize(h, T, H, b, error);
}

int gorio_apd_compute_error(gorio_apd_t* h, const double T[16], double* error) {
  if (!h || !T || !error) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_GICP_OMP) return fail(h, GORIO_ERR_UNSUPPORTED, "compute_error: GICP_OMP evaluates its functor through gorio_apd_gicp_omp_evaluate");
  if (h->method == GORIO_METHOD_ICP) return fail(h, GORIO_ERR_UNSUPPORTED, "compute_error: ICP has no weighted error (gorio_apd_icp_diag gives the mean squared distance)");
  if (is_mp(h)) return fail(h, GORIO_ERR_UNSUPPORTED, "compute_error: FastGICPMultiPoints has no error function (its solver takes full Gauss-Newton steps)");
  return lsq_compute_error(h, T, error);
}

int gorio_apd_get_correspondences(gorio_apd_t* h, int* corr, float* sq_dist, int n) {
  if (!h) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_VGICP) return fail(h, GORIO_ERR_STATE, "get_correspondences: FastVGICP pairs points with voxels, not with target points (gorio_apd_get_voxel_correspondences)");
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "get_correspondences: " + voxf_name(h) + " pairs items with voxels, not with target points (gorio_apd_ndt_cuda_get_pairs / gorio_apd_vgicp_cuda_get_pairs)");
  if (is_mp(h)) return fail(h, GORIO_ERR_UNSUPPORTED, "get_correspondences: FastGICPMultiPoints pairs a point with a neighbourhood, not with one target point (gorio_apd_gicp_mp_get_neighbors)");
  if (!h->corr_valid) return fail(h, GORIO_ERR_STATE, "no correspondences held");
  if (n != h->src->n) return fail(h, GORIO_ERR_INVALID, "get_correspondences: size mismatch");
  HIP_TRY(h, hipSetDevice(h->device));
  if (corr) HIP_TRY(h, hipMemcpyAsync(corr, h->corr, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
  if (sq_dist) HIP_TRY(h, hipMemcpyAsync(sq_dist, h->sqd, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GORIO_OK;
}

int gorio_apd_get_mahalanobis(gorio_apd_t* h, double* maha, int n) {
  if (!h || !maha) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_VGICP) return fail(h, GORIO_ERR_STATE, "get_mahalanobis: FastVGICP holds one matrix per (point, voxel) pair, not per point");
  if (h->method == GORIO_METHOD_ICP) return fail(h, GORIO_ERR_STATE, "get_mahalanobis: ICP holds no Mahalanobis matrices");
  if (is_mp(h)) return fail(h, GORIO_ERR_UNSUPPORTED, "get_mahalanobis: FastGICPMultiPoints holds no Mahalanobis matrices (they are recomputed per point and pass)");
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "get_mahalanobis: " + voxf_name(h) + " holds no Mahalanobis matrices (they are recomputed per pair)");
  if (!h->corr_valid || !h->omega_valid) return fail(h, GORIO_ERR_STATE, "no Mahalanobis matrices held (a Gauss-Newton align does not materialise them: call gorio_apd_linearize)");
  if (n != h->src->n) return fail(h, GORIO_ERR_INVALID, "get_mahalanobis: size mismatch");
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->method == GORIO_METHOD_GICP_OMP) {  // mahalanobis_ (GOH:304): the stored floats widened, zero for unpaired points
    if (h->gomp_pairs < 0 || h->gomp_cap < n) return fail(h, GORIO_ERR_STATE, "no Mahalanobis matrices held");
    std::vector<float> m9((size_t)n * 9);
    std::vector<int> cr(n);
    HIP_TRY(h, hipMemcpyAsync(m9.data(), h->gomp_maha, sizeof(float) * 9 * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(cr.data(), h->corr, sizeof(int) * n, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
      double* o = maha + (size_t)i * 16;
      for (int q = 0; q < 16; ++q) o[q] = 0.0;
      if (cr[i] < 0) continue;
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = (double)m9[(size_t)i * 9 + r * 3 + c];
    }
    return GORIO_OK;
  }
  std::vector<double> o6((size_t)n * 6);
  HIP_TRY(h, hipMemcpyAsync(o6.data(), h->omega6, sizeof(double) * 6 * n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) {
    const double* s = o6.data() + (size_t)i * 6;
    double* o = maha + (size_t)i * 16;
    o[0] = s[0]; o[1] = s[1]; o[2] = s[2]; o[3] = 0;
    o[4] = s[1]; o[5] = s[3]; o[6] = s[4]; o[7] = 0;
    o[8] = s[2]; o[9] = s[4]; o[10] = s[5]; o[11] = 0;
    o[12] = 0; o[13] = 0; o[14] = 0; o[15] = 0;
  }
  return GORIO_OK;
}

int gorio_apd_transform_source(gorio_apd_t* h, const float T[16], float* xyz_out, int n, int stride) {
  if (!h || !T || !xyz_out) return GORIO_ERR_INVALID;
  if (!h->src->present || n != h->src->n) return fail(h, GORIO_ERR_STATE, "transform_source: no matching source cloud");
  if (stride < 12 || stride % 4) return fail(h, GORIO_ERR_INVALID, "transform_source: bad stride");
  HIP_TRY(h, hipSetDevice(h->device));
  DevBuf<float> d_out;  // freed on every way out
  HIP_TRY(h, d_out.reserve(3 * (size_t)n));
  TfArg tf;
  for (int i = 0; i < 12; ++i) tf.m[i] = T[i];
  transform_cloud_kernel<<<(n + 255) / 256, 256, 0, h->stream>>>(h->src->x, h->src->y, h->src->z, n, tf, d_out);
  std::vector<float> tmp((size_t)n * 3);
  hipError_t e = hipMemcpyAsync(tmp.data(), d_out, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return fail(h, GORIO_ERR_NO_DEVICE, hipGetErrorString(e));
  const int st = stride / 4;
  for (int i = 0; i < n; ++i) {
    float* o = xyz_out + (size_t)i * st;
    o[0] = tmp[3 * (size_t)i]; o[1] = tmp[3 * (size_t)i + 1]; o[2] = tmp[3 * (size_t)i + 2];
  }
  return GORIO_OK;
}

int gorio_apd_fitness_score(gorio_apd_t* h, const float T[16], double max_range, double inlier_dist, double* score, double* inlier_fraction) {
  if (!h || !T || !score) return GORIO_ERR_INVALID;
  if (!h->src->present || !h->tgt->present) return fail(h, GORIO_ERR_STATE, "fitness_score: clouds not set");
  if ((h->comm || h->shard_only) && h->comm_world > 1)
    return fail(h, GORIO_ERR_STATE, "fitness_score: this handle searches only its rank's share of the source (gorio_apd_comm_init); score the pose on an unsharded handle");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = ensure_points(h, h->src->n);
  if (rc) return rc;
  const bool pruned = h->params.search == GORIO_SEARCH_PRUNED;
  if (pruned) {  // the same exact branch-and-bound search as the registration (matters for 100 k-point maps)
    std::vector<std::pair<gorio_apd*, DevCloud*>> both = {{h, h->src.get()}, {h, h->tgt.get()}};
    rc = run_index_build(h, both);
    if (rc) return rc;
  }
  rc = single_desc(h);
  if (rc) return rc;
  PairState s;
  double Td[16];
  for (int i = 0; i < 16; ++i) Td[i] = (double)T[i];
  init_state(s, Td);
  for (int i = 0; i < 12; ++i) s.Tf[i] = T[i];
  const int nbx = (h->src->n + 255) / 256;
  HIP_TRY(h, h->d_fit.reserve((size_t)nbx * 3));
  HIP_TRY(h, hipMemcpyAsync(h->d_state, &s, sizeof(s), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->best_key, 0xff, sizeof(unsigned long long) * h->src->n, h->stream));
  PairDesc d;
  fill_desc(h, d, h->d_state, (h->src->n + 63) / 64);
  if (!(inlier_dist > 0.0)) inlier_dist = 0.5;  // const double max_correspondence_dist = 0.5, SMO:677
  const double inlier_sq = inlier_dist * inlier_dist;
  if (pruned) {
    const int waves = (h->src->n + 63) / 64;
    launch_pruned(dim3((roundup(h->src->n, 512) + 255) / 256, fitness_splits(waves), 1), h->stream, h->d_desc, fitness_bound(max_range, inlier_sq), 0);
  } else {
    nn_search_kernel<<<dim3(nbx, d.nn_splits, 1), 256, 0, h->stream>>>(h->d_desc);
  }
  fitness_kernel<<<nbx, 256, 0, h->stream>>>(h->best_key, h->src->n, max_range, inlier_sq, h->d_fit);
  HIP_TRY(h, hipGetLastError());
  std::vector<double> part((size_t)nbx * 3);
  HIP_TRY(h, hipMemcpyAsync(part.data(), h->d_fit, sizeof(double) * part.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->corr_valid = false;
  double out[3] = {0.0, 0.0, 0.0};
  for (int bk = 0; bk < nbx; ++bk)
    for (int q = 0; q < 3; ++q) out[q] += part[(size_t)bk * 3 + q];
  *score = out[1] > 0 ? out[0] / out[1] : DBL_MAX;  // pcl: returns max double when no correspondence is in range
  if (inlier_fraction) *inlier_fraction = out[2] / (double)h->src->n;
  return GORIO_OK;
}

int gorio_apd_fitness_score_batch(gorio_apd_t** handles, int count, const float* T, double max_range, double inlier_dist, double* score, double* inlier_fraction) {
  if (count == 0) return GORIO_OK;
  if (!handles || count < 0 || !T || !score) return GORIO_ERR_INVALID;
  gorio_apd* lead = handles[0];
  if (!lead) return GORIO_ERR_INVALID;
  // every check comes before the first change to any handle: an error leaves them all as they were
  {
    std::unordered_set<gorio_apd*> distinct;
    for (int q = 0; q < count; ++q) {
      gorio_apd* h = handles[q];
      const std::string at = "fitness_score_batch: handles[" + std::to_string(q) + "]: ";
      if (!h) return fail(lead, GORIO_ERR_INVALID, at + "null handle");
      if (h->device != lead->device) return fail(lead, GORIO_ERR_INVALID, at + "all handles of a batch must live on one device");
      if (!distinct.insert(h).second) return fail(lead, GORIO_ERR_INVALID, at + "the same handle appears twice in a batch (its buffers would be raced on)");
      if (!h->src->present || !h->tgt->present) return fail(lead, GORIO_ERR_STATE, at + "clouds not set");
      if ((h->comm || h->shard_only) && h->comm_world > 1)
        return fail(lead, GORIO_ERR_STATE, at + "this handle searches only its rank's share of the source (gorio_apd_comm_init); score the pose on an unsharded handle");
    }
  }
  HIP_TRY(lead, hipSetDevice(lead->device));
  // pairs in descriptor order: the pruned-search ones first, then the brute-force ones (each handle searches as its single call would)
  std::vector<int> order;
  for (int pass = 0; pass < 2; ++pass)
    for (int q = 0; q < count; ++q)
      if ((handles[q]->params.search == GORIO_SEARCH_PRUNED) == (pass == 0)) order.push_back(q);
  int n_pruned = 0;
  long total_src_waves = 0, pruned_waves = 0;
  int max_n = 1, max_nbx = 1, max_spad_pruned = 512, max_nbx_brute = 1, max_splits_brute = 1;
  std::vector<std::pair<gorio_apd*, DevCloud*>> all;
  for (int q = 0; q < count; ++q) {
    gorio_apd* h = handles[q];
    int rc = ensure_points(h, h->src->n);
    if (rc) {
      if (h != lead) lead->err = "fitness_score_batch: handles[" + std::to_string(q) + "]: " + h->err;
      return rc;
    }
    const int waves = (h->src->n + 63) / 64;
    total_src_waves += waves;
    max_n = std::max(max_n, h->src->n);
    max_nbx = std::max(max_nbx, (h->src->n + 255) / 256);
    if (h->params.search == GORIO_SEARCH_PRUNED) {
      ++n_pruned;
      pruned_waves += waves;
      max_spad_pruned = std::max(max_spad_pruned, roundup(h->src->n, 512));
      all.emplace_back(h, h->src.get());
      all.emplace_back(h, h->tgt.get());
    }
  }
  if (!all.empty()) {  // ONE index build for every cloud that lacks one; a target shared by several handles is one cloud
    int rc = run_index_build(lead, all);
    if (rc) return rc;
  }
  if (int rc = ensure_batch(lead, count)) return rc;
  std::vector<PairDesc> descs(count);
  std::vector<PairState> states(count);
  for (int k = 0; k < count; ++k) {
    const int q = order[k];
    gorio_apd* h = handles[q];
    double Td[16];
    for (int i = 0; i < 16; ++i) Td[i] = (double)T[(size_t)q * 16 + i];
    init_state(states[k], Td);
    for (int i = 0; i < 12; ++i) states[k].Tf[i] = T[(size_t)q * 16 + i];
    fill_desc(h, descs[k], h->d_state, total_src_waves);
    if (k >= n_pruned) {
      max_nbx_brute = std::max(max_nbx_brute, descs[k].nblk);
      max_splits_brute = std::max(max_splits_brute, descs[k].nn_splits);
    }
  }
  const size_t n_part = (size_t)count * max_nbx * 3;
  HIP_TRY(lead, lead->d_fit.reserve(n_part));
  if (int rc = upload_staged(lead, lead->pin_desc, lead->d_desc, descs.data(), sizeof(PairDesc) * count)) return rc;
  if (int rc = upload_staged(lead, lead->pin_states, lead->d_states_batch, states.data(), sizeof(PairState) * count)) return rc;
  scatter_states_kernel<<<count, 64, 0, lead->stream>>>(lead->d_desc, lead->d_states_batch);
  arm_keys_kernel<<<dim3(std::min(64, (max_n + 255) / 256), count), 256, 0, lead->stream>>>(lead->d_desc);
  if (!(inlier_dist > 0.0)) inlier_dist = 0.5;  // const double max_correspondence_dist = 0.5, SMO:677
  const double inlier_sq = inlier_dist * inlier_dist;
  if (n_pruned > 0)
    launch_pruned(dim3(max_spad_pruned / 256, fitness_splits(pruned_waves), n_pruned), lead->stream, lead->d_desc, fitness_bound(max_range, inlier_sq), 0);
  if (n_pruned < count) nn_search_kernel<<<dim3(max_nbx_brute, max_splits_brute, count - n_pruned), 256, 0, lead->stream>>>(lead->d_desc + n_pruned);
  fitness_batch_kernel<<<dim3(max_nbx, count), 256, 0, lead->stream>>>(lead->d_desc, max_range, inlier_sq, lead->d_fit);
  HIP_TRY(lead, hipGetLastError());
  std::vector<double> part(n_part);
  HIP_TRY(lead, hipMemcpyAsync(part.data(), lead->d_fit, sizeof(double) * n_part, hipMemcpyDeviceToHost, lead->stream));
  HIP_TRY(lead, hipStreamSynchronize(lead->stream));
  for (int k = 0; k < count; ++k) {
    const int q = order[k];
    gorio_apd* h = handles[q];
    h->corr_valid = false;
    double out[3] = {0.0, 0.0, 0.0};
    const double* p = part.data() + (size_t)k * max_nbx * 3;
    for (int bk = 0; bk < descs[k].nblk; ++bk)  // block order, as gorio_apd_fitness_score adds them
      for (int c = 0; c < 3; ++c) out[c] += p[(size_t)bk * 3 + c];
    score[q] = out[1] > 0 ? out[0] / out[1] : DBL_MAX;
    if (inlier_fraction) inlier_fraction[q] = out[2] / (double)h->src->n;
  }
  return GORIO_OK;
}

int gorio_comm_get_unique_id(char id[128]) {
  if (!id) return GORIO_ERR_INVALID;
  Rccl& R = rccl();
  if (!R.ok) return GORIO_ERR_NO_DEVICE;
  ncclUniqueId u;
  if (R.GetUniqueId(&u) != ncclSuccess) return GORIO_ERR_NO_DEVICE;
  static_assert(sizeof(u) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id, &u, 128);
  return GORIO_OK;
}

int gorio_apd_comm_init(gorio_apd_t* h, int world_size, int rank, const char id[128]) {
  if (!h || !id || world_size < 1 || rank < 0 || rank >= world_size) return GORIO_ERR_INVALID;
  if (h->method == GORIO_METHOD_VGICP) return fail(h, GORIO_ERR_STATE, "comm_init: FastVGICP has no sharded-source mode");
  if (h->method == GORIO_METHOD_ICP) return fail(h, GORIO_ERR_STATE, "comm_init: ICP has no sharded-source mode");
  if (is_mp(h)) return fail(h, GORIO_ERR_STATE, "comm_init: FastGICPMultiPoints has no sharded-source mode");
  if (is_voxf(h)) return fail(h, GORIO_ERR_STATE, "comm_init: " + voxf_name(h) + " has no sharded-source mode");
  Rccl& R = rccl();
  if (!R.ok) return fail(h, GORIO_ERR_NO_DEVICE, "librccl could not be loaded");
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->comm) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    R.CommDestroy(h->comm);
    h->comm = nullptr;
  }
  ncclUniqueId u;
  std::memcpy(&u, id, 128);
  NCCL_TRY(h, R.CommInitRank(&h->comm, world_size, u, rank));
  h->comm_world = world_size;
  h->comm_rank = rank;
  h->shard_only = false;
  h->corr_valid = false;
  return GORIO_OK;
}

int gorio_apd_comm_info(gorio_apd_t* h, int* world_size, int* rank, long long* allreduce_count) {
  if (!h) return GORIO_ERR_INVALID;
  if (!h->comm) return fail(h, GORIO_ERR_STATE, "comm_info: the handle has no communicator");
  Rccl& R = rccl();
  int w = 0, r = 0;
  if (!R.CommCount || !R.CommUserRank) return fail(h, GORIO_ERR_NO_DEVICE, "librccl lacks ncclCommCount / ncclCommUserRank");
  NCCL_TRY(h, R.CommCount(h->comm, &w));  // what RCCL itself says, not what the caller passed to comm_init
  NCCL_TRY(h, R.CommUserRank(h->comm, &r));
  if (world_size) *world_size = w;
  if (rank) *rank = r;
  if (allreduce_count) *allreduce_count = h->allreduce_count;
  return GORIO_OK;
}

int gorio_apd_debug_set_shard(gorio_apd_t* h, int world_size, int rank) {
  if (!h || world_size < 1 || rank < 0 || rank >= world_size) return GORIO_ERR_INVALID;
  if (h->comm) return fail(h, GORIO_ERR_STATE, "debug_set_shard: the handle has a communicator");
  if (h->method == GORIO_METHOD_ICP && world_size > 1) return fail(h, GORIO_ERR_STATE, "debug_set_shard: ICP has no sharded-source mode");
  if (is_mp(h) && world_size > 1) return fail(h, GORIO_ERR_STATE, "debug_set_shard: FastGICPMultiPoints has no sharded-source mode");
  if (is_voxf(h) && world_size > 1) return fail(h, GORIO_ERR_STATE, "debug_set_shard: " + voxf_name(h) + " has no sharded-source mode");
  h->comm_world = world_size;
  h->comm_rank = rank;
  h->shard_only = world_size > 1;
  h->corr_valid = false;
  return GORIO_OK;
}

int gorio_apd_debug_set_schedule(gorio_apd_t* h, int fuse_step, int plan_search) {
  if (!h) return GORIO_ERR_INVALID;
  h->fuse_step = h->fuse_supported && fuse_step != 0;
  h->plan_search = plan_search != 0;
  return GORIO_OK;
}

int gorio_apd_debug_knn_redo_groups(gorio_apd_t* h, int* groups) {
  if (!h || !groups) return GORIO_ERR_INVALID;
  if (!h->d_redo_list) return fail(h, GORIO_ERR_STATE, "debug_knn_redo_groups: this handle has led no k-NN covariance estimation by selection (pruned search, k <= 20)");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  unsigned int count = 0;
  HIP_TRY(h, hipMemcpy(&count, h->d_redo_list, sizeof(count), hipMemcpyDeviceToHost));
  *groups = (int)count;
  return GORIO_OK;
}

int gorio_apd_debug_get_index(gorio_apd_t* h, int which, int sizes[6], float* sxyz, int* orig, float* tbox, float* sbox, float* bbox) {
  if (!h || !sizes) return GORIO_ERR_INVALID;
  DevCloud& c = which == 0 ? *h->src : *h->tgt;
  if (!c.present || !c.idx_valid) return fail(h, GORIO_ERR_STATE, "debug_get_index: no search index held for this cloud (pruned search, after the covariances or a linearisation)");
  const SearchIndex ix = c.index_view();
  const int n_blk = (ix.n_super + 63) / 64;
  sizes[0] = ix.n; sizes[1] = ix.n_spad; sizes[2] = ix.n_tiles; sizes[3] = ix.n_super; sizes[4] = n_blk; sizes[5] = c.idx_chunk;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (sxyz) {
    HIP_TRY(h, hipMemcpy(sxyz, ix.sx, sizeof(float) * ix.n_spad, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(sxyz + ix.n_spad, ix.sy, sizeof(float) * ix.n_spad, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(sxyz + 2 * (size_t)ix.n_spad, ix.sz, sizeof(float) * ix.n_spad, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(sxyz + 3 * (size_t)ix.n_spad, ix.s4, sizeof(float4) * ix.n_spad, hipMemcpyDeviceToHost));
  }
  if (orig) HIP_TRY(h, hipMemcpy(orig, ix.orig, sizeof(int) * ix.n_spad, hipMemcpyDeviceToHost));
  if (tbox) HIP_TRY(h, hipMemcpy(tbox, ix.tbox, sizeof(float) * 8 * ix.n_tiles, hipMemcpyDeviceToHost));
  if (sbox) HIP_TRY(h, hipMemcpy(sbox, ix.sbox, sizeof(float) * 8 * ix.n_super, hipMemcpyDeviceToHost));
  if (bbox) HIP_TRY(h, hipMemcpy(bbox, ix.bbox, sizeof(float) * 8 * n_blk, hipMemcpyDeviceToHost));
  return GORIO_OK;
}

int gorio_apd_comm_destroy(gorio_apd_t* h) {
  if (!h) return GORIO_ERR_INVALID;
  if (h->comm) {
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (rccl().ok) rccl().CommDestroy(h->comm);
    h->comm = nullptr;
  }
  h->comm_world = 1;
  h->comm_rank = 0;
  h->shard_only = false;
  h->corr_valid = false;
  return GORIO_OK;
}

int gorio_apd_set_profiling(gorio_apd_t* h, int enable) {
  if (!h) return GORIO_ERR_INVALID;
  h->profiling = enable != 0;
  for (int i = 0; i < 8; ++i) { h->stage_s[i] = 0; h->stage_n[i] = 0; }
  return GORIO_OK;
}

int gorio_apd_get_stage_times(gorio_apd_t* h, double seconds[8], int counts[8]) {
  if (!h) return GORIO_ERR_INVALID;
  for (int i = 0; i < 8; ++i) {
    if (seconds) seconds[i] = h->stage_s[i];
    if (counts) counts[i] = h->stage_n[i];
  }
  return GORIO_OK;
}

}  // extern "C"

#ifdef GORIO_STATS
extern "C" int gorio_debug_search_stats(unsigned long long out[24], int reset) {
  static std::vector<unsigned long long> all(1024 * 24);
  if (hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(gorio::g_search_stats), sizeof(unsigned long long) * 1024 * 24) != hipSuccess) return -1;
  for (int k = 0; k < 24; ++k) {
    out[k] = 0;
    for (int r = 0; r < 1024; ++r) out[k] = (k == 2 && false) ? std::max(out[k], all[(size_t)r * 24 + k]) : out[k] + all[(size_t)r * 24 + k];
  }
  if (reset) {
    std::fill(all.begin(), all.end(), 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(gorio::g_search_stats), all.data(), sizeof(unsigned long long) * 1024 * 24) != hipSuccess) return -1;
  }
  return 0;
}
#endif

// the preprocessing ABI (include/gorio_prep.h) keeps kernels and host side together, like apd_sc.hip and apd_ground.hip; its host side
// works through a private registration handle, hence down here
#include "../../include/gorio_prep.h"
#include "apd_prep.hip"
#include "apd_scan.hip"
#include "../../include/gorio_keyframes.h"
#include "apd_keyframes.hip"
#include "../../include/gorio_map.h"
#include "apd_map.hip"
#include "apd_batch_rounds.hip"
#include "apd_gicp_omp.hip"
#include "apd_icp.hip"
#include "../../include/gorio_search.h"
#include "apd_search.hip"
#include "apd_ndt_radius.hip"
#include "apd_gicp_mp.hip"
