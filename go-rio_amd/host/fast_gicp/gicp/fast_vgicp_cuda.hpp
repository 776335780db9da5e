// Drop-in for the reference's fast_gicp/gicp/fast_vgicp_cuda.hpp (VH:21-85) backed by the MI355X library libgorio_amd.so: the class a
// fast_gicp build on an NVIDIA box calls VGICP_CUDA (pygicp, gicp_test.cpp) and select_registration_method calls FAST_VGICP_CUDA
// (REG:52-61), here as GORIO_METHOD_VGICP_CUDA of the registration handle.  Same namespace, class name, template parameters, Ptr typedefs,
// setters and overrides as the reference; header-only; no CPU fallback (the constructor throws std::runtime_error when no HIP device is
// usable).  What the class computes is defined in include/gorio_apd.h.
//
// Like FastVGICP and NDTCuda it is a FastGICP whose handle runs another method: the device handle, the cloud uploads, the LsqRegistration
// settings and align / linearize / compute_error / fitness through the C ABI exist once, in fast_apdgicp.hpp.  The covariance setters and
// getters FastGICP adds to the reference's surface throw here (GORIO_ERR_STATE): this method's covariances are floats on the device.
//
// Member -> ABI:  setNearestNeighborSearchMethod / setKernelWidth -> gorio_apd_set_vgicp_cuda_params; setResolution /
// setNeighborSearchMethod -> gorio_apd_set_method(GORIO_METHOD_VGICP_CUDA, resolution, method, -), its radius ->
// gorio_apd_set_ndt_cuda_params; setRegularizationMethod -> params.regularization; setCorrespondenceRandomness is the no-op it is in the
// reference (VI:38: k stays 20); swapSourceAndTarget -> gorio_apd_swap_source_and_target (clouds, covariances and kept points change
// sides, the new target's map is built: VC:97-107).  Covariances, kept points and the map are made at the first linearise / align.
// Deviation: setResolution after a map was built rebuilds it (VI:41-43, 145; VC:257-263).
#ifndef FAST_GICP_FAST_VGICP_CUDA_HPP
#define FAST_GICP_FAST_VGICP_CUDA_HPP

#include <fast_gicp/gicp/fast_gicp.hpp>
#include <fast_gicp/gicp/gicp_settings.hpp>

namespace fast_gicp {

enum class NearestNeighborMethod { CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL };  // VH:21, the order of gorio_vgicp_cuda_nn

template <typename PointSource, typename PointTarget>
class FastVGICPCuda : public FastGICP<PointSource, PointTarget> {
public:
  using Scalar = float;
  using Matrix4 = typename pcl::Registration<PointSource, PointTarget, Scalar>::Matrix4;

  using PointCloudSource = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudSource;
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;

  using PointCloudTarget = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudTarget;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;

#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastVGICPCuda<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastVGICPCuda<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastVGICPCuda<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastVGICPCuda<PointSource, PointTarget>>;
#endif

protected:
  using pcl::Registration<PointSource, PointTarget, Scalar>::reg_name_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::input_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::target_;
  using Base = FastGICP<PointSource, PointTarget>;

public:
  explicit FastVGICPCuda(int device = 0) : Base(device) {  // VI:22-32: k 20, CPU_PARALLEL_KDTREE, kernel 0.5 / 3.0, PLANE, DIRECT1, resolution 1.0
    reg_name_ = "FastVGICPCuda";
  }
  virtual ~FastVGICPCuda() override {}

  void setCorrespondenceRandomness(int) {}                             // VI:38: empty in the reference, k stays 20
  void setResolution(double resolution) { resolution_ = resolution; }  // VI:41-43
  void setKernelWidth(double kernel_width, double max_dist = -1.0) {   // VI:46-51
    kernel_width_ = kernel_width;
    kernel_max_dist_ = max_dist <= 0.0 ? kernel_width * 5.0 : max_dist;
  }
  void setRegularizationMethod(RegularizationMethod method) { Base::setRegularizationMethod(method); }  // VI:54-56
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) {                     // VI:59-61
    search_method_ = method;
    radius_ = radius;
  }
  void setNearestNeighborSearchMethod(NearestNeighborMethod method) { neighbor_method_ = method; }      // VI:64-66

  virtual void swapSourceAndTarget() override { Base::swapSourceAndTarget(); }  // VI:69-72
  virtual void clearSource() override { Base::clearSource(); }                  // VI:75-77
  virtual void clearTarget() override { Base::clearTarget(); }                  // VI:80-82
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) override { Base::setInputSource(cloud); }  // VI:85-111 (the same pointer: no-op)
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override { Base::setInputTarget(cloud); }  // VI:114-140

  // ---- extras the other drop-ins have (no counterpart in the reference)
  // regs[i]->align(outputs[i], guesses[i]) for every i through ONE gorio_apd_align_batch; every result is bit for bit the single align's
  static void alignBatch(const std::vector<FastVGICPCuda*>& regs, const std::vector<Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    std::vector<FastAPDGICP<PointSource, PointTarget>*> back(regs.size());
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("FastVGICPCuda::alignBatch: null object");
      regs[i]->push_settings();
      back[i] = regs[i]->backend_.get();
    }
    FastAPDGICP<PointSource, PointTarget>::alignBatch(back, guesses, outputs);
    for (FastVGICPCuda* r : regs) r->pull_result();
  }
  static std::vector<double> getFitnessScoreBatch(const std::vector<FastVGICPCuda*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<FastAPDGICP<PointSource, PointTarget>*> back(regs.size());
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("FastVGICPCuda::getFitnessScoreBatch: null object");
      regs[i]->backend_->set_final(regs[i]->final_transformation_);
      back[i] = regs[i]->backend_.get();
    }
    return FastAPDGICP<PointSource, PointTarget>::getFitnessScoreBatch(back, max_range);
  }
  // one target, and ONE set of covariances, kept points and voxel map, for many objects (gorio_apd_set_target_shared)
  void setInputTargetShared(FastVGICPCuda& owner) {
    this->push_settings();
    this->backend_->setInputTargetShared(*owner.backend_);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(owner.target_);
    this->lazy_tree_->defer(owner.target_);
  }
  // the frame a gorio::ScanPreprocessor just produced as source / target: no upload (gorio_apd_set_source_from_scan)
  template <typename Preprocessor>
  void setInputSourceFromScan(Preprocessor& pre) {
    this->backend_->setInputSourceFromScan(pre);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputSource(pre.last_scan());
  }
  template <typename Preprocessor>
  void setInputTargetFromScan(Preprocessor& pre) {
    this->backend_->setInputTargetFromScan(pre);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(pre.last_scan());
    this->lazy_tree_->defer(pre.last_scan());
  }
  // setInputSourceKeyframe / setInputTargetKeyframe: FastGICP's, with this class' method selected first
  // parity hooks: voxels of the target map (gorio_apd_vgicp_cuda_get_voxels), points of the source (0) / target (1) the filter keeps
  int voxelCount() {
    push_method();
    int nv = 0;
    this->check(gorio_apd_vgicp_cuda_get_voxels(this->handle(), 0, &nv, nullptr, nullptr, nullptr, nullptr));
    return nv;
  }
  int keptCount(int which) {
    push_method();
    int n = 0, kept = 0;
    this->check(gorio_apd_vgicp_cuda_get_points(this->handle(), which, 0, &n, nullptr, &kept, nullptr, nullptr));
    return kept;
  }

protected:
  virtual void push_method() override {
    gorio_apd_t* h = this->handle();
    int mode = 0, kept_voxel_mode = 0, nn = 0;
    double radius = 0.0, width = 0.0, max_dist = 0.0;
    gorio_apd_get_ndt_cuda_params(h, &mode, &radius);
    gorio_apd_get_vgicp_cuda_params(h, &nn, &width, &max_dist);
    gorio_apd_get_method(h, nullptr, nullptr, nullptr, &kept_voxel_mode);  // voxel_mode is ignored by this method and kept by the handle
    if (nn != static_cast<int>(neighbor_method_) || width != kernel_width_ || max_dist != kernel_max_dist_)
      this->check(gorio_apd_set_vgicp_cuda_params(h, static_cast<int>(neighbor_method_), kernel_width_, kernel_max_dist_));
    const int search = static_cast<int>(search_method_);
    // the library checks a DIRECT_RADIUS radius in the call that puts it in use: the radius goes first when DIRECT_RADIUS is selected, last otherwise
    if (search == GORIO_VOXEL_DIRECT_RADIUS && radius != radius_) this->check(gorio_apd_set_ndt_cuda_params(h, mode, radius_));
    this->check(this->select_method(GORIO_METHOD_VGICP_CUDA, resolution_, search, kept_voxel_mode));
    if (search != GORIO_VOXEL_DIRECT_RADIUS && radius != radius_) this->check(gorio_apd_set_ndt_cuda_params(h, mode, radius_));
  }
  void pull_result() {
    this->final_transformation_ = this->backend_->getFinalTransformation();
    this->final_hessian_ = this->backend_->getFinalHessian();
    this->converged_ = this->backend_->hasConverged();
    this->nr_iterations_ = this->backend_->iterations();
  }

  double resolution_ = 1.0;
  double kernel_width_ = 0.5, kernel_max_dist_ = 3.0;
  NeighborSearchMethod search_method_ = NeighborSearchMethod::DIRECT1;
  double radius_ = -1.0;
  NearestNeighborMethod neighbor_method_ = NearestNeighborMethod::CPU_PARALLEL_KDTREE;
};
}  // namespace fast_gicp

#endif
