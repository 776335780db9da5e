// Drop-in for the reference's fast_gicp/ndt/ndt_cuda.hpp (NH:22-71) backed by the MI355X library libgorio_amd.so: the class a fast_gicp
// build on an NVIDIA box calls NDT_CUDA (pygicp, gicp_test.cpp), here as GORIO_METHOD_NDT_CUDA of the registration handle.  Same namespace,
// class name, template parameters, Ptr typedefs, setters and overrides as the reference; header-only; no CPU fallback (the constructor
// throws std::runtime_error when no HIP device is usable).  What the class computes is defined in include/gorio_apd.h.
//
// Like FastVGICP it is a FastGICP whose handle runs another method: the device handle, the cloud uploads, the LsqRegistration settings and
// align / linearize / compute_error / fitness through the C ABI exist once, in fast_apdgicp.hpp.  The members FastGICP adds to the
// reference's surface (setCorrespondenceRandomness, setRegularizationMethod, the covariance setters and getters) mean nothing to NDT: the
// first two are ignored, the covariance calls throw (GORIO_ERR_STATE).
//
// Member -> ABI:  setDistanceMode / the radius of setNeighborSearchMethod -> gorio_apd_set_ndt_cuda_params; setResolution /
// setNeighborSearchMethod -> gorio_apd_set_method(GORIO_METHOD_NDT_CUDA, resolution, method, -); swapSourceAndTarget ->
// gorio_apd_swap_source_and_target (clouds and voxel maps change sides, NC:90-93); the maps are built at the first linearise / align
// (create_voxelmaps, NI:76-79).  Deviation: setResolution after a map was built rebuilds it (the reference keeps the old map, NC:120-140).
#ifndef FAST_GICP_NDT_CUDA_HPP
#define FAST_GICP_NDT_CUDA_HPP

#include <fast_gicp/gicp/fast_gicp.hpp>
#include <fast_gicp/gicp/gicp_settings.hpp>
#include <fast_gicp/ndt/ndt_settings.hpp>

namespace fast_gicp {

template <typename PointSource, typename PointTarget>
class NDTCuda : public FastGICP<PointSource, PointTarget> {
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
  using Ptr = pcl::shared_ptr<NDTCuda<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const NDTCuda<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<NDTCuda<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const NDTCuda<PointSource, PointTarget>>;
#endif

protected:
  using pcl::Registration<PointSource, PointTarget, Scalar>::reg_name_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::input_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::target_;
  using Base = FastGICP<PointSource, PointTarget>;

public:
  explicit NDTCuda(int device = 0) : Base(device) {  // NI:11-14, NC:13-23: D2D, DIRECT7, resolution 1.0
    reg_name_ = "NDTCuda";
  }
  virtual ~NDTCuda() override {}

  void setDistanceMode(NDTDistanceMode mode) { distance_mode_ = mode; }  // NI:20
  void setResolution(double resolution) { resolution_ = resolution; }    // NI:25
  void setNeighborSearchMethod(NeighborSearchMethod method, double radius = -1.0) {  // NI:30
    search_method_ = method;
    radius_ = radius;
  }

  virtual void swapSourceAndTarget() override { Base::swapSourceAndTarget(); }  // NI:35-38
  virtual void clearSource() override { Base::clearSource(); }                  // NI:41
  virtual void clearTarget() override { Base::clearTarget(); }                  // NI:46
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) override { Base::setInputSource(cloud); }  // NI:51-60 (the same pointer: no-op)
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override { Base::setInputTarget(cloud); }  // NI:63-73

  // ---- extras the other drop-ins have (no counterpart in the reference)
  // regs[i]->align(outputs[i], guesses[i]) for every i through ONE gorio_apd_align_batch; every result is bit for bit the single align's
  static void alignBatch(const std::vector<NDTCuda*>& regs, const std::vector<Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    std::vector<FastAPDGICP<PointSource, PointTarget>*> back(regs.size());
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("NDTCuda::alignBatch: null object");
      regs[i]->push_settings();
      back[i] = regs[i]->backend_.get();
    }
    FastAPDGICP<PointSource, PointTarget>::alignBatch(back, guesses, outputs);
    for (NDTCuda* r : regs) r->pull_result();
  }
  static std::vector<double> getFitnessScoreBatch(const std::vector<NDTCuda*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<FastAPDGICP<PointSource, PointTarget>*> back(regs.size());
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("NDTCuda::getFitnessScoreBatch: null object");
      regs[i]->backend_->set_final(regs[i]->final_transformation_);
      back[i] = regs[i]->backend_.get();
    }
    return FastAPDGICP<PointSource, PointTarget>::getFitnessScoreBatch(back, max_range);
  }
  // one target, and ONE voxel map, for many objects (gorio_apd_set_target_shared)
  void setInputTargetShared(NDTCuda& owner) {
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
  // parity hook: voxels of the source (0) / target (1) map, gorio_apd_ndt_cuda_get_voxels
  int voxelCount(int which) {
    push_method();
    int nv = 0;
    this->check(gorio_apd_ndt_cuda_get_voxels(this->handle(), which, 0, &nv, nullptr, nullptr, nullptr, nullptr, nullptr));
    return nv;
  }

protected:
  virtual void push_method() override {
    gorio_apd_t* h = this->handle();
    int mode = 0, kept_voxel_mode = 0;
    double radius = 0.0;
    gorio_apd_get_ndt_cuda_params(h, &mode, &radius);
    gorio_apd_get_method(h, nullptr, nullptr, nullptr, &kept_voxel_mode);  // voxel_mode is ignored by this method and kept by the handle
    const int search = static_cast<int>(search_method_);
    const bool params_differ = mode != static_cast<int>(distance_mode_) || radius != radius_;
    // the library checks a DIRECT_RADIUS radius in the call that puts it in use: the radius goes first when DIRECT_RADIUS is selected, last otherwise
    if (search == GORIO_VOXEL_DIRECT_RADIUS && params_differ) this->check(gorio_apd_set_ndt_cuda_params(h, static_cast<int>(distance_mode_), radius_));
    this->check(this->select_method(GORIO_METHOD_NDT_CUDA, resolution_, search, kept_voxel_mode));
    if (search != GORIO_VOXEL_DIRECT_RADIUS && params_differ) this->check(gorio_apd_set_ndt_cuda_params(h, static_cast<int>(distance_mode_), radius_));
  }
  void pull_result() {
    this->final_transformation_ = this->backend_->getFinalTransformation();
    this->final_hessian_ = this->backend_->getFinalHessian();
    this->converged_ = this->backend_->hasConverged();
    this->nr_iterations_ = this->backend_->iterations();
  }

  NDTDistanceMode distance_mode_ = NDTDistanceMode::D2D;
  double resolution_ = 1.0;
  NeighborSearchMethod search_method_ = NeighborSearchMethod::DIRECT7;
  double radius_ = -1.0;
};
}  // namespace fast_gicp

#endif
