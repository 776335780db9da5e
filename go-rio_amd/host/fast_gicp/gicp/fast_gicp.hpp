// Drop-in for the reference's fast_gicp/gicp/fast_gicp.hpp (GICPH:20-104) backed by the MI355X library libgorio_amd.so.
//
// Same namespace, class name, template parameters, Ptr typedefs, public setters and overrides as the reference, so
// 4DRadarSLAM/src/radar_graph_slam/registrations.cpp:28-37 compiles unchanged against this header and the nodelets keep driving the
// object through pcl::Registration<PointXYZINormal,PointXYZINormal>::Ptr.  Header-only; setNumThreads is accepted and ignored; no CPU
// fallback (the constructor throws std::runtime_error when no HIP device is usable).
//
// What FastGICP, FastVGICP and FastAPDGICP share -- the device handle, the cloud uploads, the lazy covariance mirrors, the flush of
// the settings into gorio_apd_params, align / linearize / compute_error / fitness through the C ABI -- exists once, in
// fast_apdgicp.hpp: an object of this class owns a FastAPDGICP back end whose handle is switched to GORIO_METHOD_GICP (or
// GORIO_METHOD_VGICP, fast_vgicp.hpp) with gorio_apd_set_method, and every member below is one call into it.  FastAPDGICP itself
// is untouched by this header.
#ifndef FAST_GICP_FAST_GICP_HPP
#define FAST_GICP_FAST_GICP_HPP

#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>

namespace fast_gicp {

namespace detail {
// the shared back end: FastAPDGICP's device-side machinery with the protected hooks of LsqRegistration opened to the owning object
template <typename PointSource, typename PointTarget>
class GorioBackend : public FastAPDGICP<PointSource, PointTarget> {
  using Base = FastAPDGICP<PointSource, PointTarget>;

public:
  using LazyTree = typename Base::LazyTargetTree;
  explicit GorioBackend(int device) : Base(device) {}
  // LsqRegistration members of the owner (LSQH:75-84) -> the back end's, before a device call flushes them (push_params)
  void settings(int max_iterations, double transformation_epsilon, double corr_dist_threshold, double rotation_epsilon, LSQ_OPTIMIZER_TYPE type, int lm_max_iterations,
                double lm_init_lambda_factor) {
    this->max_iterations_ = max_iterations;
    this->transformation_epsilon_ = transformation_epsilon;
    this->corr_dist_threshold_ = corr_dist_threshold;
    this->rotation_epsilon_ = rotation_epsilon;
    this->lsq_optimizer_type_ = type;
    this->lm_max_iterations_ = lm_max_iterations;
    this->lm_init_lambda_factor_ = lm_init_lambda_factor;
  }
  void run(typename Base::PointCloudSource& output, const typename Base::Matrix4& guess) { Base::computeTransformation(output, guess); }
  double run_linearize(const Eigen::Isometry3d& trans, Eigen::Matrix<double, 6, 6>* H, Eigen::Matrix<double, 6, 1>* b) { return Base::linearize(trans, H, b); }
  double run_compute_error(const Eigen::Isometry3d& trans) { return Base::compute_error(trans); }
  int iterations() const { return this->nr_iterations_; }
  void set_final(const typename Base::Matrix4& T) { this->final_transformation_ = T; }
};
}  // namespace detail

template <typename PointSource, typename PointTarget>
class FastGICP : public LsqRegistration<PointSource, PointTarget> {
public:
  using Scalar = float;
  using Matrix4 = typename pcl::Registration<PointSource, PointTarget, Scalar>::Matrix4;
  using PointCloudSource = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudSource;
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudTarget;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  using CovarianceVector = std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastGICP<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastGICP<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastGICP<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastGICP<PointSource, PointTarget>>;
#endif

protected:
  using pcl::Registration<PointSource, PointTarget, Scalar>::reg_name_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::input_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::target_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::corr_dist_threshold_;
  using Backend = detail::GorioBackend<PointSource, PointTarget>;

public:
  explicit FastGICP(int device = 0) : backend_(new Backend(device)) {  // GICP:14-30
    reg_name_ = "FastGICP";
    corr_dist_threshold_ = std::numeric_limits<float>::max();
    // as in FastAPDGICP: pcl::Registration::align() must not rebuild a CPU kd-tree this class never searches
    typename pcl::Registration<PointSource, PointTarget, Scalar>::KdTreePtr tree(new typename Backend::LazyTree());
    lazy_tree_ = static_cast<typename Backend::LazyTree*>(tree.get());
    this->setSearchMethodTarget(tree, /*force_no_recompute=*/true);
  }
  virtual ~FastGICP() override {}
  FastGICP(const FastGICP&) = delete;
  FastGICP& operator=(const FastGICP&) = delete;

  void setNumThreads(int n) { backend_->setNumThreads(n); }                                                // GICP:36-44
  void setCorrespondenceRandomness(int k) { backend_->setCorrespondenceRandomness(k); }                     // GICP:47
  void setRegularizationMethod(RegularizationMethod method) { backend_->setRegularizationMethod(method); }  // GICP:52

  virtual void swapSourceAndTarget() override {  // GICP:57-64
    input_.swap(target_);
    lazy_tree_->defer(target_);
    backend_->swapSourceAndTarget();
  }
  virtual void clearSource() override {  // GICP:67-70
    input_.reset();
    backend_->clearSource();
  }
  virtual void clearTarget() override {  // GICP:73-76
    target_.reset();
    lazy_tree_->defer(PointCloudTargetConstPtr());
    backend_->clearTarget();
  }
  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) override {  // GICP:79-88
    if (input_ == cloud) return;
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputSource(cloud);
    backend_->setInputSource(cloud);
  }
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // GICP:91-99
    if (target_ == cloud) return;
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(cloud);
    lazy_tree_->defer(cloud);
    backend_->setInputTarget(cloud);
  }
  virtual void setSourceCovariances(const CovarianceVector& covs) { backend_->setSourceCovariances(covs); }  // GICP:102
  virtual void setTargetCovariances(const CovarianceVector& covs) { backend_->setTargetCovariances(covs); }  // GICP:107
  const CovarianceVector& getSourceCovariances() const { return backend_->getSourceCovariances(); }           // GICPH:68-70
  const CovarianceVector& getTargetCovariances() const { return backend_->getTargetCovariances(); }           // GICPH:72-74

  // pcl::Registration::getFitnessScore on the GPU, as FastAPDGICP::getFitnessScore
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    backend_->set_final(this->final_transformation_);
    return backend_->getFitnessScore(max_range);
  }
  float getInlierFraction(double max_correspondence_dist = 0.5) {
    backend_->set_final(this->final_transformation_);
    return backend_->getInlierFraction(max_correspondence_dist);
  }
  // A keyframe resident in a gorio::KeyframeStore as source / target, and the scan-to-submap target from resident keyframes (extras):
  // FastAPDGICP::setInputSourceKeyframe / setInputTargetKeyframe / setInputTargetSubmap(store, ...) with this class' method selected first
  // (the library compares a keyframe's voxel map with FastVGICP's voxel settings).
  template <typename Store>
  void setInputSourceKeyframe(Store& store, int id) {
    push_settings();
    backend_->setInputSourceKeyframe(store, id);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputSource(store.cloud(id));
  }
  template <typename Store>
  void setInputTargetKeyframe(Store& store, int id) {
    push_settings();
    backend_->setInputTargetKeyframe(store, id);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(store.cloud(id));
    lazy_tree_->defer(store.cloud(id));
  }
  template <typename Store>
  PointCloudTargetConstPtr setInputTargetSubmap(Store& store, const std::vector<int>& ids,
                                                const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& rel_poses, double voxel_leaf = 0.0) {
    push_settings();
    PointCloudTargetConstPtr out = backend_->setInputTargetSubmap(store, ids, rel_poses, voxel_leaf);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(out);
    lazy_tree_->defer(out);
    return out;
  }
  // the host-cloud form of the same assembly, and which filter its voxel_leaf > 0 runs (FastAPDGICP::setSubmapDownsampleMethod)
  PointCloudTargetConstPtr setInputTargetSubmap(const std::vector<PointCloudTargetConstPtr>& clouds,
                                                const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& rel_poses, double voxel_leaf = 0.0) {
    push_settings();
    PointCloudTargetConstPtr out = backend_->setInputTargetSubmap(clouds, rel_poses, voxel_leaf);
    pcl::Registration<PointSource, PointTarget, Scalar>::setInputTarget(out);
    lazy_tree_->defer(out);
    return out;
  }
  void setSubmapDownsampleMethod(int method) { backend_->setSubmapDownsampleMethod(method); }
  int getSubmapDownsampleMethod() const { return backend_->getSubmapDownsampleMethod(); }
  gorio_apd_t* handle() { return backend_->handle(); }

protected:
  // which registration the handle runs: gorio_apd_set_method before every device call, like the settings (FastVGICP overrides)
  virtual void push_method() { check(select_method(GORIO_METHOD_GICP, 1.0, GORIO_VOXEL_DIRECT1, GORIO_VOXEL_ADDITIVE)); }

  int select_method(int method, double resolution, int search, int mode) {  // a repeated call would drop the correspondences held
    int m = 0, s = 0, a = 0;
    double r = 0.0;
    gorio_apd_get_method(backend_->handle(), &m, &r, &s, &a);
    if (m == method && r == resolution && s == search && a == mode) return GORIO_OK;
    return gorio_apd_set_method(backend_->handle(), method, resolution, search, mode);
  }
  void push_settings() {
    push_method();
    backend_->settings(this->max_iterations_, this->transformation_epsilon_, corr_dist_threshold_, this->rotation_epsilon_, this->lsq_optimizer_type_, this->lm_max_iterations_,
                       this->lm_init_lambda_factor_);
  }
  void check(int rc) const {
    if (rc < 0) throw std::runtime_error(std::string(reg_name_) + " (gorio_amd): " + gorio_apd_last_error(backend_->handle()) + " [code " + std::to_string(rc) + "]");
  }

  virtual void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {  // GICP:110-123 + LSQ:55-80
    push_settings();
    backend_->run(output, guess);
    this->final_transformation_ = backend_->getFinalTransformation();
    this->final_hessian_ = backend_->getFinalHessian();
    this->converged_ = backend_->hasConverged();
    this->nr_iterations_ = backend_->iterations();
  }
  virtual void update_correspondences(const Eigen::Isometry3d& trans) { linearize(trans, nullptr, nullptr); }  // GICP:126-165
  virtual double linearize(const Eigen::Isometry3d& trans, Eigen::Matrix<double, 6, 6>* H, Eigen::Matrix<double, 6, 1>* b) override {  // GICP:169-231
    push_settings();
    return backend_->run_linearize(trans, H, b);
  }
  virtual double compute_error(const Eigen::Isometry3d& trans) override { return backend_->run_compute_error(trans); }  // GICP:234-257

  std::unique_ptr<Backend> backend_;
  typename Backend::LazyTree* lazy_tree_ = nullptr;
};
}  // namespace fast_gicp

#endif
