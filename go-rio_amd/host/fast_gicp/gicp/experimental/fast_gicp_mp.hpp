// fast_gicp::FastGICPMultiPoints<PointSource, PointTarget> -- the multi-point GICP of the reference's experimental directory
// (fast_gicp/gicp/experimental/fast_gicp_mp.hpp:40-56) on top of ONE registration handle of include/gorio_apd.h switched to
// GORIO_METHOD_GICP_MP.  Every source point is matched against a distribution merged from all target points within
// neighbor_search_radius_; covariances, neighbourhoods, merge and linearisation run on the GPU, the Gauss-Newton shell inside the
// library.  No CPU fallback: the constructor throws std::runtime_error when no HIP device is usable.
// Only the class surface is the reference's; every body is a call into the C ABI.  Constructor defaults are those of
// fast_gicp_mp_impl.hpp:20-36: k 20, 64 iterations, rotation and transformation epsilon 1e-5, PLANE, radius 0.5.
//   - setNumThreads is accepted and ignored.
//   - The covariances are made at setInputSource / setInputTarget, as in the reference (fast_gicp_mp_impl.hpp:68-77).  A
//     setCorrespondenceRandomness / setRegularizationMethod AFTER them makes the next align estimate them again (the reference would go on
//     with the old ones).
//   - ADDITION: setNeighborSearchRadius (the reference fixes 0.5 in its constructor and has no setter).
//   - Extras in the shape of the other drop-ins: setInputTargetShared, setInputSourceFromScan / setInputTargetFromScan,
//     setInputSourceKeyframe / setInputTargetKeyframe, getFitnessScore on the GPU, handle(), and the loop-closure shape: static alignBatch
//     (gorio_apd_gicp_mp_align_batch: N objects, usually on one shared target, in lock-step rounds over one batched radius search per
//     round; every result bit for bit the object's own align) with getFitnessScoreBatch and getBatchCounts.
#ifndef FAST_GICP_FAST_GICP_MP_HPP
#define FAST_GICP_FAST_GICP_MP_HPP

#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/registration/registration.h>

#include <fast_gicp/gicp/gicp_settings.hpp>

#include "gorio_apd.h"
#include "gorio_scan.h"
#include "gorio_keyframes.h"

namespace fast_gicp {

template <typename PointSource, typename PointTarget>
class FastGICPMultiPoints : public pcl::Registration<PointSource, PointTarget, float> {
 public:
  using Scalar = float;
  using Base = pcl::Registration<PointSource, PointTarget, Scalar>;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = typename Base::PointCloudTarget;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;

 protected:
  using Base::converged_;
  using Base::corr_dist_threshold_;
  using Base::final_transformation_;
  using Base::input_;
  using Base::max_iterations_;
  using Base::nr_iterations_;
  using Base::reg_name_;
  using Base::target_;
  using Base::transformation_epsilon_;

 public:
  explicit FastGICPMultiPoints(int device = 0) {
    k_correspondences_ = 20;
    reg_name_ = "FastGICPMultiPoints";
    max_iterations_ = 64;
    rotation_epsilon_ = 1e-5;
    transformation_epsilon_ = 1e-5;
    regularization_method_ = RegularizationMethod::PLANE;
    corr_dist_threshold_ = std::numeric_limits<float>::max();  // never read
    neighbor_search_radius_ = 0.5;
    const int rc = gorio_apd_create(&h_, device);
    if (rc != GORIO_OK) throw std::runtime_error("fast_gicp::FastGICPMultiPoints (gorio_amd): no usable HIP device [code " + std::to_string(rc) + "]");
    check(gorio_apd_set_method(h_, GORIO_METHOD_GICP_MP, 1.0, GORIO_VOXEL_DIRECT1, GORIO_VOXEL_ADDITIVE), "FastGICPMultiPoints");
    // pcl::Registration::align() must not build a CPU kd-tree of every target for a class that never searches it
    this->setSearchMethodTarget(this->getSearchMethodTarget(), /*force_no_recompute=*/true);
  }
  virtual ~FastGICPMultiPoints() override { gorio_apd_destroy(h_); }
  FastGICPMultiPoints(const FastGICPMultiPoints&) = delete;
  FastGICPMultiPoints& operator=(const FastGICPMultiPoints&) = delete;

  void setNumThreads(int) {}  // the GPU decides

  void setRotationEpsilon(double eps) { rotation_epsilon_ = eps; }

  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; }

  void setRegularizationMethod(RegularizationMethod method) { regularization_method_ = method; }

  // ADDITION (not in the reference): neighbor_search_radius_ of fast_gicp_mp.hpp:72
  void setNeighborSearchRadius(double radius) { neighbor_search_radius_ = radius; }

  double getRotationEpsilon() const { return rotation_epsilon_; }
  double getTransformationEpsilon() const { return transformation_epsilon_; }
  int getCorrespondenceRandomness() const { return k_correspondences_; }
  RegularizationMethod getRegularizationMethod() const { return regularization_method_; }
  double getNeighborSearchRadius() const { return neighbor_search_radius_; }
  int getMaximumIterations() const { return max_iterations_; }
  int getNumberOfIterations() const { return nr_iterations_; }

  virtual void setInputSource(const PointCloudSourceConstPtr& cloud) override {
    if (cloud->points.empty()) return;
    Base::setInputSource(cloud);
    check(gorio_apd_set_source(h_, cloud->points[0].data, &cloud->points[0].normal_x, (int)cloud->size(), (int)sizeof(PointSource)), "setInputSource");
    calculate_covariances(0, "setInputSource");
  }

  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override {
    Base::setInputTarget(cloud);
    const int n = (int)cloud->size();
    check(n ? gorio_apd_set_target(h_, cloud->points[0].data, &cloud->points[0].normal_x, n, (int)sizeof(PointTarget)) : gorio_apd_clear_target(h_), "setInputTarget");
    if (n) calculate_covariances(1, "setInputTarget");
  }

  // The target of `owner` as this object's target: device cloud, search index and float covariances are shared, nothing is uploaded or
  // estimated twice.  Both objects must carry the same k and regularisation.
  void setInputTargetShared(FastGICPMultiPoints& owner) {
    push_params();
    owner.push_params();
    check(gorio_apd_set_target_shared(h_, owner.h_), "setInputTargetShared");
    Base::setInputTarget(owner.target_);
  }
  // The frame a gorio::ScanPreprocessor just produced / a keyframe resident in a gorio::KeyframeStore as source or target: the handle
  // shares the device cloud and its search index, nothing is uploaded; the host cloud becomes input_ / target_.
  template <typename Preprocessor>
  void setInputSourceFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("fast_gicp::FastGICPMultiPoints::setInputSourceFromScan: the preprocessor's last process() produced no frame");
    check(gorio_apd_set_source_from_scan(h_, pre.handle()), "setInputSourceFromScan");
    Base::setInputSource(pre.last_scan());
    calculate_covariances(0, "setInputSourceFromScan");
  }
  template <typename Preprocessor>
  void setInputTargetFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("fast_gicp::FastGICPMultiPoints::setInputTargetFromScan: the preprocessor's last process() produced no frame");
    check(gorio_apd_set_target_from_scan(h_, pre.handle()), "setInputTargetFromScan");
    Base::setInputTarget(pre.last_scan());
    calculate_covariances(1, "setInputTargetFromScan");
  }
  template <typename Store>
  void setInputSourceKeyframe(Store& store, int id) {
    check(gorio_apd_set_source_from_keyframe(h_, store.handle(), id), "setInputSourceKeyframe");
    Base::setInputSource(store.cloud(id));
    calculate_covariances(0, "setInputSourceKeyframe");
  }
  template <typename Store>
  void setInputTargetKeyframe(Store& store, int id) {
    check(gorio_apd_set_target_from_keyframe(h_, store.handle(), id), "setInputTargetKeyframe");
    Base::setInputTarget(store.cloud(id));
    calculate_covariances(1, "setInputTargetKeyframe");
  }

  // pcl::Registration::getFitnessScore on the GPU (gorio_apd_fitness_score), at final_transformation_
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    float T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) T[r * 4 + c] = final_transformation_(r, c);
    double score = 0.0;
    check(gorio_apd_fitness_score(h_, T, max_range, 0.0, &score, nullptr), "getFitnessScore");
    return score;
  }
  // passes of the last align, source points used and neighbours found in its last pass
  void getPassCounts(int& passes, int& used, long long& neighbours) const { check(gorio_apd_gicp_mp_diag(h_, &passes, &used, &neighbours, nullptr), "getPassCounts"); }
  // align() of every object from its own guess in ONE gorio_apd_gicp_mp_align_batch.  Parameters and radii may differ per object.  A null
  // object or a guess count that does not match throws std::invalid_argument, an object without source or target and whatever the
  // library refuses std::runtime_error, before any object has changed.
  static void alignBatch(const std::vector<FastGICPMultiPoints*>& regs, const std::vector<Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    if (regs.size() != guesses.size()) throw std::invalid_argument("fast_gicp::FastGICPMultiPoints::alignBatch: one guess per object");
    const std::size_t count = regs.size();
    for (std::size_t i = 0; i < count; ++i) {
      if (!regs[i]) throw std::invalid_argument("fast_gicp::FastGICPMultiPoints::alignBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::runtime_error("fast_gicp::FastGICPMultiPoints::alignBatch: object " + std::to_string(i) + " has no source or no target");
    }
    if (outputs) outputs->resize(count);
    if (count == 0) return;
    std::vector<gorio_apd_t*> hs(count);
    std::vector<float> G(count * 16), T(count * 16);
    std::vector<int> conv(count), nr(count);
    for (std::size_t i = 0; i < count; ++i) {
      regs[i]->push_params();
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) G[i * 16 + 4 * r + c] = guesses[i](r, c);
    }
    regs[0]->check(gorio_apd_gicp_mp_align_batch(hs.data(), (int)count, G.data(), T.data(), conv.data(), nr.data()), "alignBatch");
    for (std::size_t i = 0; i < count; ++i) {
      FastGICPMultiPoints& o = *regs[i];
      o.take_results(&T[i * 16], conv[i], nr[i]);
      if (outputs) o.move_source(&T[i * 16], (*outputs)[i], "alignBatch");
    }
  }
  // getFitnessScore of every object at its own final transformation through ONE gorio_apd_fitness_score_batch
  static std::vector<double> getFitnessScoreBatch(const std::vector<FastGICPMultiPoints*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<double> score(regs.size());
    if (regs.empty()) return score;
    std::vector<gorio_apd_t*> hs(regs.size());
    std::vector<float> T(regs.size() * 16);
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("fast_gicp::FastGICPMultiPoints::getFitnessScoreBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::logic_error("fast_gicp::FastGICPMultiPoints::getFitnessScoreBatch: no source or no target");
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[i * 16 + 4 * r + c] = regs[i]->final_transformation_(r, c);
    }
    regs[0]->check(gorio_apd_fitness_score_batch(hs.data(), (int)regs.size(), T.data(), max_range, 0.0, score.data(), nullptr), "getFitnessScoreBatch");
    return score;
  }
  // of the last alignBatch this object led (regs[0]): lock-step rounds, kernel launches and synchronisations of all rounds, and the
  // launches of its most expensive round
  void getBatchCounts(int& rounds, int& launches, int& syncs, int& max_round_launches) const {
    check(gorio_apd_gicp_mp_batch_diag(h_, &rounds, &launches, &syncs, &max_round_launches), "getBatchCounts");
  }
  gorio_apd_t* handle() { return h_; }

 protected:
  virtual void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {
    push_params();
    float g[16], T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) g[r * 4 + c] = guess(r, c);
    int conv = 0, nit = 0;
    check(gorio_apd_align(h_, g, T, nullptr, &conv, &nit, nullptr), "align");
    take_results(T, conv, nit);
    move_source(T, output, "align");
  }

 private:
  int k_correspondences_;
  double rotation_epsilon_;
  double neighbor_search_radius_;
  RegularizationMethod regularization_method_;
  gorio_apd_t* h_ = nullptr;

  void take_results(const float* T, int conv, int nit) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) final_transformation_(r, c) = T[r * 4 + c];
    converged_ = conv != 0;
    nr_iterations_ = nit;
  }
  void move_source(const float* T, PointCloudSource& output, const char* what) {  // pcl::transformPointCloud(*input_, output, final_transformation_), fast_gicp_mp_impl.hpp:114
    const int n = (int)input_->size();
    if ((int)output.size() != n) output.points = input_->points;
    if (n > 0) check(gorio_apd_transform_source(h_, T, output.points[0].data, n, (int)sizeof(PointSource)), what);
  }
  void check(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("fast_gicp::FastGICPMultiPoints::") + what + " (gorio_amd): " + gorio_apd_last_error(h_) + " [code " + std::to_string(rc) + "]");
  }
  void push_params() {  // the members this class reads -> gorio_apd_params + gorio_apd_set_gicp_mp_params
    gorio_apd_params p;
    gorio_apd_default_params(&p);
    p.k_correspondences = k_correspondences_;
    p.regularization = static_cast<int>(regularization_method_);
    p.max_iterations = max_iterations_;
    p.rotation_epsilon = rotation_epsilon_;
    p.transformation_epsilon = transformation_epsilon_;
    check(gorio_apd_set_params(h_, &p), "parameters");
    check(gorio_apd_set_gicp_mp_params(h_, neighbor_search_radius_), "parameters");
  }
  void calculate_covariances(int which, const char* what) {  // fast_gicp_mp_impl.hpp:70, 76
    push_params();
    int n = 0;
    check(gorio_apd_gicp_mp_get_covariances(h_, which, 0, &n, nullptr), what);
  }
};

}  // namespace fast_gicp

#endif
