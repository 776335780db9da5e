// gorio::IterativeClosestPoint -- pcl::IterativeClosestPoint as select_registration_method hands it out (registrations.cpp:72-79, ICP),
// on top of ONE registration handle of include/gorio_apd.h switched to GORIO_METHOD_ICP.  The correspondence search, the gate, the
// reciprocal check and the 17 sums of the rigid-transform estimate run on the GPU; the loop and its convergence criteria run inside the
// library, one round trip per iteration.  No CPU fallback: the constructor throws std::runtime_error when no HIP device is usable.
// The header lives under gorio/ and the class in namespace gorio, so a deployment that also has PCL's <pcl/registration/icp.h> keeps
// both; the one-line edit of the factory is in INTEGRATION.md.
// Setters and getters are those of pcl::IterativeClosestPoint / pcl::Registration with PCL's constructor defaults: 10 iterations,
// transformation epsilon 0, sqrt(DBL_MAX) correspondence distance, euclidean fitness epsilon -DBL_MAX, no reciprocal correspondences.
// getConvergeCriteria() gives read access to the convergence state of the last align (the criteria themselves are the library's).
// Extras in the shape of the other drop-ins: setInputTargetShared, setInputSourceFromScan / setInputTargetFromScan,
// setInputSourceKeyframe / setInputTargetKeyframe, alignBatch (gorio_apd_icp_align_batch: every result bit for bit the single align's),
// getFitnessScoreBatch, handle().
#pragma once
#include <cfloat>
#include <cmath>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/registration/registration.h>

#include "gorio_apd.h"
#include "gorio_scan.h"
#include "gorio_keyframes.h"

namespace gorio {

template <typename PointSource, typename PointTarget>
class IterativeClosestPoint : public pcl::Registration<PointSource, PointTarget> {
 protected:
  using Base = pcl::Registration<PointSource, PointTarget>;
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
  using PointCloudSource = pcl::PointCloud<PointSource>;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = pcl::PointCloud<PointTarget>;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  using Ptr = std::shared_ptr<IterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const IterativeClosestPoint<PointSource, PointTarget>>;

  // pcl::registration::DefaultConvergenceCriteria::ConvergenceState, same values
  enum ConvergenceState {
    CONVERGENCE_CRITERIA_NOT_CONVERGED = 0,
    CONVERGENCE_CRITERIA_ITERATIONS = 1,
    CONVERGENCE_CRITERIA_TRANSFORM = 2,
    CONVERGENCE_CRITERIA_ABS_MSE = 3,
    CONVERGENCE_CRITERIA_REL_MSE = 4,
    CONVERGENCE_CRITERIA_NO_CORRESPONDENCES = 5,
    CONVERGENCE_CRITERIA_FAILURE_AFTER_MAX_ITERATIONS = 6
  };
  // What getConvergeCriteria() hands out: the outcome of the last align
  class ConvergenceCriteria {
   public:
    ConvergenceState getConvergenceState() const { return state_; }
    int getIterations() const { return iterations_; }
    double getMeanSquaredError() const { return mse_; }
    int getCorrespondences() const { return pairs_; }

   private:
    friend class IterativeClosestPoint;
    ConvergenceState state_ = CONVERGENCE_CRITERIA_NOT_CONVERGED;
    int iterations_ = 0, pairs_ = -1;
    double mse_ = 0.0;
  };

  explicit IterativeClosestPoint(int device = 0) : criteria_(new ConvergenceCriteria) {
    reg_name_ = "IterativeClosestPoint";
    max_iterations_ = 10;
    transformation_epsilon_ = 0.0;
    corr_dist_threshold_ = std::sqrt(std::numeric_limits<double>::max());
    const int rc = gorio_apd_create(&h_, device);
    if (rc != GORIO_OK) throw std::runtime_error("gorio::IterativeClosestPoint (gorio_amd): no usable HIP device [code " + std::to_string(rc) + "]");
    check(gorio_apd_set_method(h_, GORIO_METHOD_ICP, 1.0, GORIO_VOXEL_DIRECT1, GORIO_VOXEL_ADDITIVE), "IterativeClosestPoint");
    // pcl::Registration::align() must not build a CPU kd-tree of every target for a class that never searches it
    this->setSearchMethodTarget(this->getSearchMethodTarget(), /*force_no_recompute=*/true);
  }
  virtual ~IterativeClosestPoint() { gorio_apd_destroy(h_); }
  IterativeClosestPoint(const IterativeClosestPoint&) = delete;
  IterativeClosestPoint& operator=(const IterativeClosestPoint&) = delete;

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {
    if (cloud->points.empty()) return;
    Base::setInputSource(cloud);
    check(gorio_apd_set_source(h_, cloud->points[0].data, &cloud->points[0].normal_x, (int)cloud->size(), (int)sizeof(PointSource)), "setInputSource");
  }
  void setInputTarget(const PointCloudTargetConstPtr& target) override {
    Base::setInputTarget(target);
    const int n = (int)target->size();
    check(n ? gorio_apd_set_target(h_, target->points[0].data, &target->points[0].normal_x, n, (int)sizeof(PointTarget)) : gorio_apd_clear_target(h_), "setInputTarget");
  }
  // The target of `owner` as this object's target: the device cloud and its search index are shared, nothing is uploaded twice.  The
  // loop-closure shape: N candidate objects on one keyframe's target, then alignBatch.
  void setInputTargetShared(IterativeClosestPoint& owner) {
    push_params();
    owner.push_params();
    check(gorio_apd_set_target_shared(h_, owner.h_), "setInputTargetShared");
    Base::setInputTarget(owner.target_);
  }
  // The frame a gorio::ScanPreprocessor just produced / a keyframe resident in a gorio::KeyframeStore as source or target: the handle
  // shares the device cloud and its search index, nothing is uploaded; the host cloud becomes input_ / target_.
  template <typename Preprocessor>
  void setInputSourceFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("gorio::IterativeClosestPoint::setInputSourceFromScan: the preprocessor's last process() produced no frame");
    check(gorio_apd_set_source_from_scan(h_, pre.handle()), "setInputSourceFromScan");
    Base::setInputSource(pre.last_scan());
  }
  template <typename Preprocessor>
  void setInputTargetFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("gorio::IterativeClosestPoint::setInputTargetFromScan: the preprocessor's last process() produced no frame");
    check(gorio_apd_set_target_from_scan(h_, pre.handle()), "setInputTargetFromScan");
    Base::setInputTarget(pre.last_scan());
  }
  template <typename Store>
  void setInputSourceKeyframe(Store& store, int id) {
    check(gorio_apd_set_source_from_keyframe(h_, store.handle(), id), "setInputSourceKeyframe");
    Base::setInputSource(store.cloud(id));
  }
  template <typename Store>
  void setInputTargetKeyframe(Store& store, int id) {
    check(gorio_apd_set_target_from_keyframe(h_, store.handle(), id), "setInputTargetKeyframe");
    Base::setInputTarget(store.cloud(id));
  }

  // pcl::IterativeClosestPoint / pcl::Registration members the base stand-in does not carry (setMaximumIterations,
  // setTransformationEpsilon and setMaxCorrespondenceDistance are the base's)
  void setUseReciprocalCorrespondences(bool use) { use_reciprocal_ = use; }
  bool getUseReciprocalCorrespondences() const { return use_reciprocal_; }
  void setTransformationRotationEpsilon(double epsilon) { transformation_rotation_epsilon_ = epsilon; }
  double getTransformationRotationEpsilon() const { return transformation_rotation_epsilon_; }
  void setEuclideanFitnessEpsilon(double epsilon) { euclidean_fitness_epsilon_ = epsilon; }
  double getEuclideanFitnessEpsilon() const { return euclidean_fitness_epsilon_; }
  int getMaximumIterations() const { return max_iterations_; }
  double getTransformationEpsilon() const { return transformation_epsilon_; }
  std::shared_ptr<const ConvergenceCriteria> getConvergeCriteria() const { return criteria_; }
  int getNumberOfIterations() const { return nr_iterations_; }

  // pcl::Registration::getFitnessScore on the GPU (gorio_apd_fitness_score), at final_transformation_
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    float T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) T[r * 4 + c] = final_transformation_(r, c);
    double score = 0.0;
    check(gorio_apd_fitness_score(h_, T, max_range, 0.0, &score, nullptr), "getFitnessScore");
    return score;
  }
  // regs[i]->align(outputs[i], guesses[i]) for every i through ONE gorio_apd_icp_align_batch: afterwards every object is in the state its
  // own align leaves (hasConverged, getFinalTransformation, getConvergeCriteria), bit for bit.  The objects must carry the same maximum
  // iterations, transformation epsilon and correspondence distance; the reciprocal switch and the other two epsilons may differ.
  static void alignBatch(const std::vector<IterativeClosestPoint*>& regs, const std::vector<typename Base::Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    if (regs.size() != guesses.size()) throw std::invalid_argument("gorio::IterativeClosestPoint::alignBatch: one guess per object");
    const std::size_t count = regs.size();
    for (std::size_t i = 0; i < count; ++i) {
      if (!regs[i]) throw std::invalid_argument("gorio::IterativeClosestPoint::alignBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::runtime_error("gorio::IterativeClosestPoint::alignBatch: object " + std::to_string(i) + " has no source or no target");
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
    regs[0]->check(gorio_apd_icp_align_batch(hs.data(), (int)count, G.data(), T.data(), conv.data(), nr.data()), "alignBatch");
    for (std::size_t i = 0; i < count; ++i) {
      IterativeClosestPoint& o = *regs[i];
      o.take_results(&T[i * 16], conv[i], nr[i]);
      if (outputs) o.move_source(&T[i * 16], (*outputs)[i], "alignBatch");
    }
  }
  // getFitnessScore of every object at its own final transformation through ONE gorio_apd_fitness_score_batch
  static std::vector<double> getFitnessScoreBatch(const std::vector<IterativeClosestPoint*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<double> score(regs.size());
    if (regs.empty()) return score;
    std::vector<gorio_apd_t*> hs(regs.size());
    std::vector<float> T(regs.size() * 16);
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("gorio::IterativeClosestPoint::getFitnessScoreBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::logic_error("gorio::IterativeClosestPoint::getFitnessScoreBatch: no source or no target");
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[i * 16 + 4 * r + c] = regs[i]->final_transformation_(r, c);
    }
    regs[0]->check(gorio_apd_fitness_score_batch(hs.data(), (int)regs.size(), T.data(), max_range, 0.0, score.data(), nullptr), "getFitnessScoreBatch");
    return score;
  }
  // lock-step rounds and kernel launches of the last alignBatch this object led (regs[0])
  void getBatchCounts(int& rounds, int& launches) const { check(gorio_apd_icp_batch_diag(h_, &rounds, &launches), "getBatchCounts"); }
  gorio_apd_t* handle() { return h_; }

 protected:
  void computeTransformation(PointCloudSource& output, const typename Base::Matrix4& guess) override {
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
  gorio_apd_t* h_ = nullptr;
  bool use_reciprocal_ = false;
  double transformation_rotation_epsilon_ = 0.0;
  double euclidean_fitness_epsilon_ = -std::numeric_limits<double>::max();
  std::shared_ptr<ConvergenceCriteria> criteria_;

  void check(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("gorio::IterativeClosestPoint::") + what + " (gorio_amd): " + gorio_apd_last_error(h_) + " [code " + std::to_string(rc) + "]");
  }
  void push_params() {  // the members ICP reads -> gorio_apd_params + gorio_apd_set_icp_params
    gorio_apd_params p;
    gorio_apd_default_params(&p);
    p.corr_dist_threshold = corr_dist_threshold_;
    p.max_iterations = max_iterations_;
    p.transformation_epsilon = transformation_epsilon_;
    check(gorio_apd_set_params(h_, &p), "parameters");
    check(gorio_apd_set_icp_params(h_, use_reciprocal_ ? 1 : 0, euclidean_fitness_epsilon_, transformation_rotation_epsilon_), "parameters");
  }
  void take_results(const float* T, int conv, int nit) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) final_transformation_(r, c) = T[r * 4 + c];
    converged_ = conv != 0;
    nr_iterations_ = nit;
    int state = 0;
    check(gorio_apd_icp_diag(h_, &criteria_->iterations_, &state, &criteria_->mse_, &criteria_->pairs_), "align");
    criteria_->state_ = static_cast<ConvergenceState>(state);
  }
  void move_source(const float* T, PointCloudSource& out, const char* what) {  // output = final_transformation_ * input_
    const int n = (int)input_->size();
    if ((int)out.size() != n) out.points = input_->points;
    if (n > 0) check(gorio_apd_transform_source(h_, T, out.points[0].data, n, (int)sizeof(PointSource)), what);
  }
};

}  // namespace gorio
