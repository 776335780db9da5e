// Drop-in for ndt_omp/include/pclomp/gicp_omp.h of the Go-RIO sources (GOH; GO = gicp_omp_impl.hpp): pclomp::GeneralizedIterativeClosestPoint
// with the surface select_registration_method (registrations.cpp:91-100, GICP_OMP) and ndt_omp/apps/align.cpp use, on top of ONE
// registration handle of include/gorio_apd.h switched to GORIO_METHOD_GICP_OMP.  Covariances, correspondences, Mahalanobis matrices and
// the functor run on the GPU; the BFGS shell runs inside the library, one device evaluation per round trip.  No CPU fallback: the
// constructor throws std::runtime_error when no HIP device is usable.
// Every member of GOH:141-260 is here.  estimateRigidTransformationBFGS is public in the reference but reads the object's private
// Mahalanobis matrices, so it only works from inside computeTransformation: a direct call is refused (std::logic_error).  setUseReciprocalCorrespondences
// (registrations.cpp:96) is accepted and unused, as GO never reads it.  getFitnessScore runs on the GPU as in the fast_gicp drop-ins.
// Extras without a counterpart in the reference: setInputSourceFromScan / setInputTargetFromScan, setInputSourceKeyframe /
// setInputTargetKeyframe, handle(), and the batch surface in the shape of pclomp/ndt_omp.h: setInputTargetShared, alignBatch
// (gorio_apd_gicp_omp_align_batch: the aligns of many objects in lock-step rounds, every result bit for bit the single align's),
// getFitnessScoreBatch.
#pragma once
#include <cfloat>
#include <cmath>
#include <functional>
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

namespace pclomp {

template <typename PointSource, typename PointTarget>
class GeneralizedIterativeClosestPoint : public pcl::Registration<PointSource, PointTarget> {
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
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = pcl::PointCloud<PointTarget>;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  using MatricesVector = std::vector<Eigen::Matrix3d, Eigen::aligned_allocator<Eigen::Matrix3d>>;
  using MatricesVectorPtr = std::shared_ptr<MatricesVector>;
  using MatricesVectorConstPtr = std::shared_ptr<const MatricesVector>;
  using Ptr = std::shared_ptr<GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const GeneralizedIterativeClosestPoint<PointSource, PointTarget>>;
  using Vector6d = Eigen::Matrix<double, 6, 1>;

  explicit GeneralizedIterativeClosestPoint(int device = 0) : k_correspondences_(20), gicp_epsilon_(0.001), rotation_epsilon_(2e-3), max_inner_iterations_(20) {  // GOH:116-136
    reg_name_ = "GeneralizedIterativeClosestPoint";
    max_iterations_ = 200;
    transformation_epsilon_ = 5e-4;
    corr_dist_threshold_ = 5.;
    const int rc = gorio_apd_create(&h_, device);
    if (rc != GORIO_OK) throw std::runtime_error("pclomp::GeneralizedIterativeClosestPoint (gorio_amd): no usable HIP device [code " + std::to_string(rc) + "]");
    check(gorio_apd_set_method(h_, GORIO_METHOD_GICP_OMP, 1.0, GORIO_VOXEL_DIRECT1, GORIO_VOXEL_ADDITIVE), "GeneralizedIterativeClosestPoint");
    // pcl::Registration::align() must not build a CPU kd-tree of every target for a class that never searches it (as in FastAPDGICP)
    this->setSearchMethodTarget(this->getSearchMethodTarget(), /*force_no_recompute=*/true);
  }
  virtual ~GeneralizedIterativeClosestPoint() { gorio_apd_destroy(h_); }
  GeneralizedIterativeClosestPoint(const GeneralizedIterativeClosestPoint&) = delete;
  GeneralizedIterativeClosestPoint& operator=(const GeneralizedIterativeClosestPoint&) = delete;

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {  // GOH:141-157
    if (cloud->points.empty()) return;  // "Invalid or empty point cloud dataset given!"
    Base::setInputSource(cloud);
    check(gorio_apd_set_source(h_, cloud->points[0].data, &cloud->points[0].normal_x, (int)cloud->size(), (int)sizeof(PointSource)), "setInputSource");
    input_covariances_.reset();
    pairs_valid_ = false;
  }
  void setSourceCovariances(const MatricesVectorPtr& covariances) { input_covariances_ = covariances; }  // GOH:164-168
  void setInputTarget(const PointCloudTargetConstPtr& target) override {  // GOH:173-178
    Base::setInputTarget(target);
    const int n = (int)target->size();
    check(n ? gorio_apd_set_target(h_, target->points[0].data, &target->points[0].normal_x, n, (int)sizeof(PointTarget)) : gorio_apd_clear_target(h_), "setInputTarget");
    target_covariances_.reset();
    pairs_valid_ = false;
  }
  void setTargetCovariances(const MatricesVectorPtr& covariances) { target_covariances_ = covariances; }  // GOH:185-189
  // The target of `owner` as this object's target (extra): the device cloud, its covariances and its search index are shared, nothing is
  // uploaded or estimated twice.  The loop-closure shape: N candidate objects on one keyframe's target, then alignBatch.
  void setInputTargetShared(GeneralizedIterativeClosestPoint& owner) {
    push_params();
    owner.push_params();
    check(gorio_apd_set_target_shared(h_, owner.h_), "setInputTargetShared");
    Base::setInputTarget(owner.target_);
    target_covariances_.reset();
    pairs_valid_ = false;
  }

  // The frame a gorio::ScanPreprocessor just produced / a keyframe resident in a gorio::KeyframeStore as source or target (extras): the
  // handle shares the device cloud and its search index, nothing is uploaded; the host cloud becomes input_ / target_.
  template <typename Preprocessor>
  void setInputSourceFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("pclomp::GeneralizedIterativeClosestPoint::setInputSourceFromScan: the preprocessor's last process() produced no frame");
    push_params();
    check(gorio_apd_set_source_from_scan(h_, pre.handle()), "setInputSourceFromScan");
    Base::setInputSource(pre.last_scan());
    input_covariances_.reset();
    pairs_valid_ = false;
  }
  template <typename Preprocessor>
  void setInputTargetFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("pclomp::GeneralizedIterativeClosestPoint::setInputTargetFromScan: the preprocessor's last process() produced no frame");
    push_params();
    check(gorio_apd_set_target_from_scan(h_, pre.handle()), "setInputTargetFromScan");
    Base::setInputTarget(pre.last_scan());
    target_covariances_.reset();
    pairs_valid_ = false;
  }
  template <typename Store>
  void setInputSourceKeyframe(Store& store, int id) {
    push_params();
    check(gorio_apd_set_source_from_keyframe(h_, store.handle(), id), "setInputSourceKeyframe");
    Base::setInputSource(store.cloud(id));
    input_covariances_.reset();
    pairs_valid_ = false;
  }
  template <typename Store>
  void setInputTargetKeyframe(Store& store, int id) {
    push_params();
    check(gorio_apd_set_target_from_keyframe(h_, store.handle(), id), "setInputTargetKeyframe");
    Base::setInputTarget(store.cloud(id));
    target_covariances_.reset();
    pairs_valid_ = false;
  }

  // GOH:199-204.  Public in the reference, but it reads the object's private Mahalanobis matrices and temporaries, so it only works from
  // inside computeTransformation; here that whole loop is one library call, and a direct call is refused.
  void estimateRigidTransformationBFGS(const PointCloudSource&, const std::vector<int>&, const PointCloudTarget&, const std::vector<int>&, Eigen::Matrix4f&) {
    throw std::logic_error("pclomp::GeneralizedIterativeClosestPoint::estimateRigidTransformationBFGS: the inner solve runs inside align() (gorio_apd_align)");
  }

  // GOH:207-211: Mahalanobis matrix of source point `index` after the last align (identity for a point without a pair, as the resize of GO:384 leaves it)
  const Eigen::Matrix4f& mahalanobis(size_t index) const {
    if (!pairs_valid_) throw std::logic_error("pclomp::GeneralizedIterativeClosestPoint::mahalanobis: no align yet");
    if (mahalanobis_.empty()) {
      const int n = (int)input_->size();
      std::vector<double> m((size_t)n * 16);
      std::vector<int> corr(n);
      check(gorio_apd_get_mahalanobis(h_, m.data(), n), "mahalanobis");
      check(gorio_apd_get_correspondences(h_, corr.data(), nullptr, n), "mahalanobis");
      mahalanobis_.resize(n);
      for (int i = 0; i < n; ++i) {
        mahalanobis_[i].setIdentity();
        if (corr[i] < 0) continue;
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) mahalanobis_[i](r, c) = (float)m[(size_t)i * 16 + r * 4 + c];
      }
    }
    return mahalanobis_.at(index);
  }

  // GOH:220-221, GO:125-177: d/d_rx, d/d_ry, d/d_rz of tr(dR^T R) into g(3), g(4), g(5)
  void computeRDerivative(const Vector6d& x, const Eigen::Matrix3d& R, Vector6d& g) const {
    const double phi = x(3), theta = x(4), psi = x(5);
    const double cphi = std::cos(phi), sphi = std::sin(phi), ctheta = std::cos(theta), stheta = std::sin(theta), cpsi = std::cos(psi), spsi = std::sin(psi);
    Eigen::Matrix3d dPhi, dTheta, dPsi;
    dPhi(0, 0) = 0.; dPhi(1, 0) = 0.; dPhi(2, 0) = 0.;
    dPhi(0, 1) = sphi * spsi + cphi * cpsi * stheta; dPhi(1, 1) = -cpsi * sphi + cphi * spsi * stheta; dPhi(2, 1) = cphi * ctheta;
    dPhi(0, 2) = cphi * spsi - cpsi * sphi * stheta; dPhi(1, 2) = -cphi * cpsi - sphi * spsi * stheta; dPhi(2, 2) = -ctheta * sphi;
    dTheta(0, 0) = -cpsi * stheta; dTheta(1, 0) = -spsi * stheta; dTheta(2, 0) = -ctheta;
    dTheta(0, 1) = cpsi * ctheta * sphi; dTheta(1, 1) = ctheta * sphi * spsi; dTheta(2, 1) = -sphi * stheta;
    dTheta(0, 2) = cphi * cpsi * ctheta; dTheta(1, 2) = cphi * ctheta * spsi; dTheta(2, 2) = -cphi * stheta;
    dPsi(0, 0) = -ctheta * spsi; dPsi(1, 0) = cpsi * ctheta; dPsi(2, 0) = 0.;
    dPsi(0, 1) = -cphi * cpsi - sphi * spsi * stheta; dPsi(1, 1) = -cphi * spsi + cpsi * sphi * stheta; dPsi(2, 1) = 0.;
    dPsi(0, 2) = cpsi * sphi - cphi * spsi * stheta; dPsi(1, 2) = sphi * spsi + cphi * cpsi * stheta; dPsi(2, 2) = 0.;
    g(3) = inner_prod(dPhi, R);
    g(4) = inner_prod(dTheta, R);
    g(5) = inner_prod(dPsi, R);
  }

  void setRotationEpsilon(double epsilon) { rotation_epsilon_ = epsilon; }  // GOH:228-229
  double getRotationEpsilon() { return rotation_epsilon_; }                 // GOH:234-235
  void setCorrespondenceRandomness(int k) { k_correspondences_ = k; }       // GOH:243-244
  int getCorrespondenceRandomness() { return k_correspondences_; }          // GOH:249-250
  void setMaximumOptimizerIterations(int max) { max_inner_iterations_ = max; }  // GOH:255-256
  int getMaximumOptimizerIterations() { return max_inner_iterations_; }         // GOH:259-260
  void setUseReciprocalCorrespondences(bool use) { use_reciprocal_ = use; }  // pcl::IterativeClosestPoint's setter (registrations.cpp:96); GO never reads it
  bool getUseReciprocalCorrespondences() const { return use_reciprocal_; }

  // pcl::Registration::getFitnessScore on the GPU (gorio_apd_fitness_score), at final_transformation_
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) override {
    float T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) T[r * 4 + c] = final_transformation_(r, c);
    double score = 0.0;
    check(gorio_apd_fitness_score(h_, T, max_range, 0.0, &score, nullptr), "getFitnessScore");
    pairs_valid_ = false;  // the score's search replaced the correspondences held
    return score;
  }
  // regs[i]->align(outputs[i], guesses[i]) for every i through ONE gorio_apd_gicp_omp_align_batch (extra): afterwards every object is in
  // the state its own align leaves (hasConverged, getFinalTransformation, getIterationCounts, mahalanobis), bit for bit.  The objects must
  // carry the same pcl::Registration settings, rotation epsilon and correspondence randomness; the optimizer iterations may differ.
  static void alignBatch(const std::vector<GeneralizedIterativeClosestPoint*>& regs, const std::vector<typename Base::Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    if (regs.size() != guesses.size()) throw std::invalid_argument("pclomp::GeneralizedIterativeClosestPoint::alignBatch: one guess per object");
    const std::size_t count = regs.size();
    for (std::size_t i = 0; i < count; ++i) {
      if (!regs[i]) throw std::invalid_argument("pclomp::GeneralizedIterativeClosestPoint::alignBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::runtime_error("pclomp::GeneralizedIterativeClosestPoint::alignBatch: object " + std::to_string(i) + " has no source or no target");
    }
    if (outputs) outputs->resize(count);
    if (count == 0) return;
    std::vector<gorio_apd_t*> hs(count);
    std::vector<float> G(count * 16), T(count * 16);
    std::vector<int> conv(count), nr(count);
    for (std::size_t i = 0; i < count; ++i) {
      GeneralizedIterativeClosestPoint& o = *regs[i];
      o.push_params();
      o.upload_covariances(o.input_covariances_, true);
      o.upload_covariances(o.target_covariances_, false);
      hs[i] = o.h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) G[i * 16 + 4 * r + c] = guesses[i](r, c);
    }
    regs[0]->check(gorio_apd_gicp_omp_align_batch(hs.data(), (int)count, G.data(), T.data(), conv.data(), nr.data(), nullptr), "alignBatch");
    for (std::size_t i = 0; i < count; ++i) {
      GeneralizedIterativeClosestPoint& o = *regs[i];
      o.mahalanobis_.clear();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) o.final_transformation_(r, c) = T[i * 16 + 4 * r + c];
      o.converged_ = conv[i] != 0;
      o.nr_iterations_ = nr[i];
      o.pairs_valid_ = true;
      if (outputs) {
        PointCloudSource& out = (*outputs)[i];
        const int n = (int)o.input_->size();
        if ((int)out.size() != n) out.points = o.input_->points;
        if (n > 0) o.check(gorio_apd_transform_source(o.h_, &T[i * 16], out.points[0].data, n, (int)sizeof(PointSource)), "alignBatch");
      }
    }
  }
  // getFitnessScore of every object at its own final transformation through ONE gorio_apd_fitness_score_batch (extra)
  static std::vector<double> getFitnessScoreBatch(const std::vector<GeneralizedIterativeClosestPoint*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<double> score(regs.size());
    if (regs.empty()) return score;
    std::vector<gorio_apd_t*> hs(regs.size());
    std::vector<float> T(regs.size() * 16);
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("pclomp::GeneralizedIterativeClosestPoint::getFitnessScoreBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::logic_error("pclomp::GeneralizedIterativeClosestPoint::getFitnessScoreBatch: no source or no target");
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[i * 16 + 4 * r + c] = regs[i]->final_transformation_(r, c);
    }
    regs[0]->check(gorio_apd_fitness_score_batch(hs.data(), (int)regs.size(), T.data(), max_range, 0.0, score.data(), nullptr), "getFitnessScoreBatch");
    for (std::size_t i = 0; i < regs.size(); ++i) regs[i]->pairs_valid_ = false;  // the score's search replaced the correspondences held
    return score;
  }
  // outer iterations, minimizeOneStep calls and functor evaluations of the last align (extra: gorio_apd_gicp_omp_diag)
  void getIterationCounts(int& outer, int& inner_total, int& evaluations) const { gorio_apd_gicp_omp_diag(h_, &outer, &inner_total, &evaluations, nullptr); }
  gorio_apd_t* handle() { return h_; }

 protected:
  int k_correspondences_;
  double gicp_epsilon_;
  double rotation_epsilon_;
  int max_inner_iterations_;
  MatricesVectorPtr input_covariances_;
  MatricesVectorPtr target_covariances_;
  mutable std::vector<Eigen::Matrix4f> mahalanobis_;

  void computeTransformation(PointCloudSource& output, const typename Base::Matrix4& guess) override {  // GO:375-520
    push_params();
    upload_covariances(input_covariances_, true);
    upload_covariances(target_covariances_, false);
    float g[16], T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) g[r * 4 + c] = guess(r, c);
    int conv = 0, nit = 0;
    mahalanobis_.clear();
    check(gorio_apd_align(h_, g, T, nullptr, &conv, &nit, nullptr), "align");
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) final_transformation_(r, c) = T[r * 4 + c];
    converged_ = conv != 0;
    nr_iterations_ = nit;
    pairs_valid_ = true;
    const int n = (int)input_->size();  // GO:519
    if ((int)output.size() != n) output.points = input_->points;
    if (n > 0) check(gorio_apd_transform_source(h_, T, output.points[0].data, n, (int)sizeof(PointSource)), "align");
  }

 private:
  gorio_apd_t* h_ = nullptr;
  bool use_reciprocal_ = false;
  mutable bool pairs_valid_ = false;

  static double inner_prod(const Eigen::Matrix3d& mat1, const Eigen::Matrix3d& mat2) {  // matricesInnerProd, GOH:324-334
    double r = 0.;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) r += mat1(j, i) * mat2(i, j);
    return r;
  }
  void check(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("pclomp::GeneralizedIterativeClosestPoint::") + what + " (gorio_amd): " + gorio_apd_last_error(h_) + " [code " + std::to_string(rc) + "]");
  }
  void push_params() {  // the members GO reads -> gorio_apd_params + gorio_apd_set_gicp_omp_params
    gorio_apd_params p;
    gorio_apd_default_params(&p);
    p.k_correspondences = k_correspondences_;
    p.corr_dist_threshold = corr_dist_threshold_;
    p.max_iterations = max_iterations_;
    p.rotation_epsilon = rotation_epsilon_;
    p.transformation_epsilon = transformation_epsilon_;
    check(gorio_apd_set_params(h_, &p), "parameters");
    check(gorio_apd_set_gicp_omp_params(h_, gicp_epsilon_, max_inner_iterations_), "parameters");
  }
  // covariances supplied by the caller (GO:386, 392: used when the vector is not empty); a vector whose size is not the cloud's leaves
  // the cloud without covariances and the library estimates them (the reference would read past such a vector)
  void upload_covariances(const MatricesVectorPtr& covs, bool source) {
    if (!covs || covs->empty()) return;
    std::vector<double> rm(covs->size() * 16, 0.0);
    for (std::size_t i = 0; i < covs->size(); ++i)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) rm[i * 16 + r * 4 + c] = (*covs)[i](r, c);
    check(source ? gorio_apd_set_source_covariances(h_, rm.data(), (int)covs->size()) : gorio_apd_set_target_covariances(h_, rm.data(), (int)covs->size()), "covariances");
  }
};

}  // namespace pclomp
