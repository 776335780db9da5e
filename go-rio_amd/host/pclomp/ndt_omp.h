// Drop-in for ndt_omp/include/pclomp/ndt_omp.h of the Go-RIO sources (NDTH; NDT = ndt_omp_impl.hpp): pclomp::NormalDistributionsTransform
// with the surface select_registration_method (registrations.cpp:117-134) and ndt_omp/apps/align.cpp use, on top of the C ABI of
// include/gorio_ndt.h.  Every body is an ABI call; the voxel map, the derivative sums and the score run on the GPU.  KDTREE is refused
// by the library (std::runtime_error here); its neighbourhood -- pcl::NormalDistributionsTransform -- is the class of gorio/ndt.hpp.
// getFitnessScore, which the nodelets call after every match (scan_matching_odometry_nodelet.cpp:675, loop_detector.cpp:229, 415), is computed on the GPU as the fast_gicp drop-ins do, through a registration handle of include/gorio_apd.h
// that holds the same two clouds; through a pcl::Registration base pointer real PCL still runs its own CPU version.
// Extras without a counterpart in the reference (INTEGRATION.md sections 8, 11): setInputTargetShared, alignBatch, getFitnessScoreBatch,
// calculateScoreBatch, and the inputs that are already on the device: setInputSourceFromScan / setInputTargetFromScan (the frame a
// gorio::ScanPreprocessor just produced) and setInputTargetSubmap (scan-to-submap mode).
#pragma once
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/registration/registration.h>

#include "gorio_apd.h"
#include "gorio_ndt.h"
#include "gorio_scan.h"
#include "gorio_keyframes.h"

namespace pclomp {

enum NeighborSearchMethod { KDTREE, DIRECT26, DIRECT7, DIRECT1 };  // NDTH:52-57

template <typename PointSource, typename PointTarget>
class NormalDistributionsTransform : public pcl::Registration<PointSource, PointTarget> {
 protected:
  using Base = pcl::Registration<PointSource, PointTarget>;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourceConstPtr = typename Base::PointCloudSourceConstPtr;
  using PointCloudTarget = typename Base::PointCloudTarget;
  using PointCloudTargetPtr = typename Base::PointCloudTargetPtr;
  using PointCloudTargetConstPtr = typename Base::PointCloudTargetConstPtr;
  using Base::converged_;
  using Base::final_transformation_;
  using Base::input_;
  using Base::max_iterations_;
  using Base::nr_iterations_;
  using Base::reg_name_;
  using Base::target_;
  using Base::transformation_epsilon_;

 public:
  using Ptr = std::shared_ptr<NormalDistributionsTransform<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const NormalDistributionsTransform<PointSource, PointTarget>>;

  NormalDistributionsTransform() {  // NDT:47-76
    reg_name_ = "NormalDistributionsTransform";
    check(gorio_ndt_create(&h_, 0), "NormalDistributionsTransform");
    gorio_ndt_default_params(&p_);
    transformation_epsilon_ = p_.transformation_epsilon;
    max_iterations_ = p_.max_iterations;
  }
  virtual ~NormalDistributionsTransform() {
    gorio_ndt_destroy(h_);
    if (fit_) gorio_apd_destroy(fit_);
  }
  NormalDistributionsTransform(const NormalDistributionsTransform&) = delete;
  NormalDistributionsTransform& operator=(const NormalDistributionsTransform&) = delete;

  void setNumThreads(int) {}  // NDTH:115: accepted, ignored
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {  // NDTH:122-127
    Base::setInputTarget(cloud);
    fit_target_stale_ = true;
    fit_shared_with_ = nullptr;
    const int n = (int)cloud->size();
    check(gorio_ndt_set_target(h_, n ? &cloud->points[0].x : nullptr, n, (int)sizeof(PointTarget)), "setInputTarget");
  }
  // One map for many registrations (extra): reference the target another object already holds on the device -- its points and its voxel
  // map -- instead of uploading a private copy and building the same map again.  The objects must agree in resolution.
  void setInputTargetShared(NormalDistributionsTransform& owner) {
    check(gorio_ndt_set_target_shared(h_, owner.h_), "setInputTargetShared");
    Base::setInputTarget(owner.target_);
    fit_target_stale_ = true;
    fit_shared_with_ = &owner;
  }
  void setInputSource(const PointCloudSourceConstPtr& cloud) override {
    Base::setInputSource(cloud);
    fit_source_stale_ = true;
    const int n = (int)cloud->size();
    check(gorio_ndt_set_source(h_, n ? &cloud->points[0].x : nullptr, n, (int)sizeof(PointSource)), "setInputSource");
  }
  // The frame a gorio::ScanPreprocessor just produced (radar_preprocessing/scan_preprocessor.hpp) as source / target (extra): one
  // device-to-device copy into the NDT handle (gorio_ndt_set_source_from_scan) instead of an upload of the cloud process() downloaded.
  // The pcl cloud that process() returned becomes input_ / target_.  The same call hands the frame to the private handle of
  // getFitnessScore, with the search index the preprocessing built -- now, not at the first getFitnessScore: by then the preprocessor
  // may hold the next frame.  So a getFitnessScore after the match uploads nothing and builds no index.
  template <typename Preprocessor>
  void setInputSourceFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("pclomp::NormalDistributionsTransform::setInputSourceFromScan: the preprocessor's last process() produced no frame");
    check(gorio_ndt_set_source_from_scan(h_, pre.handle()), "setInputSourceFromScan");
    Base::setInputSource(pre.last_scan());
    fit_source_stale_ = true;  // until the hand-off below has succeeded
    ensure_fitness_handle("setInputSourceFromScan");
    check_apd(gorio_apd_set_source_from_scan(fit_, pre.handle()), "setInputSourceFromScan");
    fit_source_stale_ = false;
  }
  template <typename Preprocessor>
  void setInputTargetFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("pclomp::NormalDistributionsTransform::setInputTargetFromScan: the preprocessor's last process() produced no frame");
    check(gorio_ndt_set_target_from_scan(h_, pre.handle()), "setInputTargetFromScan");
    Base::setInputTarget(pre.last_scan());
    fit_target_stale_ = true;
    fit_shared_with_ = nullptr;
    ensure_fitness_handle("setInputTargetFromScan");
    check_apd(gorio_apd_set_target_from_scan(fit_, pre.handle()), "setInputTargetFromScan");
    fit_target_stale_ = false;
  }
  // A keyframe resident in a gorio::KeyframeStore (radar_graph_slam/keyframe_store.hpp) as source / target (extra; loop_detector.cpp:222,
  // 391 with NDT_OMP): one device-to-device copy into the NDT handle instead of an upload; the store's host cloud becomes input_ /
  // target_.  The private handle of getFitnessScore shares the keyframe where its settings allow it (it estimates no covariances; a
  // keyframe whose covariances carry another k_correspondences is uploaded from the host copy at the first getFitnessScore instead).
  template <typename Store>
  void setInputSourceKeyframe(Store& store, int id) {
    check(gorio_ndt_set_source_from_keyframe(h_, store.handle(), id), "setInputSourceKeyframe");
    Base::setInputSource(store.cloud(id));
    ensure_fitness_handle("setInputSourceKeyframe");
    fit_source_stale_ = gorio_apd_set_source_from_keyframe(fit_, store.handle(), id) < 0;
  }
  template <typename Store>
  void setInputTargetKeyframe(Store& store, int id) {
    check(gorio_ndt_set_target_from_keyframe(h_, store.handle(), id), "setInputTargetKeyframe");
    Base::setInputTarget(store.cloud(id));
    fit_shared_with_ = nullptr;
    ensure_fitness_handle("setInputTargetKeyframe");
    fit_target_stale_ = gorio_apd_set_target_from_keyframe(fit_, store.handle(), id) < 0;
  }
  // Scan-to-submap target assembly on the GPU (extra; the signature and the return value of FastAPDGICP::setInputTargetSubmap, in place of
  // the CPU loop of scan_matching_odometry_nodelet.cpp:602-612): keyframe clouds moved by their relative poses, concatenated, downsampled
  // (voxel_leaf <= 0: the launch files' NONE).  The fitness handle assembles it (gorio_apd_set_target_submap) and keeps it as its own
  // target; the NDT handle takes a copy on the device (gorio_ndt_set_target_from_apd).  The assembled cloud is returned and kept as target_.
  PointCloudTargetConstPtr setInputTargetSubmap(const std::vector<PointCloudTargetConstPtr>& clouds,
                                                const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& rel_poses, double voxel_leaf = 0.0) {
    if (clouds.empty() || clouds.size() != rel_poses.size()) throw std::invalid_argument("pclomp::NormalDistributionsTransform::setInputTargetSubmap: one relative pose per keyframe cloud");
    std::vector<gorio_apd_keyframe> fr(clouds.size());
    std::vector<double> poses(clouds.size() * 16);
    for (std::size_t k = 0; k < clouds.size(); ++k) {
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) poses[k * 16 + r * 4 + c] = rel_poses[k](r, c);
      const bool any = clouds[k] && !clouds[k]->points.empty();
      fr[k].xyz = any ? &clouds[k]->points[0].x : nullptr;
      fr[k].label = nullptr;  // neither NDT nor the fitness score reads labels
      fr[k].n = any ? static_cast<int>(clouds[k]->size()) : 0;
      fr[k].point_stride_bytes = static_cast<int>(sizeof(PointTarget));
      fr[k].rel_pose = &poses[k * 16];
    }
    ensure_fitness_handle("setInputTargetSubmap");
    fit_target_stale_ = true;  // whatever happens below, the fitness handle's target is no longer target_
    fit_shared_with_ = nullptr;
    int n = 0;
    check_apd(gorio_apd_set_target_submap(fit_, fr.data(), static_cast<int>(fr.size()), voxel_leaf, &n), "setInputTargetSubmap");
    check(gorio_ndt_set_target_from_apd(h_, fit_), "setInputTargetSubmap");
    PointCloudTargetPtr out(new PointCloudTarget());
    out->resize(n);
    if (n > 0) check_apd(gorio_apd_get_target_points(fit_, &out->points[0].x, nullptr, n, static_cast<int>(sizeof(PointTarget))), "setInputTargetSubmap");
    for (auto& p : out->points) p.data[3] = 1.0f;
    Base::setInputTarget(out);
    fit_target_stale_ = false;
    return out;
  }
  // which filter the voxel_leaf > 0 branch of setInputTargetSubmap runs: GORIO_DOWNSAMPLE_VOXELGRID (default) or
  // GORIO_DOWNSAMPLE_APPROX_VOXELGRID, on the fitness handle that assembles the submap (gorio_apd_set_submap_downsample)
  void setSubmapDownsampleMethod(int method) {
    ensure_fitness_handle("setSubmapDownsampleMethod");
    check_apd(gorio_apd_set_submap_downsample(fit_, method), "setSubmapDownsampleMethod");
  }
  void setResolution(float resolution) {  // NDTH:132-142
    p_.resolution = resolution;
    push("setResolution");
  }
  float getResolution() const { return (float)p_.resolution; }
  double getStepSize() const { return p_.step_size; }
  void setStepSize(double step_size) {
    p_.step_size = step_size;
    push("setStepSize");
  }
  double getOutlierRatio() const { return p_.outlier_ratio; }
  void setOutlierRatio(double outlier_ratio) {
    p_.outlier_ratio = outlier_ratio;
    push("setOutlierRatio");
  }
  void setNeighborhoodSearchMethod(NeighborSearchMethod method) {  // NDTH:189-191
    p_.search = (int)method;
    push("setNeighborhoodSearchMethod");
  }
  double getTransformationProbability() const { return trans_probability_; }
  int getFinalNumIteration() const { return nr_iterations_; }
  const gorio_ndt_diag& getDiagnostics() const { return diag_; }

  // calculateScore (NDT:935-983): the cloud as given (already transformed), scored against the target
  double calculateScore(const PointCloudSource& cloud) const {
    const int n = (int)cloud.size();
    check(gorio_ndt_set_source(h_, n ? &cloud.points[0].x : nullptr, n, (int)sizeof(PointSource)), "calculateScore");
    const float I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double score = 0.0;
    const int rc = gorio_ndt_calculate_score(h_, I, &score);
    if (input_) {  // the registration's own source comes back
      const int m = (int)input_->size();
      check(gorio_ndt_set_source(h_, m ? &input_->points[0].x : nullptr, m, (int)sizeof(PointSource)), "calculateScore");
    }
    check(rc, "calculateScore");
    return score;
  }

  // pcl::Registration::getFitnessScore(max_range) as the nodelets call it: mean squared nearest-neighbour distance of the source moved by
  // final_transformation_, computed on the GPU (gorio_apd_fitness_score).  The clouds go to that handle at the first call after they changed.
  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    if (!input_ || !target_) throw std::logic_error("pclomp::NormalDistributionsTransform::getFitnessScore: no source or no target");
    fill_fitness_handle(nullptr, "getFitnessScore");
    float T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) T[4 * r + c] = final_transformation_(r, c);
    double score = 0.0;
    check_apd(gorio_apd_fitness_score(fit_, T, max_range, 0.0, &score, nullptr), "getFitnessScore");
    return score;
  }

  // ---- batch surface (extra; no counterpart in the reference).  Loop-closure verification (loop_detector.cpp:386-422) aligns N
  // candidate sources against one target and scores each result: N x (align, getFitnessScore).  These members do the same for N objects
  // -- typically sharing the target through setInputTargetShared -- with one device round trip per evaluation round.

  // regs[i]->align(outputs[i], guesses[i]) for every i through ONE gorio_ndt_align_batch: afterwards every object is in the state the
  // single align leaves (getFinalTransformation, hasConverged, getFinalNumIteration, getTransformationProbability, getDiagnostics),
  // bit for bit; outputs (may be null) receives the moved sources.  The objects' settings may differ.  On an error std::runtime_error
  // with the library's message, and no object is modified.
  static void alignBatch(const std::vector<NormalDistributionsTransform*>& regs, const std::vector<Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    if (regs.size() != guesses.size()) throw std::invalid_argument("pclomp::NormalDistributionsTransform::alignBatch: one guess per object");
    const std::size_t count = regs.size();
    for (std::size_t i = 0; i < count; ++i) {
      if (!regs[i]) throw std::invalid_argument("pclomp::NormalDistributionsTransform::alignBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::runtime_error("pclomp::NormalDistributionsTransform::alignBatch: object " + std::to_string(i) + " has no source or no target");
    }
    if (outputs) outputs->resize(count);
    if (count == 0) return;
    std::vector<gorio_ndt_t*> hs(count);
    std::vector<float> G(count * 16), T(count * 16);
    std::vector<int> conv(count), nr(count);
    std::vector<double> prob(count);
    std::vector<gorio_ndt_diag> diag(count);
    for (std::size_t i = 0; i < count; ++i) {
      regs[i]->p_.transformation_epsilon = regs[i]->transformation_epsilon_;  // as computeTransformation does
      regs[i]->p_.max_iterations = regs[i]->max_iterations_;
      regs[i]->push("alignBatch");
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) G[i * 16 + 4 * r + c] = guesses[i](r, c);
    }
    check(gorio_ndt_align_batch(hs.data(), (int)count, G.data(), T.data(), conv.data(), nr.data(), prob.data(), diag.data(), nullptr), "alignBatch");
    for (std::size_t i = 0; i < count; ++i) {
      NormalDistributionsTransform& o = *regs[i];
      o.trans_probability_ = prob[i];
      o.diag_ = diag[i];
      PointCloudSource* out = nullptr;
      if (outputs) {  // what pcl::Registration::align does to output before computeTransformation
        out = &(*outputs)[i];
        out->points = o.input_->points;
        for (auto& p : out->points) p.data[3] = 1.0f;
      }
      o.finish_align(&T[i * 16], conv[i], nr[i], out);
    }
  }

  // regs[i]->calculateScore(regs[i]'s own source moved by transforms[i]) for every i through ONE gorio_ndt_calculate_score_batch: the
  // values gorio_ndt_calculate_score gives one by one, bit for bit.  No object is modified.
  static std::vector<double> calculateScoreBatch(const std::vector<NormalDistributionsTransform*>& regs, const std::vector<Matrix4>& transforms) {
    if (regs.size() != transforms.size()) throw std::invalid_argument("pclomp::NormalDistributionsTransform::calculateScoreBatch: one transform per object");
    const std::size_t count = regs.size();
    for (std::size_t i = 0; i < count; ++i) {
      if (!regs[i]) throw std::invalid_argument("pclomp::NormalDistributionsTransform::calculateScoreBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::runtime_error("pclomp::NormalDistributionsTransform::calculateScoreBatch: object " + std::to_string(i) + " has no source or no target");
    }
    std::vector<double> score(count);
    if (count == 0) return score;
    std::vector<gorio_ndt_t*> hs(count);
    std::vector<float> T(count * 16);
    for (std::size_t i = 0; i < count; ++i) {
      hs[i] = regs[i]->h_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[i * 16 + 4 * r + c] = transforms[i](r, c);
    }
    check(gorio_ndt_calculate_score_batch(hs.data(), (int)count, T.data(), score.data()), "calculateScoreBatch");
    return score;
  }

  // regs[i]->getFitnessScore(max_range) for every i through ONE gorio_apd_fitness_score_batch at the final transformations: the same
  // values, bit for bit.  Objects that share an NDT target share the fitness target too (gorio_apd_set_target_shared).
  static std::vector<double> getFitnessScoreBatch(const std::vector<NormalDistributionsTransform*>& regs, double max_range = std::numeric_limits<double>::max()) {
    std::vector<double> score(regs.size());
    if (regs.empty()) return score;
    for (std::size_t i = 0; i < regs.size(); ++i) {
      if (!regs[i]) throw std::invalid_argument("pclomp::NormalDistributionsTransform::getFitnessScoreBatch: null object");
      if (!regs[i]->input_ || !regs[i]->target_) throw std::logic_error("pclomp::NormalDistributionsTransform::getFitnessScoreBatch: no source or no target");
    }
    std::vector<gorio_apd_t*> hs(regs.size());
    std::vector<float> T(regs.size() * 16);
    for (std::size_t i = 0; i < regs.size(); ++i) {  // owners first: a sharer links to a fitness handle that already holds the target
      if (!regs[i]->fit_shared_with_) regs[i]->fill_fitness_handle(nullptr, "getFitnessScoreBatch");
    }
    for (std::size_t i = 0; i < regs.size(); ++i) {
      NormalDistributionsTransform& o = *regs[i];
      if (o.fit_shared_with_) {
        NormalDistributionsTransform* owner = nullptr;  // only an owner that is in this batch and still on the shared cloud
        for (std::size_t k = 0; k < regs.size() && !owner; ++k)
          if (regs[k] == o.fit_shared_with_ && !regs[k]->fit_shared_with_ && regs[k]->target_ == o.target_) owner = regs[k];
        o.fill_fitness_handle(owner, "getFitnessScoreBatch");
      }
      hs[i] = o.fit_;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[i * 16 + 4 * r + c] = o.final_transformation_(r, c);
    }
    regs[0]->check_apd(gorio_apd_fitness_score_batch(hs.data(), (int)regs.size(), T.data(), max_range, 0.0, score.data(), nullptr), "getFitnessScoreBatch");
    return score;
  }

 protected:
  gorio_ndt_t* handle() const { return h_; }  // for gorio::NormalDistributionsTransform (gorio/ndt.hpp), which switches the radius search on

  void computeTransformation(PointCloudSource& output, const Eigen::Matrix4f& guess) override {  // NDT:81-171
    p_.transformation_epsilon = transformation_epsilon_;
    p_.max_iterations = max_iterations_;
    push("align");
    float G[16], T[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) G[4 * r + c] = guess(r, c);
    int conv = 0, nr = 0;
    check(gorio_ndt_align(h_, G, T, &conv, &nr, &trans_probability_, &diag_), "align");
    finish_align(T, conv, nr, &output);
  }

 private:
  gorio_ndt_t* h_ = nullptr;
  gorio_ndt_params p_;
  gorio_ndt_diag diag_ = {0, 0, 0, 0.0};
  double trans_probability_ = 0.0;
  gorio_apd_t* fit_ = nullptr;  // getFitnessScore only
  bool fit_target_stale_ = true, fit_source_stale_ = true;
  NormalDistributionsTransform* fit_shared_with_ = nullptr;  // the object setInputTargetShared named (not dereferenced: compared with batch members only)

  // what computeTransformation leaves behind, from the ABI's outputs; output (may be null) holds the source on entry
  void finish_align(const float* T, int conv, int nr, PointCloudSource* output) {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) final_transformation_(r, c) = T[4 * r + c];
    converged_ = conv != 0;
    nr_iterations_ = nr;
    if (!output) return;
    for (auto& p : output->points) {  // the cloud moved by the final transformation, as trans_cloud holds it (NDT:833)
      const float x = p.x, y = p.y, z = p.z;
      p.x = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
      p.y = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
      p.z = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
    }
  }
  void ensure_fitness_handle(const char* what) {
    if (!fit_) check_apd(gorio_apd_create(&fit_, 0), what);
  }
  // the private registration handle of getFitnessScore holds the object's two clouds; with share_from the target is that object's
  // fitness target (one copy on the device) instead of an upload of its own.  A side that is not stale is already there: uploaded by
  // an earlier call, handed over by setInput*FromScan, or assembled by setInputTargetSubmap.
  void fill_fitness_handle(NormalDistributionsTransform* share_from, const char* what) {
    ensure_fitness_handle(what);
    if (fit_target_stale_) {
      if (share_from && share_from->fit_ && !share_from->fit_target_stale_) {
        check_apd(gorio_apd_set_target_shared(fit_, share_from->fit_), what);
      } else {
        const int n = (int)target_->size();
        check_apd(gorio_apd_set_target(fit_, n ? &target_->points[0].x : nullptr, nullptr, n, (int)sizeof(PointTarget)), what);
      }
      fit_target_stale_ = false;
    }
    if (fit_source_stale_) {
      const int n = (int)input_->size();
      check_apd(gorio_apd_set_source(fit_, n ? &input_->points[0].x : nullptr, nullptr, n, (int)sizeof(PointSource)), what);
      fit_source_stale_ = false;
    }
  }

  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("pclomp::NormalDistributionsTransform::") + what + ": " + gorio_ndt_last_error());
  }
  void check_apd(int rc, const char* what) const {
    if (rc < 0) throw std::runtime_error(std::string("pclomp::NormalDistributionsTransform::") + what + ": " + gorio_apd_last_error(fit_));
  }
  void push(const char* what) { check(gorio_ndt_set_params(h_, &p_), what); }
};

}  // namespace pclomp
