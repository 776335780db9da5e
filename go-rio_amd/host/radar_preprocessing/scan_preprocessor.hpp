// gorio::ScanPreprocessor<PointT>: the body of the preprocessing nodelet's cloud_callback (apps/preprocessing_nodelet_ntu.cpp:370-581,
// "PREP") without ROS, on top of the C ABI of include/gorio_scan.h.  One object per sensor: it owns the pipeline handle and with it the
// Patchwork++ state that the nodelet keeps in its PatchWorkpp member.  The scan goes to the GPU once and stays there through every
// stage; process() downloads only what the nodelet publishes.  There is no CPU fallback: without a HIP device process() throws.
//
// What the nodelet does around the callback stays with the caller: message conversion, the TF lookup of PREP:487-501 (the rotation is
// a parameter) and publishing.  The RANSAC samples of the ego-velocity estimate are drawn here from the caller's std::mt19937, the way
// REVE:186-193 draws them (one std::shuffle of 0 .. n_valid - 1 per iteration, the first n_ransac_points taken), so a fixed seed gives
// a fixed result.
#ifndef GORIO_SCAN_PREPROCESSOR_HPP
#define GORIO_SCAN_PREPROCESSOR_HPP

#include <algorithm>
#include <memory>
#include <numeric>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_scan.h>

namespace gorio {

// REVE:186-193 for n_iter iterations: out[n_iter][k].  Empty when RANSAC is off or there are fewer valid targets than one sample needs
// (the estimate then fails in the library, as REVE:180 does).
inline std::vector<unsigned int> draw_ransac_samples(const gorio_reve_config& cfg, int n_valid, std::mt19937& rng) {
  std::vector<unsigned int> out;
  if (!cfg.use_ransac || n_valid < cfg.n_ransac_points) return out;
  const int n_iter = gorio_prep_reve_ransac_iterations(&cfg);
  std::vector<unsigned int> idx(n_valid);
  std::iota(idx.begin(), idx.end(), 0u);
  for (int k = 0; k < n_iter; ++k) {
    std::shuffle(idx.begin(), idx.end(), rng);
    out.insert(out.end(), idx.begin(), idx.begin() + cfg.n_ransac_points);
  }
  return out;
}

template <typename PointT>
class ScanPreprocessor {
 public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudPtr = typename Cloud::Ptr;
  using CloudConstPtr = typename Cloud::ConstPtr;

  struct Result {
    int status = GORIO_SCAN_EMPTY;  // gorio_scan_status
    CloudPtr full_scan;             // what the nodelet publishes (PREP:570-579); null unless status is GORIO_SCAN_OK
    double v_r[3] = {0, 0, 0}, sigma_v_r[3] = {0, 0, 0};
    int n_ground = 0, n_clusters = 0;
    std::string message;            // for GORIO_SCAN_REFUSED: the refusing stage's own text
  };

  explicit ScanPreprocessor(const gorio_scan_params& params, int device = 0) : params_(params) {
    if (gorio_scan_create(&h_, device, &params) != 0) throw std::runtime_error(std::string("gorio_scan_create: ") + gorio_scan_last_error());
  }
  ScanPreprocessor() : ScanPreprocessor(defaults()) {}
  ~ScanPreprocessor() { gorio_scan_destroy(h_); }
  ScanPreprocessor(const ScanPreprocessor&) = delete;
  ScanPreprocessor& operator=(const ScanPreprocessor&) = delete;

  static gorio_scan_params defaults() {
    gorio_scan_params p;
    gorio_scan_default_params(&p);
    return p;
  }

  // PREP:370-581.  raw_points: any type with float x, y, z (geometry_msgs::Point32); power = channels[2].values, doppler =
  // channels[0].values; ang_vel = the IMU's angular velocity (3 doubles) or nullptr when no IMU message is at hand (PREP:660-662).
  // Result::full_scan is the cloud the nodelet publishes: intensity = power, curvature = Doppler, normal_x = cluster label.  A stage that
  // refuses the cloud (one not larger than mean_k, say) gives status GORIO_SCAN_REFUSED with that stage's text in Result::message; the
  // next process() starts clean.  Anything else that fails (no device, a bad argument) throws std::runtime_error.
  template <typename RawPointT>
  Result process(const std::vector<RawPointT>& raw_points, const std::vector<float>& power, const std::vector<float>& doppler, const double* ang_vel, std::mt19937& rng) {
    const int n = static_cast<int>(raw_points.size());
    if (power.size() != raw_points.size() || doppler.size() != raw_points.size()) throw std::invalid_argument("ScanPreprocessor::process: one power and one Doppler value per point");
    stage_.resize(5 * static_cast<std::size_t>(n));
    for (int i = 0; i < n; ++i) {
      float* r = &stage_[5 * static_cast<std::size_t>(i)];
      r[0] = raw_points[i].x;
      r[1] = raw_points[i].y;
      r[2] = raw_points[i].z;
      r[3] = power[i];
      r[4] = doppler[i];
    }
    return process_packed(stage_.data(), n, ang_vel, rng);
  }

  // the same on a message already packed as n x (x, y, z, power, doppler) floats; raw5 may be null when n is 0
  Result process_packed(const float* raw5, int n, const double* ang_vel, std::mt19937& rng) {
    last_.reset();
    int n_gated = 0, n_valid = 0;
    check(gorio_scan_load(h_, raw5, raw5 ? raw5 + 3 : nullptr, raw5 ? raw5 + 4 : nullptr, n, 20, &n_gated, &n_valid));
    const std::vector<unsigned int> samples = draw_ransac_samples(params_.reve, n_valid, rng);
    gorio_scan_result r;
    const int rc = gorio_scan_run(h_, samples.empty() ? nullptr : samples.data(), static_cast<int>(samples.size()) / std::max(params_.reve.n_ransac_points, 1), ang_vel, &r);
    Result o;
    if (rc < 0 && r.status == GORIO_SCAN_REFUSED) o.message = gorio_scan_last_error();
    else check(rc);
    o.status = r.status;
    for (int q = 0; q < 3; ++q) {
      o.v_r[q] = r.v_r[q];
      o.sigma_v_r[q] = r.sigma_v_r[q];
    }
    o.n_ground = r.n_ground;
    o.n_clusters = r.n_clusters;
    if (r.status != GORIO_SCAN_OK) return o;
    CloudPtr out(new Cloud());
    out->resize(r.n_out);
    if (r.n_out > 0) {
      PointT& p0 = out->points[0];
      check(gorio_scan_get_output(h_, &p0.x, &p0.intensity, &p0.curvature, &p0.normal_x, static_cast<int>(sizeof(PointT)), r.n_out));
    }
    o.full_scan = out;
    last_ = out;
    return o;
  }

  // process_packed for many sensors (or many recorded messages, one object each) in lock-step rounds on the GPU (include/gorio_scan_batch.h):
  // message i goes through pre[i].  The RANSAC samples are drawn in member order from the one rng, so the results, last_scan() included,
  // equal the same process_packed calls made one after another with the same generator.  ang_vel[i] may be null, and so may raw5[i] when
  // n[i] is 0.  The exception rules are process_packed's: a refused member is a Result with `message` and does not throw.
  static std::vector<Result> processBatch(const std::vector<ScanPreprocessor*>& pre, const std::vector<const float*>& raw5, const std::vector<int>& n,
                                          const std::vector<const double*>& ang_vel, std::mt19937& rng) {
    const std::size_t count = pre.size();
    if (raw5.size() != count || n.size() != count || ang_vel.size() != count) throw std::invalid_argument("ScanPreprocessor::processBatch: one message, size and angular velocity per object");
    std::vector<Result> out(count);
    if (count == 0) return out;
    std::vector<gorio_scan_t*> hs(count);
    std::vector<const float*> power(count), doppler(count);
    std::vector<int> stride(count, 20), n_gated(count, 0), n_valid(count, 0);
    for (std::size_t i = 0; i < count; ++i) {
      if (!pre[i]) throw std::invalid_argument("ScanPreprocessor::processBatch: null object");
      pre[i]->last_.reset();
      hs[i] = pre[i]->h_;
      power[i] = raw5[i] ? raw5[i] + 3 : nullptr;
      doppler[i] = raw5[i] ? raw5[i] + 4 : nullptr;
    }
    batch_check(gorio_scan_load_batch(hs.data(), static_cast<int>(count), raw5.data(), power.data(), doppler.data(), n.data(), stride.data(), n_gated.data(), n_valid.data()));
    std::vector<std::vector<unsigned int>> samples(count);
    std::vector<const unsigned int*> sample_ptr(count);
    std::vector<int> n_iter(count);
    for (std::size_t i = 0; i < count; ++i) {
      const gorio_scan_params& P = pre[i]->params_;
      samples[i] = draw_ransac_samples(P.reve, n_valid[i], rng);
      sample_ptr[i] = samples[i].empty() ? nullptr : samples[i].data();
      n_iter[i] = static_cast<int>(samples[i].size()) / std::max(P.reve.n_ransac_points, 1);
    }
    std::vector<gorio_scan_result> res(count);
    std::vector<int> codes(count, 0);
    batch_check(gorio_scan_run_batch(hs.data(), static_cast<int>(count), sample_ptr.data(), n_iter.data(), ang_vel.data(), res.data(), codes.data()));
    for (std::size_t i = 0; i < count; ++i) {
      const gorio_scan_result& r = res[i];
      Result& o = out[i];
      if (codes[i] < 0 && r.status == GORIO_SCAN_REFUSED) o.message = gorio_scan_handle_error(hs[i]);
      else if (codes[i] < 0) throw std::runtime_error(std::string("ScanPreprocessor (gorio_amd): member ") + std::to_string(i) + ": " + gorio_scan_handle_error(hs[i]) + " [code " + std::to_string(codes[i]) + "]");
      o.status = r.status;
      for (int q = 0; q < 3; ++q) {
        o.v_r[q] = r.v_r[q];
        o.sigma_v_r[q] = r.sigma_v_r[q];
      }
      o.n_ground = r.n_ground;
      o.n_clusters = r.n_clusters;
      if (r.status != GORIO_SCAN_OK) continue;
      CloudPtr cloud(new Cloud());
      cloud->resize(r.n_out);
      if (r.n_out > 0) {
        PointT& p0 = cloud->points[0];
        pre[i]->check(gorio_scan_get_output(hs[i], &p0.x, &p0.intensity, &p0.curvature, &p0.normal_x, static_cast<int>(sizeof(PointT)), r.n_out));
      }
      o.full_scan = cloud;
      pre[i]->last_ = cloud;
    }
    return out;
  }

  // the cloud of the last process() that produced a frame (null otherwise): what FastAPDGICP::setInputSourceFromScan keeps as input_
  CloudConstPtr last_scan() const { return last_; }
  gorio_scan_t* handle() { return h_; }
  const gorio_scan_params& params() const { return params_; }

 private:
  void check(int rc) const {
    if (rc < 0) throw std::runtime_error(std::string("ScanPreprocessor (gorio_amd): ") + gorio_scan_last_error() + " [code " + std::to_string(rc) + "]");
  }
  static void batch_check(int rc) {
    if (rc < 0) throw std::runtime_error(std::string("ScanPreprocessor (gorio_amd): ") + gorio_scan_last_error() + " [code " + std::to_string(rc) + "]");
  }
  gorio_scan_params params_;
  gorio_scan_t* h_ = nullptr;
  std::vector<float> stage_;
  CloudConstPtr last_;
};

}  // namespace gorio
#endif
