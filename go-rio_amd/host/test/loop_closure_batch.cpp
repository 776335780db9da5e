// Loop-closure verification (loop_detector.cpp:386-422) through the drop-in fast_gicp::FastAPDGICP, twice:
//   single: the reference pattern -- ONE object, setInputTarget(keyframe), then per candidate setInputSource, align(*aligned, guess),
//           getFitnessScore() (and getInlierFraction());
//   batch:  N objects sharing the target (setInputTargetShared), ONE alignBatch, ONE getFitnessScoreBatch, ONE getInlierFractionBatch.
// Input: binary [int32 n_cand][int32 n_tgt][n_tgt x (x,y,z,label) float32], then per candidate [int32 n][n x (x,y,z,label) float32]
// [16 float32: guess, row-major].  Output: one JSON line per candidate and mode.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>

using PointT = pcl::PointXYZINormal;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;

static void configure(Reg& r) {  // registrations.cpp:38-51 with launch/ntu_loop3.launch:85-96
  r.setNumThreads(0);
  r.setTransformationEpsilon(0.1);
  r.setMaximumIterations(64);
  r.setMaxCorrespondenceDistance(2.0);
  r.setCorrespondenceRandomness(20);
  r.setDistVar(0.86);
  r.setAzimuthVar(0.5);
  r.setElevationVar(1.0);
}

static pcl::PointCloud<PointT>::Ptr read_cloud(std::FILE* f) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return nullptr;
  std::vector<float> buf((size_t)n * 4);
  if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return nullptr;
  pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
  c->resize(n);
  for (int i = 0; i < n; ++i) {
    PointT& p = c->points[i];
    p.x = buf[4 * i];
    p.y = buf[4 * i + 1];
    p.z = buf[4 * i + 2];
    p.normal_x = buf[4 * i + 3];
  }
  return c;
}

static void print(const char* mode, int i, const Eigen::Matrix4f& T, bool converged, int nr_iterations, const Eigen::Matrix<double, 6, 6>& H, double fitness, float inlier,
                  const pcl::PointCloud<PointT>& aligned) {
  std::printf("{\"mode\": \"%s\", \"i\": %d, \"converged\": %d, \"nr_iterations\": %d, \"fitness\": %.17g, \"inlier\": %.9g, \"aligned0\": [%.9g, %.9g, %.9g], \"T\": [", mode, i,
              converged ? 1 : 0, nr_iterations, fitness, inlier, aligned.points[0].x, aligned.points[0].y, aligned.points[0].z);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("], \"H\": [");
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) std::printf("%.17g%s", H(r, c), (r == 5 && c == 5) ? "" : ", ");
  std::printf("]}\n");
}

// nr_iterations_ is protected in pcl::Registration (the reference's callers never read it); a member pointer formed in a subclass reads it
struct Probe : Reg {
  static int iterations(const Reg& r) { return r.*(&Probe::nr_iterations_); }
};

static bool same(const Eigen::Matrix4f& a, const Eigen::Matrix4f& b) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c)
      if (a(r, c) != b(r, c)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s candidates.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_cand = 0;
  if (std::fread(&n_cand, 4, 1, f) != 1 || n_cand <= 0) return 2;
  pcl::PointCloud<PointT>::Ptr target = read_cloud(f);
  if (!target) return 2;
  std::vector<pcl::PointCloud<PointT>::Ptr> sources;
  std::vector<Eigen::Matrix4f> guesses;
  for (int k = 0; k < n_cand; ++k) {
    pcl::PointCloud<PointT>::Ptr c = read_cloud(f);
    float g[16];
    if (!c || std::fread(g, 4, 16, f) != 16) return 2;
    Eigen::Matrix4f G;
    for (int r = 0; r < 4; ++r)
      for (int cc = 0; cc < 4; ++cc) G(r, cc) = g[r * 4 + cc];
    sources.push_back(c);
    guesses.push_back(G);
  }
  std::fclose(f);

  try {
    // ---- the reference pattern: one registration object, N aligns and N fitness calls
    Reg single;
    configure(single);
    single.setInputTarget(target);
    for (int k = 0; k < n_cand; ++k) {
      single.setInputSource(sources[k]);
      pcl::PointCloud<PointT> aligned;
      single.align(aligned, guesses[k]);
      const double fitness = single.getFitnessScore();
      const float inlier = single.getInlierFraction();
      print("single", k, single.getFinalTransformation(), single.hasConverged(), Probe::iterations(single), single.getFinalHessian(), fitness, inlier, aligned);
    }

    // ---- the batch surface: N objects on one shared target, one device pass per step
    std::vector<std::unique_ptr<Reg>> objs;
    std::vector<Reg*> regs;
    for (int k = 0; k < n_cand; ++k) {
      objs.emplace_back(new Reg());
      configure(*objs.back());
      if (k == 0) objs[0]->setInputTarget(target);
      else objs[k]->setInputTargetShared(*objs[0]);
      objs[k]->setInputSource(sources[k]);
      regs.push_back(objs[k].get());
    }
    std::vector<pcl::PointCloud<PointT>> aligned;
    Reg::alignBatch(regs, guesses, &aligned);
    const std::vector<double> fitness = Reg::getFitnessScoreBatch(regs);
    const std::vector<float> inlier = Reg::getInlierFractionBatch(regs);
    for (int k = 0; k < n_cand; ++k)
      print("batch", k, regs[k]->getFinalTransformation(), regs[k]->hasConverged(), Probe::iterations(*regs[k]), regs[k]->getFinalHessian(), fitness[k], inlier[k], aligned[k]);

    // ---- errors: objects whose settings differ cannot share one lock-step batch, and the failed call changes none of them
    if (n_cand < 2) return 0;
    const Eigen::Matrix4f before = regs[0]->getFinalTransformation();
    regs[1]->setMaxCorrespondenceDistance(1.0);
    std::string what;
    try {
      Reg::alignBatch(regs, guesses);
    } catch (const std::runtime_error& e) {
      what = e.what();
    }
    regs[1]->setMaxCorrespondenceDistance(2.0);
    std::printf("{\"mismatch_error\": \"%s\", \"unchanged\": %d}\n", what.empty() ? "" : "runtime_error", same(regs[0]->getFinalTransformation(), before) ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  return 0;
}
