// Loop-closure verification (loop_detector.cpp:386-422) with the registration method GICP_OMP, through the drop-in
// pclomp::GeneralizedIterativeClosestPoint configured by the factory's setter calls (registrations.cpp:91-100), twice:
//   single: ONE object, setInputTarget(keyframe), then per candidate setInputSource, align(*aligned, guess), getFitnessScore();
//   batch:  N objects sharing the target (setInputTargetShared), ONE alignBatch, ONE getFitnessScoreBatch, best candidate by score.
// Input: binary [int32 n_cand][int32 n_tgt][n_tgt x (x,y,z,label) float32], then per candidate [int32 n][n x (x,y,z,label) float32]
// [16 float32: guess, row-major]; argv[2..] = reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance,
// reg_correspondence_randomness, reg_max_optimizer_iterations.  Output: one JSON line per candidate and mode, every float in hex, then one
// line with the best candidate of either mode and whether the two modes agree bit for bit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <pclomp/gicp_omp.h>

using PointT = pcl::PointXYZINormal;
using Reg = pclomp::GeneralizedIterativeClosestPoint<PointT, PointT>;

static void configure(Reg& gicp, char** argv) {  // registrations.cpp:91-100
  gicp.setTransformationEpsilon(std::atof(argv[2]));
  gicp.setMaximumIterations(std::atoi(argv[3]));
  gicp.setUseReciprocalCorrespondences(false);
  gicp.setMaxCorrespondenceDistance(std::atof(argv[4]));
  gicp.setCorrespondenceRandomness(std::atoi(argv[5]));
  gicp.setMaximumOptimizerIterations(std::atoi(argv[6]));
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

struct Result {
  float T[16];
  int converged, outer, inner, evaluations;
  double fitness;
  float aligned0[3];
};

static Result result_of(Reg& r, double fitness, const pcl::PointCloud<PointT>& aligned) {
  Result o;
  const Eigen::Matrix4f T = r.getFinalTransformation();
  for (int a = 0; a < 4; ++a)
    for (int c = 0; c < 4; ++c) o.T[a * 4 + c] = T(a, c);
  o.converged = r.hasConverged() ? 1 : 0;
  r.getIterationCounts(o.outer, o.inner, o.evaluations);
  o.fitness = fitness;
  o.aligned0[0] = aligned.points[0].x; o.aligned0[1] = aligned.points[0].y; o.aligned0[2] = aligned.points[0].z;
  return o;
}

static void print(const char* mode, int i, const Result& o) {
  std::printf("{\"mode\": \"%s\", \"i\": %d, \"converged\": %d, \"outer\": %d, \"inner\": %d, \"evaluations\": %d, \"fitness\": \"%a\", \"aligned0\": \"%a %a %a\", \"T\": \"", mode, i,
              o.converged, o.outer, o.inner, o.evaluations, o.fitness, o.aligned0[0], o.aligned0[1], o.aligned0[2]);
  for (int q = 0; q < 16; ++q) std::printf("%a%s", o.T[q], q == 15 ? "" : " ");
  std::printf("\"}\n");
}

static int best_of(const std::vector<Result>& r) {  // loop_detector.cpp:405-413: the converged candidate of the smallest score
  int best = -1;
  for (int k = 0; k < (int)r.size(); ++k)
    if (r[k].converged && (best < 0 || r[k].fitness < r[best].fitness)) best = k;
  return best;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: %s candidates.bin transformation_epsilon maximum_iterations max_correspondence_distance correspondence_randomness max_optimizer_iterations\n", argv[0]);
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
    if (!c || c->empty() || std::fread(g, 4, 16, f) != 16) return 2;
    Eigen::Matrix4f G;
    for (int r = 0; r < 4; ++r)
      for (int cc = 0; cc < 4; ++cc) G(r, cc) = g[r * 4 + cc];
    sources.push_back(c);
    guesses.push_back(G);
  }
  std::fclose(f);

  try {
    // ---- the reference pattern: one registration object, N aligns and N fitness calls
    std::vector<Result> one_by_one, batched;
    Reg single;
    configure(single, argv);
    single.setInputTarget(target);
    for (int k = 0; k < n_cand; ++k) {
      single.setInputSource(sources[k]);
      pcl::PointCloud<PointT> aligned;
      single.align(aligned, guesses[k]);
      one_by_one.push_back(result_of(single, 0.0, aligned));
      one_by_one.back().fitness = single.getFitnessScore();
      print("single", k, one_by_one.back());
    }

    // ---- the batch surface: N objects on one shared target, one round trip per lock-step round
    std::vector<std::unique_ptr<Reg>> objs;
    std::vector<Reg*> regs;
    for (int k = 0; k < n_cand; ++k) {
      objs.emplace_back(new Reg());
      configure(*objs.back(), argv);
      if (k == 0) objs[0]->setInputTarget(target);
      else objs[k]->setInputTargetShared(*objs[0]);
      objs[k]->setInputSource(sources[k]);
      regs.push_back(objs[k].get());
    }
    std::vector<pcl::PointCloud<PointT>> aligned;
    Reg::alignBatch(regs, guesses, &aligned);
    for (int k = 0; k < n_cand; ++k) batched.push_back(result_of(*regs[k], 0.0, aligned[k]));  // the counts before the score's search
    const std::vector<double> fitness = Reg::getFitnessScoreBatch(regs);
    for (int k = 0; k < n_cand; ++k) {
      batched[k].fitness = fitness[k];
      print("batch", k, batched[k]);
    }
    int rounds = 0, launches = 0;
    gorio_apd_gicp_omp_batch_diag(regs[0]->handle(), &rounds, &launches);
    bool same = true;
    for (int k = 0; k < n_cand; ++k) {
      const Result &a = one_by_one[k], &b = batched[k];
      same = same && std::memcmp(a.T, b.T, sizeof(a.T)) == 0 && a.converged == b.converged && a.outer == b.outer && a.inner == b.inner && a.evaluations == b.evaluations &&
             std::memcmp(&a.fitness, &b.fitness, sizeof(double)) == 0 && std::memcmp(a.aligned0, b.aligned0, sizeof(a.aligned0)) == 0;
    }
    std::printf("{\"best_single\": %d, \"best_batch\": %d, \"bit_identical\": %d, \"rounds\": %d, \"launches\": %d}\n", best_of(one_by_one), best_of(batched), same ? 1 : 0, rounds, launches);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  return 0;
}
