// Loop-closure verification (loop_detector.cpp:386-422) with the default registration method, through the drop-in
// pclomp::NormalDistributionsTransform configured by the factory's setter calls (registrations.cpp:120-133), twice:
//   single: ONE object, setInputTarget(keyframe), then per candidate setInputSource, align(*aligned, guess), getFitnessScore();
//   batch:  N objects sharing the target (setInputTargetShared), ONE alignBatch, ONE getFitnessScoreBatch.
// Input: binary [int32 n_cand][int32 n_tgt][n_tgt x (x,y,z,label) float32], then per candidate [int32 n][n x (x,y,z,label) float32]
// [16 float32: guess, row-major]; argv[2] = resolution, argv[3] = DIRECT7 | DIRECT1 | DIRECT26.  Output: one JSON line per candidate and mode.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <pclomp/ndt_omp.h>

using PointT = pcl::PointXYZINormal;
using Reg = pclomp::NormalDistributionsTransform<PointT, PointT>;

static void configure(Reg& ndt, double ndt_resolution, const std::string& nn_search_method) {  // registrations.cpp:120-133
  int num_threads = 0;
  if (num_threads > 0) ndt.setNumThreads(num_threads);
  ndt.setTransformationEpsilon(0.01);
  ndt.setMaximumIterations(64);
  ndt.setResolution(ndt_resolution);
  if (nn_search_method == "KDTREE") ndt.setNeighborhoodSearchMethod(pclomp::KDTREE);
  else if (nn_search_method == "DIRECT1") ndt.setNeighborhoodSearchMethod(pclomp::DIRECT1);
  else if (nn_search_method == "DIRECT26") ndt.setNeighborhoodSearchMethod(pclomp::DIRECT26);
  else ndt.setNeighborhoodSearchMethod(pclomp::DIRECT7);
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

static void print(const char* mode, int i, const Reg& r, double fitness, const pcl::PointCloud<PointT>& aligned) {
  const Eigen::Matrix4f T = r.getFinalTransformation();
  std::printf("{\"mode\": \"%s\", \"i\": %d, \"converged\": %d, \"iterations\": %d, \"probability\": %.17g, \"n_derivatives\": %d, \"n_hessians\": %d, \"n_mt\": %d, "
              "\"score\": %.17g, \"fitness\": %.17g, \"aligned0\": [%.9g, %.9g, %.9g], \"T\": [",
              mode, i, r.hasConverged() ? 1 : 0, r.getFinalNumIteration(), r.getTransformationProbability(), r.getDiagnostics().n_derivatives, r.getDiagnostics().n_hessians,
              r.getDiagnostics().n_mt_iterations, r.getDiagnostics().score, fitness, aligned.points[0].x, aligned.points[0].y, aligned.points[0].z);
  for (int a = 0; a < 4; ++a)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(a, c), (a == 3 && c == 3) ? "" : ", ");
  std::printf("]}\n");
}

static bool same(const Eigen::Matrix4f& a, const Eigen::Matrix4f& b) {
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c)
      if (a(r, c) != b(r, c)) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s candidates.bin resolution DIRECT7|DIRECT1|DIRECT26\n", argv[0]);
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
  const double resolution = std::atof(argv[2]);
  const std::string search = argv[3];

  try {
    // ---- the reference pattern: one registration object, N aligns and N fitness calls
    Reg single;
    configure(single, resolution, search);
    single.setInputTarget(target);
    for (int k = 0; k < n_cand; ++k) {
      single.setInputSource(sources[k]);
      pcl::PointCloud<PointT> aligned;
      single.align(aligned, guesses[k]);
      print("single", k, single, single.getFitnessScore(), aligned);
    }

    // ---- the batch surface: N objects on one shared target, one round trip per evaluation round
    std::vector<std::unique_ptr<Reg>> objs;
    std::vector<Reg*> regs;
    for (int k = 0; k < n_cand; ++k) {
      objs.emplace_back(new Reg());
      configure(*objs.back(), resolution, search);
      if (k == 0) objs[0]->setInputTarget(target);
      else objs[k]->setInputTargetShared(*objs[0]);
      objs[k]->setInputSource(sources[k]);
      regs.push_back(objs[k].get());
    }
    std::vector<pcl::PointCloud<PointT>> aligned;
    Reg::alignBatch(regs, guesses, &aligned);
    const std::vector<double> fitness = Reg::getFitnessScoreBatch(regs);
    for (int k = 0; k < n_cand; ++k) print("batch", k, *regs[k], fitness[k], aligned[k]);

    // ---- errors: a sharer whose resolution does not fit the shared map is refused, and the failed call changes no object
    if (n_cand < 2) return 0;
    const Eigen::Matrix4f before = regs[0]->getFinalTransformation();
    regs[1]->setResolution((float)(resolution * 0.5));
    std::string what;
    try {
      Reg::alignBatch(regs, guesses);
    } catch (const std::runtime_error& e) {
      what = e.what();
    }
    regs[1]->setResolution((float)resolution);
    std::printf("{\"mismatch_error\": \"%s\", \"names_resolution\": %d, \"unchanged\": %d}\n", what.empty() ? "" : "runtime_error",
                what.find("resolution") != std::string::npos ? 1 : 0, same(regs[0]->getFinalTransformation(), before) ? 1 : 0);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU (or KDTREE): the drop-in refuses instead of falling back to a CPU path
  }
  return 0;
}
