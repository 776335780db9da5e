// The loop-closure shape with the drop-in fast_gicp::FastGICPMultiPoints: N candidate objects on ONE shared target (the first frame), every
// later frame the source of one object, aligned by alignBatch -- and, on fresh objects, by N single aligns.  Both must give the same bits.
// Input: a binary file [int32 n_frames >= 2] then per frame [int32 n][n x (x,y,z,label) float32] (the target first).
// Output: one JSON line; poses with 9 significant digits (the float bits).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/experimental/fast_gicp_mp.hpp>

using PointT = pcl::PointXYZINormal;
using Mp = fast_gicp::FastGICPMultiPoints<PointT, PointT>;

static void print_pose(const Eigen::Matrix4f& T) {
  std::printf("[");
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]");
}

static void print_align(Mp& mp, const pcl::PointCloud<PointT>& aligned, double fitness) {
  int passes = 0, used = 0;
  long long neighbours = 0;
  mp.getPassCounts(passes, used, neighbours);
  const PointT& a0 = aligned.points[0];
  std::printf("{\"converged\": %d, \"iterations\": %d, \"passes\": %d, \"used\": %d, \"neighbours\": %lld, \"fitness\": %.17g, \"aligned0\": [%.9g, %.9g, %.9g], \"T\": ", mp.hasConverged() ? 1 : 0,
              mp.getNumberOfIterations(), passes, used, neighbours, fitness, a0.x, a0.y, a0.z);
  print_pose(mp.getFinalTransformation());
  std::printf("}");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s frames.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames < 2) return 2;
  std::vector<pcl::PointCloud<PointT>::Ptr> frames;
  for (int k = 0; k < n_frames; ++k) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 2;
    std::vector<float> buf((size_t)n * 4);
    if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return 2;
    pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
    c->resize(n);
    for (int i = 0; i < n; ++i) {
      PointT& p = c->points[i];
      p.x = buf[4 * i];
      p.y = buf[4 * i + 1];
      p.z = buf[4 * i + 2];
      p.normal_x = buf[4 * i + 3];
    }
    frames.push_back(c);
  }
  std::fclose(f);
  const int n = n_frames - 1;

  std::vector<std::unique_ptr<Mp>> batch, single;
  try {
    for (int i = 0; i < 2 * n; ++i) (i < n ? batch : single).emplace_back(new Mp());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  try {
    Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
    guess(0, 3) = 0.02f;  // every candidate starts a little off
    for (std::vector<std::unique_ptr<Mp>>* set : {&batch, &single}) {
      (*set)[0]->setInputTarget(frames[0]);
      for (int i = 0; i < n; ++i) {
        if (i > 0) (*set)[i]->setInputTargetShared(*(*set)[0]);
        if (i == n - 1) (*set)[i]->setNeighborSearchRadius(0.25);  // parameters that are not part of the shared covariances may differ
        (*set)[i]->setInputSource(frames[1 + i]);
      }
    }
    std::vector<Mp*> regs;
    for (auto& m : batch) regs.push_back(m.get());
    std::vector<Eigen::Matrix4f> guesses((size_t)n, guess);
    std::vector<pcl::PointCloud<PointT>> outputs;
    Mp::alignBatch(regs, guesses, &outputs);
    const std::vector<double> fit = Mp::getFitnessScoreBatch(regs);
    int rounds = 0, launches = 0, syncs = 0, max_round = 0;
    batch[0]->getBatchCounts(rounds, launches, syncs, max_round);
    std::printf("{\"count\": %d, \"rounds\": %d, \"launches\": %d, \"syncs\": %d, \"max_round_launches\": %d, \"batch\": [", n, rounds, launches, syncs, max_round);
    for (int i = 0; i < n; ++i) {
      if (i) std::printf(", ");
      print_align(*batch[i], outputs[i], fit[i]);
    }
    std::printf("], \"single\": [");
    for (int i = 0; i < n; ++i) {
      pcl::PointCloud<PointT> aligned;
      single[i]->align(aligned, guess);
      if (i) std::printf(", ");
      print_align(*single[i], aligned, single[i]->getFitnessScore());
    }
    // the exception rules of alignBatch
    int invalid = 0, runtime = 0;
    try {
      Mp::alignBatch(regs, std::vector<Eigen::Matrix4f>((size_t)n + 1, guess));
    } catch (const std::invalid_argument&) {
      ++invalid;
    }
    try {
      std::vector<Mp*> with_null = regs;
      with_null[0] = nullptr;
      Mp::alignBatch(with_null, guesses);
    } catch (const std::invalid_argument&) {
      ++invalid;
    }
    try {
      std::vector<Mp*> twice = regs;
      twice.push_back(regs[0]);
      Mp::alignBatch(twice, std::vector<Eigen::Matrix4f>((size_t)n + 1, guess));
    } catch (const std::runtime_error&) {
      ++runtime;
    }
    Mp::alignBatch({}, {});
    std::printf("], \"invalid_argument\": %d, \"runtime_error\": %d}\n", invalid, runtime);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
