// Drives the drop-in gorio::IterativeClosestPoint the way the factory and the odometry nodelet do: the setter calls of
// select_registration_method (registrations.cpp:72-79: ICP), then, through a pcl::Registration base pointer, the call order of
// scan_matching_odometry_nodelet.cpp:430-479: setInputTarget(first frame), and for every later frame setInputSource, align(*aligned,
// guess = the previous transformation), hasConverged, getFinalTransformation.  Afterwards the same aligns once more as ONE alignBatch of
// fresh objects on a shared target, compared bit for bit with the singles.
// Input: a binary file [int32 n_frames >= 2] then per frame [int32 n][n x (x,y,z,label) float32] (the keyframe first); argv[2..] = the
// launch parameters reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance,
// reg_use_reciprocal_correspondences.  Output: one JSON line; poses with 9 significant digits (the float bits).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <gorio/icp.hpp>

using PointT = pcl::PointXYZINormal;
using Icp = gorio::IterativeClosestPoint<PointT, PointT>;

static std::shared_ptr<Icp> make_icp(double transformation_epsilon, int maximum_iterations, double max_correspondence_distance, bool use_reciprocal) {
  std::shared_ptr<Icp> icp(new Icp());
  icp->setTransformationEpsilon(transformation_epsilon);
  icp->setMaximumIterations(maximum_iterations);
  icp->setMaxCorrespondenceDistance(max_correspondence_distance);
  icp->setUseReciprocalCorrespondences(use_reciprocal);
  return icp;
}

static pcl::Registration<PointT, PointT>::Ptr select_registration_method(double transformation_epsilon, int maximum_iterations, double max_correspondence_distance, bool use_reciprocal) {
  return make_icp(transformation_epsilon, maximum_iterations, max_correspondence_distance, use_reciprocal);
}

static void print_pose(const Eigen::Matrix4f& T) {
  std::printf("[");
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s frames.bin transformation_epsilon maximum_iterations max_correspondence_distance use_reciprocal_correspondences\n", argv[0]);
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
  const double eps = std::atof(argv[2]), dist = std::atof(argv[4]);
  const int max_it = std::atoi(argv[3]);
  const bool recip = std::atoi(argv[5]) != 0;

  pcl::Registration<PointT, PointT>::Ptr registration;
  try {
    registration = select_registration_method(eps, max_it, dist, recip);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  try {
    Icp* icp = dynamic_cast<Icp*>(registration.get());
    Icp fresh;  // the constructor defaults
    std::printf("{\"defaults\": {\"max_iterations\": %d, \"transformation_epsilon\": %.17g, \"fitness_epsilon_is_lowest\": %d, \"distance_is_sqrt_max\": %d, \"reciprocal\": %d}, \"aligns\": [",
                fresh.getMaximumIterations(), fresh.getTransformationEpsilon(), fresh.getEuclideanFitnessEpsilon() == -std::numeric_limits<double>::max() ? 1 : 0,
                fresh.getMaxCorrespondenceDistance() == std::sqrt(std::numeric_limits<double>::max()) ? 1 : 0, fresh.getUseReciprocalCorrespondences() ? 1 : 0);
    registration->setInputTarget(frames[0]);
    Eigen::Matrix4f prev_trans = Eigen::Matrix4f::Identity();
    std::vector<Eigen::Matrix4f> guesses, finals;
    std::vector<int> states, iterations;
    for (int k = 1; k < n_frames; ++k) {
      registration->setInputSource(frames[k]);
      pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
      guesses.push_back(prev_trans);
      registration->align(*aligned, prev_trans);
      const bool converged = registration->hasConverged();
      const Eigen::Matrix4f T = registration->getFinalTransformation();
      if (converged) prev_trans = T;  // SMO:473-479: an unconverged frame keeps the last transformation
      const auto crit = icp->getConvergeCriteria();
      const PointT& a0 = aligned->points[0];
      std::printf("%s{\"converged\": %d, \"iterations\": %d, \"state\": %d, \"pairs\": %d, \"mse\": %.17g, \"fitness\": %.17g, \"aligned0\": [%.9g, %.9g, %.9g], \"T\": ", k > 1 ? ", " : "",
                  converged ? 1 : 0, icp->getNumberOfIterations(), (int)crit->getConvergenceState(), crit->getCorrespondences(), crit->getMeanSquaredError(), registration->getFitnessScore(), a0.x,
                  a0.y, a0.z);
      print_pose(T);
      std::printf("}");
      finals.push_back(T);
      states.push_back((int)crit->getConvergenceState());
      iterations.push_back(icp->getNumberOfIterations());
    }
    // the same aligns as one batch: fresh objects, the keyframe uploaded once and shared
    std::vector<std::shared_ptr<Icp>> objs;
    std::vector<Icp*> regs;
    for (int k = 1; k < n_frames; ++k) {
      objs.push_back(make_icp(eps, max_it, dist, recip));
      if (k == 1) objs[0]->setInputTarget(frames[0]);
      else objs.back()->setInputTargetShared(*objs[0]);
      objs.back()->setInputSource(frames[k]);
      regs.push_back(objs.back().get());
    }
    std::vector<pcl::PointCloud<PointT>> outputs;
    Icp::alignBatch(regs, guesses, &outputs);
    int equal = 1, rounds = 0, launches = 0, longest = 0;
    for (size_t i = 0; i < regs.size(); ++i) {
      const Eigen::Matrix4f T = regs[i]->getFinalTransformation();
      if (std::memcmp(T.data(), finals[i].data(), sizeof(float) * 16) != 0) equal = 0;
      if ((int)regs[i]->getConvergeCriteria()->getConvergenceState() != states[i] || regs[i]->getNumberOfIterations() != iterations[i]) equal = 0;
      if (outputs[i].size() != frames[i + 1]->size()) equal = 0;
      longest = std::max(longest, std::max(iterations[i], 1));
    }
    regs[0]->getBatchCounts(rounds, launches);
    const std::vector<double> scores = Icp::getFitnessScoreBatch(regs);
    std::printf("], \"batch_equals_singles\": %d, \"rounds\": %d, \"launches\": %d, \"longest\": %d, \"batch_fitness\": [", equal, rounds, launches, longest);
    for (size_t i = 0; i < scores.size(); ++i) std::printf("%s%.17g", i ? ", " : "", scores[i]);
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
