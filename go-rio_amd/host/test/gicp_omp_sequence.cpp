// Drives the drop-in pclomp::GeneralizedIterativeClosestPoint the way the factory and the demo do: the setter calls of
// select_registration_method (registrations.cpp:91-100: GICP_OMP), then set target / set source / align of ndt_omp/apps/align.cpp:15-21
// through a pcl::Registration base pointer; afterwards the members of gicp_omp.h:141-260 on the object itself.
// Input: a binary file [int32 n_frames = 2] then per frame [int32 n][n x (x,y,z,label) float32] (target, source); argv[2..] = the launch
// parameters reg_transformation_epsilon, reg_maximum_iterations, reg_max_correspondence_distance, reg_correspondence_randomness,
// reg_max_optimizer_iterations.  Output: one JSON line with the pose (9 significant digits: the float bits) and the counts.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <pclomp/gicp_omp.h>

using PointT = pcl::PointXYZINormal;

static pcl::Registration<PointT, PointT>::Ptr select_registration_method(double transformation_epsilon, int maximum_iterations, double max_correspondence_distance,
                                                                         int correspondence_randomness, int max_optimizer_iterations) {
  std::shared_ptr<pclomp::GeneralizedIterativeClosestPoint<PointT, PointT>> gicp(new pclomp::GeneralizedIterativeClosestPoint<PointT, PointT>());
  gicp->setTransformationEpsilon(transformation_epsilon);
  gicp->setMaximumIterations(maximum_iterations);
  gicp->setUseReciprocalCorrespondences(false);
  gicp->setMaxCorrespondenceDistance(max_correspondence_distance);
  gicp->setCorrespondenceRandomness(correspondence_randomness);
  gicp->setMaximumOptimizerIterations(max_optimizer_iterations);
  return gicp;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    std::fprintf(stderr, "usage: %s frames.bin transformation_epsilon maximum_iterations max_correspondence_distance correspondence_randomness max_optimizer_iterations\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames != 2) return 2;
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

  pcl::Registration<PointT, PointT>::Ptr registration;
  try {
    registration = select_registration_method(std::atof(argv[2]), std::atoi(argv[3]), std::atof(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  try {
    registration->setInputTarget(frames[0]);
    registration->setInputSource(frames[1]);
    pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
    registration->align(*aligned);
    auto* gicp = dynamic_cast<pclomp::GeneralizedIterativeClosestPoint<PointT, PointT>*>(registration.get());
    int outer = 0, inner = 0, evals = 0;
    gicp->getIterationCounts(outer, inner, evals);
    const Eigen::Matrix4f T = registration->getFinalTransformation();
    const Eigen::Matrix4f M0 = gicp->mahalanobis(0);
    const PointT& a0 = aligned->points[0];
    std::printf("{\"converged\": %d, \"outer\": %d, \"inner\": %d, \"evaluations\": %d, \"k\": %d, \"max_inner\": %d, \"rotation_epsilon\": %.17g, \"fitness\": %.17g, \"aligned0\": [%.9g, %.9g, %.9g], \"m00\": %.9g, \"T\": [",
                registration->hasConverged() ? 1 : 0, outer, inner, evals, gicp->getCorrespondenceRandomness(), gicp->getMaximumOptimizerIterations(), gicp->getRotationEpsilon(),
                registration->getFitnessScore(), a0.x, a0.y, a0.z, M0(0, 0));
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
    std::printf("]}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
