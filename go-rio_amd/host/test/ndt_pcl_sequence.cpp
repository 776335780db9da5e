// Drives the drop-in gorio::NormalDistributionsTransform (gorio/ndt.hpp) the way the factory builds plain "NDT"
// (registrations.cpp:111-115: setTransformationEpsilon, setMaximumIterations, setResolution -- no neighbourhood choice) and the way the
// nodelets then use what the factory returned, through a pcl::Registration base pointer (scan_matching_odometry_nodelet.cpp:620-675):
// setInputTarget, setInputSource, align(aligned, guess), hasConverged, getFinalTransformation, getFitnessScore.
// Input: a binary file [int32 n_frames = 2] then per frame [int32 n][n x (x,y,z,label) float32] (target, source); argv[2] = resolution.
// Output: one JSON line with the pose (9 significant digits: the float bits) and the counts.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <gorio/ndt.hpp>

using PointT = pcl::PointXYZINormal;

static pcl::Registration<PointT, PointT>::Ptr select_registration_method(double ndt_resolution) {
  std::shared_ptr<gorio::NormalDistributionsTransform<PointT, PointT>> ndt(new gorio::NormalDistributionsTransform<PointT, PointT>());
  ndt->setTransformationEpsilon(0.01);
  ndt->setMaximumIterations(64);
  ndt->setResolution(ndt_resolution);
  return ndt;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s frames.bin resolution\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames != 2) return 2;
  std::vector<pcl::PointCloud<PointT>::Ptr> frames;
  for (int k = 0; k < n_frames; ++k) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
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
    registration = select_registration_method(std::atof(argv[2]));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  auto* ndt = dynamic_cast<gorio::NormalDistributionsTransform<PointT, PointT>*>(registration.get());
  if (ndt->getOulierRatio() != 0.55 || ndt->getStepSize() != 0.1 || ndt->getResolution() != (float)std::atof(argv[2])) return 4;  // the constructor's values
  registration->setInputTarget(frames[0]);
  registration->setInputSource(frames[1]);
  pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
  registration->align(*aligned, Eigen::Matrix4f::Identity());
  const Eigen::Matrix4f T = registration->getFinalTransformation();
  std::printf("{\"converged\": %d, \"iterations\": %d, \"probability\": %.17g, \"n_derivatives\": %d, \"n_mt\": %d, \"score_aligned\": %.17g, \"fitness\": %.17g, \"T\": [",
              registration->hasConverged() ? 1 : 0, ndt->getFinalNumIteration(), ndt->getTransformationProbability(), ndt->getDiagnostics().n_derivatives,
              ndt->getDiagnostics().n_mt_iterations, ndt->calculateScore(*aligned), registration->getFitnessScore());
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]}\n");
  return 0;
}
