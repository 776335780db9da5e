// Drives the three drop-in registrations select_registration_method hands out (registrations.cpp:28-37 FAST_GICP, :38-51 FAST_APDGICP,
// :63-71 FAST_VGICP) through a pcl::Registration base pointer in the nodelet's call order (scan_matching_odometry_nodelet.cpp): set
// target (SMO:430), set source (SMO:442), align (SMO:465), hasConverged / getFinalTransformation (SMO:473-479), getFitnessScore (SMO:675),
// new keyframe (SMO:588).  Afterwards the FastVGICP specials: setInputTarget with the pointer already held (early-out, VG:56-59) and
// swapSourceAndTarget (VG:46-53).
// Input: a binary file [int32 n_frames] then per frame [int32 n][n x (x,y,z,label) float32].  Output: one JSON line per step.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <fast_gicp/gicp/fast_gicp.hpp>
#include <fast_gicp/gicp/fast_vgicp.hpp>

using PointT = pcl::PointXYZINormal;

static pcl::Registration<PointT, PointT>::Ptr select_registration_method(const std::string& registration_method) {  // values of launch/ntu_loop3.launch:85-96
  if (registration_method == "FAST_GICP") {
    std::shared_ptr<fast_gicp::FastGICP<PointT, PointT>> gicp(new fast_gicp::FastGICP<PointT, PointT>());
    gicp->setNumThreads(0);
    gicp->setTransformationEpsilon(0.1);
    gicp->setMaximumIterations(64);
    gicp->setMaxCorrespondenceDistance(2.0);
    gicp->setCorrespondenceRandomness(20);
    return gicp;
  } else if (registration_method == "FAST_APDGICP") {
    std::shared_ptr<fast_gicp::FastAPDGICP<PointT, PointT>> apdgicp(new fast_gicp::FastAPDGICP<PointT, PointT>());
    apdgicp->setNumThreads(0);
    apdgicp->setTransformationEpsilon(0.1);
    apdgicp->setMaximumIterations(64);
    apdgicp->setMaxCorrespondenceDistance(2.0);
    apdgicp->setCorrespondenceRandomness(20);
    apdgicp->setDistVar(0.86);
    apdgicp->setAzimuthVar(0.5);
    apdgicp->setElevationVar(1.0);
    return apdgicp;
  }
  std::shared_ptr<fast_gicp::FastVGICP<PointT, PointT>> vgicp(new fast_gicp::FastVGICP<PointT, PointT>());
  vgicp->setNumThreads(0);
  vgicp->setResolution(1.0);
  vgicp->setTransformationEpsilon(0.1);
  vgicp->setMaximumIterations(64);
  vgicp->setCorrespondenceRandomness(20);
  return vgicp;
}

static void print_step(const char* method, const char* step, int frame, pcl::Registration<PointT, PointT>& reg) {
  const Eigen::Matrix4f T = reg.getFinalTransformation();
  std::printf("{\"method\": \"%s\", \"step\": \"%s\", \"frame\": %d, \"converged\": %d, \"fitness\": %.17g, \"T\": [", method, step, frame, reg.hasConverged() ? 1 : 0, reg.getFitnessScore());
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]}\n");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s frames.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1) return 2;
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

  for (const char* method : {"FAST_GICP", "FAST_APDGICP", "FAST_VGICP"}) {
    pcl::Registration<PointT, PointT>::Ptr registration;
    try {
      registration = select_registration_method(method);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 3;  // no GPU: the drop-ins refuse instead of falling back to a CPU path
    }
    Eigen::Matrix4f prev_trans = Eigen::Matrix4f::Identity();
    registration->setInputTarget(frames[0]);
    for (int k = 1; k < n_frames; ++k) {
      registration->setInputSource(frames[k]);
      pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
      registration->align(*aligned, prev_trans);
      print_step(method, "align", k, *registration);
      if (registration->hasConverged()) prev_trans = registration->getFinalTransformation();
      if (k % 2 == 0) {  // new keyframe
        registration->setInputTarget(frames[k]);
        prev_trans = Eigen::Matrix4f::Identity();
      }
    }
    if (std::strcmp(method, "FAST_VGICP") == 0) {
      auto* vgicp = dynamic_cast<fast_gicp::FastVGICP<PointT, PointT>*>(registration.get());
      // the target pointer already held: an early-out, nothing is uploaded and the voxel map stays (VG:56-59)
      registration->setInputTarget(frames[1]);
      registration->setInputSource(frames[2]);
      pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
      registration->align(*aligned, Eigen::Matrix4f::Identity());
      print_step(method, "fresh_target", 2, *registration);
      const int voxels = vgicp->voxelCount();
      registration->setInputTarget(frames[1]);
      registration->align(*aligned, Eigen::Matrix4f::Identity());
      print_step(method, "same_target_pointer", 2, *registration);
      std::printf("{\"method\": \"%s\", \"step\": \"voxels\", \"before\": %d, \"after\": %d}\n", method, voxels, vgicp->voxelCount());
      vgicp->swapSourceAndTarget();  // VG:46-53: frame 2 is the target now
      registration->align(*aligned, Eigen::Matrix4f::Identity());
      print_step(method, "swapped", 1, *registration);
    }
  }
  return 0;
}
