// Drives the drop-in fast_gicp::FastGICPMultiPoints through a pcl::Registration base pointer in the call order of the odometry nodelet
// (scan_matching_odometry_nodelet.cpp:430-479): setInputTarget(first frame), and for every later frame setInputSource, align(*aligned,
// guess = the previous transformation), hasConverged, getFinalTransformation.  Then one align on a shared target, and one with another
// radius and regularisation.
// Input: a binary file [int32 n_frames >= 2] then per frame [int32 n][n x (x,y,z,label) float32] (the keyframe first).
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

static void print_align(Mp& mp, pcl::Registration<PointT, PointT>& reg, const pcl::PointCloud<PointT>& aligned) {
  int passes = 0, used = 0;
  long long neighbours = 0;
  mp.getPassCounts(passes, used, neighbours);
  const PointT& a0 = aligned.points[0];
  std::printf("{\"converged\": %d, \"iterations\": %d, \"passes\": %d, \"used\": %d, \"neighbours\": %lld, \"fitness\": %.17g, \"aligned0\": [%.9g, %.9g, %.9g], \"T\": ", reg.hasConverged() ? 1 : 0,
              mp.getNumberOfIterations(), passes, used, neighbours, reg.getFitnessScore(), a0.x, a0.y, a0.z);
  print_pose(reg.getFinalTransformation());
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

  std::shared_ptr<Mp> mp;
  try {
    mp.reset(new Mp());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  try {
    pcl::Registration<PointT, PointT>::Ptr registration = mp;
    std::printf("{\"defaults\": {\"k_correspondences\": %d, \"max_iterations\": %d, \"rotation_epsilon\": %.17g, \"transformation_epsilon\": %.17g, \"regularization\": %d, "
                "\"corr_dist_is_float_max\": %d, \"neighbor_search_radius\": %.17g}, \"aligns\": [",
                mp->getCorrespondenceRandomness(), mp->getMaximumIterations(), mp->getRotationEpsilon(), mp->getTransformationEpsilon(), (int)mp->getRegularizationMethod(),
                mp->getMaxCorrespondenceDistance() == (double)std::numeric_limits<float>::max() ? 1 : 0, mp->getNeighborSearchRadius());
    mp->setNumThreads(8);  // accepted, ignored
    registration->setInputTarget(frames[0]);
    Eigen::Matrix4f prev_trans = Eigen::Matrix4f::Identity();
    for (int k = 1; k < n_frames; ++k) {
      registration->setInputSource(frames[k]);
      pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
      registration->align(*aligned, prev_trans);
      if (k > 1) std::printf(", ");
      print_align(*mp, *registration, *aligned);
      if (registration->hasConverged()) prev_trans = registration->getFinalTransformation();  // SMO:473-479
    }
    std::printf("], \"shared\": ");
    {  // a second object on the first one's target: nothing uploaded or estimated twice
      Mp other;
      other.setInputTargetShared(*mp);
      other.setInputSource(frames[1]);
      pcl::PointCloud<PointT> aligned;
      other.align(aligned);
      print_align(other, other, aligned);
    }
    std::printf(", \"variant\": ");
    {  // the addition and two reference setters
      Mp other;
      other.setNeighborSearchRadius(0.25);
      other.setRegularizationMethod(fast_gicp::RegularizationMethod::FROBENIUS);
      other.setCorrespondenceRandomness(12);
      other.setRotationEpsilon(1e-4);
      other.setTransformationEpsilon(1e-4);
      other.setInputTarget(frames[0]);
      other.setInputSource(frames[1]);
      pcl::PointCloud<PointT> aligned;
      other.align(aligned);
      print_align(other, other, aligned);
    }
    std::printf("}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  return 0;
}
