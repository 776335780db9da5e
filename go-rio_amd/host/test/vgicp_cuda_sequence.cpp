// Drives the drop-in fast_gicp::FastVGICPCuda (fast_gicp/gicp/fast_vgicp_cuda.hpp) through a pcl::Registration base pointer in the nodelet's
// call order (set target, set source, align, hasConverged / getFinalTransformation, getFitnessScore, new keyframe), once per neighbour
// method, with the setter calls of the reference's gicp_test.cpp.  Then the class' specials: swapSourceAndTarget, a changed resolution with
// DIRECT_RADIUS, alignBatch over objects sharing one target.
// Input: a binary file [int32 n_frames] then per frame [int32 n][n x (x,y,z,label) float32].  Output: one JSON line per step.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_vgicp_cuda.hpp>

using PointT = pcl::PointXYZINormal;
using VGICP = fast_gicp::FastVGICPCuda<PointT, PointT>;

static void print_step(const char* mode, const char* step, int frame, pcl::Registration<PointT, PointT>& reg, double fitness) {
  const Eigen::Matrix4f T = reg.getFinalTransformation();
  std::printf("{\"mode\": \"%s\", \"step\": \"%s\", \"frame\": %d, \"converged\": %d, \"fitness\": %.17g, \"T\": [", mode, step, frame, reg.hasConverged() ? 1 : 0, fitness);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.9g%s", T(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]}\n");
}

static fast_gicp::NearestNeighborMethod method_of(const char* mode) {
  if (std::strcmp(mode, "KDTREE") == 0) return fast_gicp::NearestNeighborMethod::CPU_PARALLEL_KDTREE;
  if (std::strcmp(mode, "BRUTEFORCE") == 0) return fast_gicp::NearestNeighborMethod::GPU_BRUTEFORCE;
  return fast_gicp::NearestNeighborMethod::GPU_RBF_KERNEL;
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
  if (n_frames < 3) return 2;

  for (const char* mode : {"KDTREE", "BRUTEFORCE", "RBF"}) {
    std::shared_ptr<VGICP> vgicp;
    try {
      vgicp.reset(new VGICP());
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
    }
    vgicp->setResolution(2.0);
    vgicp->setNearestNeighborSearchMethod(method_of(mode));
    vgicp->setCorrespondenceRandomness(7);  // ignored, as in the reference: k stays 20
    vgicp->setKernelWidth(0.5);             // max_dist = 2.5
    vgicp->setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT7);
    pcl::Registration<PointT, PointT>::Ptr registration = vgicp;
    Eigen::Matrix4f prev_trans = Eigen::Matrix4f::Identity();
    registration->setInputTarget(frames[0]);
    for (int k = 1; k < n_frames; ++k) {
      registration->setInputSource(frames[k]);
      pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
      registration->align(*aligned, prev_trans);
      print_step(mode, "align", k, *registration, vgicp->getFitnessScore());
      if (registration->hasConverged()) prev_trans = registration->getFinalTransformation();
      if (k % 2 == 0) {  // new keyframe
        registration->setInputTarget(frames[k]);
        prev_trans = Eigen::Matrix4f::Identity();
      }
    }
    pcl::PointCloud<PointT>::Ptr aligned(new pcl::PointCloud<PointT>());
    registration->setInputTarget(frames[0]);
    registration->setInputSource(frames[1]);
    registration->align(*aligned, Eigen::Matrix4f::Identity());
    std::printf("{\"mode\": \"%s\", \"step\": \"counts\", \"voxels\": %d, \"kept_source\": %d, \"kept_target\": %d, \"source\": %d, \"target\": %d}\n", mode, vgicp->voxelCount(),
                vgicp->keptCount(0), vgicp->keptCount(1), (int)frames[1]->size(), (int)frames[0]->size());
    vgicp->swapSourceAndTarget();  // VI:69-72: frame 1 is the target now; covariances went with the clouds, its map is built
    registration->align(*aligned, Eigen::Matrix4f::Identity());
    print_step(mode, "swapped", 0, *registration, vgicp->getFitnessScore());
    vgicp->setResolution(1.0);  // rebuilds the map (deviation from VI:41-43, 145)
    vgicp->setRegularizationMethod(fast_gicp::RegularizationMethod::MIN_EIG);
    vgicp->setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT_RADIUS, 1.5);
    registration->align(*aligned, Eigen::Matrix4f::Identity());
    print_step(mode, "radius", 0, *registration, vgicp->getFitnessScore());

    // alignBatch: every later frame against frame 0, held once on the device
    std::vector<std::unique_ptr<VGICP>> objs;
    std::vector<VGICP*> regs;
    std::vector<Eigen::Matrix4f> guesses;
    for (int k = 1; k < n_frames; ++k) {
      objs.emplace_back(new VGICP());
      VGICP& o = *objs.back();
      o.setResolution(2.0);
      o.setNearestNeighborSearchMethod(method_of(mode));
      o.setKernelWidth(0.5);
      o.setNeighborSearchMethod(fast_gicp::NeighborSearchMethod::DIRECT7);
      if (k == 1) o.setInputTarget(frames[0]);
      else o.setInputTargetShared(*objs.front());
      o.setInputSource(frames[k]);
      regs.push_back(&o);
      guesses.push_back(Eigen::Matrix4f::Identity());
    }
    VGICP::alignBatch(regs, guesses);
    const std::vector<double> fit = VGICP::getFitnessScoreBatch(regs);
    for (int k = 1; k < n_frames; ++k) print_step(mode, "batch", k, *regs[k - 1], fit[k - 1]);
  }
  return 0;
}
