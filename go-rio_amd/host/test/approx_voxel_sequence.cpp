// downsample_method APPROX_VOXELGRID through the C++ classes (scan_matching_odometry_nodelet.cpp:150-154, 405-415, 602-618):
//   filter        frame 0 through gorio::ApproximateVoxelGrid<PointXYZINormal>, with all data and with x, y, z only
//   submap_host   the scan-to-submap target from host clouds with setSubmapDownsampleMethod(GORIO_DOWNSAMPLE_APPROX_VOXELGRID)
//   submap_store  the same target from keyframes resident in a gorio::KeyframeStore
//   align         the newest scan against that submap
// Input: frames.bin = [int32 n_frames] then per frame [int32 n][n x (x, y, z, label) float32] (intensity is 5 + label); the last frame
// is the newest scan, the others are the keyframes.  poses.bin = (n_frames - 1) x 16 doubles, row-major rel_pose per keyframe.
// Output: ONE JSON line.  Clouds are printed as their size and the FNV-1a hash of their averaged floats in point order; the first point
// and the pose at 9 significant digits (which identify a float).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <gorio/approx_voxel_grid.hpp>
#include <radar_graph_slam/keyframe_store.hpp>

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;
using Store = gorio::KeyframeStore<PointT>;
using PoseVector = std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>;

static Cloud::Ptr read_cloud(std::FILE* f) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return nullptr;
  std::vector<float> buf((size_t)n * 4);
  if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return nullptr;
  Cloud::Ptr c(new Cloud());
  c->resize(n);
  for (int i = 0; i < n; ++i) {
    PointT& p = c->points[i];
    p.x = buf[4 * i];
    p.y = buf[4 * i + 1];
    p.z = buf[4 * i + 2];
    p.data[3] = 1.0f;
    p.normal_x = buf[4 * i + 3];
    p.intensity = 5.0f + buf[4 * i + 3];
  }
  return c;
}

// FNV-1a over the listed floats of every point, in point order
static std::uint64_t cloud_hash(const Cloud& c, const int* offsets, int count) {
  std::uint64_t h = 1469598103934665603ull;
  for (const PointT& p : c.points) {
    const float* f = &p.x;
    for (int k = 0; k < count; ++k) {
      unsigned char b[4];
      std::memcpy(b, f + offsets[k], 4);
      for (int q = 0; q < 4; ++q) h = (h ^ b[q]) * 1099511628211ull;
    }
  }
  return h;
}

static std::string cloud_json(const Cloud& c, const int* offsets, int count) {
  char buf[512];
  const PointT z;
  const PointT& p = c.points.empty() ? z : c.points[0];
  std::snprintf(buf, sizeof(buf), "{\"n\": %d, \"hash\": \"%016llx\", \"width\": %u, \"height\": %u, \"is_dense\": %d, \"first\": [%.9g, %.9g, %.9g, %.9g, %.9g]}", (int)c.size(),
                (unsigned long long)cloud_hash(c, offsets, count), c.width, c.height, c.is_dense ? 1 : 0, p.x, p.y, p.z, p.normal_x, p.intensity);
  return buf;
}

struct Probe : Reg {  // nr_iterations_ is protected in pcl::Registration
  static int iterations(const Reg& r) { return r.*(&Probe::nr_iterations_); }
};

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s frames.bin poses.bin voxel_leaf\n", argv[0]);
    return 2;
  }
  const double leaf = std::atof(argv[3]);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames < 2) return 2;
  std::vector<Cloud::ConstPtr> frames;
  for (int k = 0; k < n_frames; ++k) {
    Cloud::Ptr c = read_cloud(f);
    if (!c) return 2;
    frames.push_back(c);
  }
  std::fclose(f);
  PoseVector rel(n_frames - 1);
  f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  for (int k = 0; k < n_frames - 1; ++k) {
    double m[16];
    if (std::fread(m, 8, 16, f) != 16) return 2;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) rel[k](r, c) = m[r * 4 + c];
  }
  std::fclose(f);
  const Cloud::ConstPtr newest = frames.back();
  frames.pop_back();
  static const int kAll[8] = {0, 1, 2, 4, 5, 6, 8, 9}, kSubmap[4] = {0, 1, 2, 4};
  try {
    // ---- the filter as the nodelets build it: new ApproximateVoxelGrid, setLeafSize(r, r, r), setInputCloud, filter
    gorio::ApproximateVoxelGrid<PointT> vg;
    vg.setLeafSize((float)leaf, (float)leaf, (float)leaf);
    vg.setInputCloud(frames[0]);
    Cloud all, xyz;
    vg.filter(all);
    const bool default_all = vg.getDownsampleAllData();
    vg.setDownsampleAllData(false);
    gorio::ApproximateVoxelGrid<PointT>::Vector3f aniso;
    aniso(0) = (float)leaf, aniso(1) = 2.0f * (float)leaf, aniso(2) = 4.0f * (float)leaf;
    vg.setLeafSize(aniso);
    vg.filter(xyz);
    const gorio::ApproximateVoxelGrid<PointT>::Vector3f got = vg.getLeafSize();
    // ---- the submap with downsample_method APPROX_VOXELGRID, from host clouds and from the store
    Reg host, kf;
    for (Reg* r : {&host, &kf}) {  // registrations.cpp:38-51 with launch/ntu_loop3.launch:85-96
      r->setNumThreads(0);
      r->setTransformationEpsilon(0.1);
      r->setMaximumIterations(64);
      r->setMaxCorrespondenceDistance(2.0);
      r->setCorrespondenceRandomness(20);
      r->setSubmapDownsampleMethod(GORIO_DOWNSAMPLE_APPROX_VOXELGRID);
    }
    Cloud::ConstPtr sub_host = host.setInputTargetSubmap(frames, rel, leaf);
    Store store;
    std::vector<int> ids;
    for (const Cloud::ConstPtr& c : frames) ids.push_back(store.add(c));
    Cloud::ConstPtr sub_store = kf.setInputTargetSubmap(store, ids, rel, leaf);
    // ---- the newest scan against it
    host.setInputSource(newest);
    Cloud aligned;
    host.align(aligned);
    const Eigen::Matrix4f T = host.getFinalTransformation();
    std::printf("{\"filter\": %s, \"filter_xyz\": %s, \"default_all_data\": %d, \"leaf\": [%.9g, %.9g, %.9g], \"method\": %d, \"submap_host\": %s, \"submap_store\": %s, ",
                cloud_json(all, kAll, 8).c_str(), cloud_json(xyz, kAll, 3).c_str(), default_all ? 1 : 0, got(0), got(1), got(2), host.getSubmapDownsampleMethod(),
                cloud_json(*sub_host, kSubmap, 4).c_str(), cloud_json(*sub_store, kSubmap, 4).c_str());
    std::printf("\"align\": {\"converged\": %d, \"nr_iterations\": %d, \"T\": [", host.hasConverged() ? 1 : 0, Probe::iterations(host));
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b < 4; ++b) std::printf("%.9g%s", T(a, b), (a == 3 && b == 3) ? "" : ", ");
    std::printf("]}}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the classes refuse instead of falling back to a CPU path
  }
  return 0;
}
