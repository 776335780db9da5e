// The back end's map publishing (radar_graph_slam_nodelet.cpp:858-878 and :1184) through the drop-in classes: the frames become keyframes
// of a gorio::KeyframeStore, and radar_graph_slam::MapCloudGenerator::generate(store, ids, poses, resolution) is called once per resolution
// given on the command line.
// Input: frames.bin = [int32 n_frames] then per frame [int32 n][n x (x, y, z, label) float32] (intensity is 5 + label), and poses.bin =
// n_frames x 16 float64, row-major 4 x 4.
// Output: per resolution one JSON line with the count and the points' float bits (x, y, z, intensity), the rows sorted.
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <radar_graph_slam/keyframe_store.hpp>
#include <radar_graph_slam/map_cloud_generator.hpp>

using StorePointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<StorePointT>;

static Cloud::Ptr read_cloud(std::FILE* f) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return nullptr;
  std::vector<float> buf((size_t)n * 4);
  if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return nullptr;
  Cloud::Ptr c(new Cloud());
  c->resize(n);
  for (int i = 0; i < n; ++i) {
    StorePointT& p = c->points[i];
    p.x = buf[4 * i];
    p.y = buf[4 * i + 1];
    p.z = buf[4 * i + 2];
    p.data[3] = 1.0f;
    p.normal_x = buf[4 * i + 3];
    p.intensity = 5.0f + buf[4 * i + 3];
  }
  return c;
}

static std::uint32_t bits(float v) {
  std::uint32_t u;
  std::memcpy(&u, &v, 4);
  return u;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s frames.bin poses.bin resolution [resolution ...]\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames <= 0) return 2;
  std::vector<Cloud::Ptr> frames;
  for (int k = 0; k < n_frames; ++k) {
    Cloud::Ptr c = read_cloud(f);
    if (!c) return 2;
    frames.push_back(c);
  }
  std::fclose(f);
  std::vector<Eigen::Isometry3d> poses(n_frames);
  f = std::fopen(argv[2], "rb");
  if (!f) return 2;
  for (int k = 0; k < n_frames; ++k) {
    double T[16];
    if (std::fread(T, 8, 16, f) != 16) return 2;
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) poses[k].matrix()(r, c) = T[4 * r + c];
  }
  std::fclose(f);
  try {
    gorio::KeyframeStore<StorePointT> store;
    radar_graph_slam::MapCloudGenerator generator;
    std::vector<int> ids;
    for (const Cloud::Ptr& c : frames) ids.push_back(store.add(c));
    for (int a = 3; a < argc; ++a) {
      const double resolution = std::atof(argv[a]);
      auto cloud = generator.generate(store, ids, poses, resolution);
      if (!cloud || cloud->width != cloud->size() || cloud->height != 1 || cloud->is_dense) return 4;
      std::vector<std::array<std::uint32_t, 4>> rows;
      for (const auto& p : cloud->points) {
        if (p.data[3] != 1.0f) return 4;
        rows.push_back({bits(p.x), bits(p.y), bits(p.z), bits(p.intensity)});
      }
      std::sort(rows.begin(), rows.end());
      std::printf("{\"resolution\": %.17g, \"n\": %d, \"n_kept\": %d, \"bits\": [", resolution, (int)rows.size(), generator.info().n_kept);
      for (std::size_t i = 0; i < rows.size(); ++i) std::printf("%s[%u, %u, %u, %u]", i ? ", " : "", rows[i][0], rows[i][1], rows[i][2], rows[i][3]);
      std::printf("]}\n");
    }
    if (generator.generate(store, {}, {}, 0.05)) return 4;  // MCG:14-17: nullptr and a warning
    try {
      generator.generate(store, ids, {}, 0.05);
      return 4;
    } catch (const std::invalid_argument&) {
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-ins refuse instead of falling back to a CPU path
  }
  return 0;
}
