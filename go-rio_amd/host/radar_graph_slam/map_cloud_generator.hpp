// radar_graph_slam::MapCloudGenerator (include/radar_graph_slam/map_cloud_generator.hpp and src/radar_graph_slam/map_cloud_generator.cpp,
// "MCG", of the Go-RIO sources) with the keyframes taken from a gorio::KeyframeStore on the GPU, on top of the C ABI of include/gorio_map.h.
// The reference's generate walks KeyFrameSnapshot objects, each a host cloud and a pose (MCG:13-32); here the clouds are the store's
// keyframes, named by id, and the poses are the snapshot's poses of the moment.  Only the finished map comes back to the host.
// There is no CPU fallback: without a HIP device generate throws.
#ifndef GORIO_MAP_CLOUD_GENERATOR_HPP
#define GORIO_MAP_CLOUD_GENERATOR_HPP

#include <cstddef>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Dense>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_map.h>
#include <radar_graph_slam/keyframe_store.hpp>

namespace radar_graph_slam {

class MapCloudGenerator {
 public:
  using PointT = pcl::PointXYZI;

  explicit MapCloudGenerator(int device = 0) {
    if (gorio_map_create(&h_, device) != 0) throw std::runtime_error(std::string("gorio_map_create: ") + gorio_map_last_error());
  }
  ~MapCloudGenerator() { gorio_map_destroy(h_); }
  MapCloudGenerator(const MapCloudGenerator&) = delete;
  MapCloudGenerator& operator=(const MapCloudGenerator&) = delete;

  // generate(keyframes, resolution), MCG:13-89: ids of `store` in the order the snapshot lists its keyframes, one pose per id.
  // resolution <= 0: every kept point with its intensity (MCG:38-39); otherwise one point per occupied voxel, intensity 0 (MCG:41-50, 84).
  template <typename StorePointT>
  pcl::PointCloud<PointT>::Ptr generate(gorio::KeyframeStore<StorePointT>& store, const std::vector<int>& ids, const std::vector<Eigen::Isometry3d>& poses, double resolution) const {
    if (ids.size() != poses.size()) throw std::invalid_argument("MapCloudGenerator::generate: one pose per keyframe id");
    if (ids.empty()) {
      std::cerr << "warning: keyframes empty!!" << std::endl;  // MCG:14-17
      return nullptr;
    }
    std::vector<double> T(ids.size() * 16);
    for (std::size_t k = 0; k < ids.size(); ++k) {
      const auto& m = poses[k].matrix();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) T[k * 16 + r * 4 + c] = m(r, c);
    }
    int n = 0;
    check(gorio_map_generate(h_, store.handle(), ids.data(), T.data(), static_cast<int>(ids.size()), resolution, &n), "generate");
    pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
    cloud->points.resize(static_cast<std::size_t>(n));  // data[3] = 1 from the constructor
    PointT* p = n ? cloud->points.data() : nullptr;
    check(gorio_map_get(h_, p ? &p->x : nullptr, p ? &p->intensity : nullptr, static_cast<int>(sizeof(PointT)), n), "generate");
    cloud->width = static_cast<std::uint32_t>(cloud->points.size());  // MCG:34-36, 81-83
    cloud->height = 1;
    cloud->is_dense = false;
    return cloud;
  }

  gorio_map_info_t info() const {
    gorio_map_info_t i;
    check(gorio_map_info(h_, &i), "info");
    return i;
  }
  gorio_map_t* handle() const { return h_; }

 private:
  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("MapCloudGenerator::") + what + " (gorio_amd): " + gorio_map_last_error() + " [code " + std::to_string(rc) + "]");
  }
  gorio_map_t* h_ = nullptr;
};

}  // namespace radar_graph_slam
#endif
