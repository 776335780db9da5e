// gorio::ApproximateVoxelGrid<PointT>: pcl::ApproximateVoxelGrid on the MI355X (libgorio_amd.so), with the members the reference calls
// (preprocessing_nodelet_ntu.cpp:140-145, scan_matching_odometry_nodelet.cpp:150-154, fast_apdgicp/src/python/main.cpp:49-54).
// As with gorio::IterativeClosestPoint, PCL's own class keeps its name; a nodelet's edit is the one line that constructs the filter:
//     auto voxelgrid = new pcl::ApproximateVoxelGrid<PointT>();   ->   auto voxelgrid = new gorio::ApproximateVoxelGrid<PointT>();
// Header-only; every body is a call of include/gorio_prep.h (gorio_prep_approx_voxel_downsample), where the filter is defined -- recalled
// from PCL 1.10, parity unpinned.  No CPU fallback: without a HIP device filter() throws std::runtime_error.
//
// Member -> ABI:  setLeafSize / getLeafSize -> leaf[3] (floats, as PCL stores them); setDownsampleAllData(true, PCL's default) -> the
// field offsets of the point type's float fields (gorio::avg_point_fields), false -> x, y, z only; setInputCloud -> pts / n /
// stride_bytes = sizeof(PointT); filter(output) -> out / out_stride_bytes / out_capacity = n, output.resize(n_out).
// The output has height 1, width = its size and is_dense false, as PCL leaves it; fields that are not averaged (the padding floats,
// and everything but x, y, z with setDownsampleAllData(false)) keep the values of a default-constructed point.
// Deviation (include/gorio_prep.h): a cloud with a non-finite coordinate, or a cell coordinate outside (-2^30, 2^30), is refused:
// filter() throws and leaves the output empty.
#ifndef GORIO_APPROX_VOXEL_GRID_HPP
#define GORIO_APPROX_VOXEL_GRID_HPP

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>

#include <Eigen/Core>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_prep.h>

namespace gorio {

// float offsets of the fields pcl::ApproximateVoxelGrid averages with downsample_all_data_ (every float field of the point), x y z first
template <typename PointT>
struct avg_point_fields;
template <>
struct avg_point_fields<pcl::PointXYZINormal> {  // x y z | normal_x normal_y normal_z | intensity curvature
  static constexpr int count = 8;
  static const int* offsets() {
    static const int o[count] = {0, 1, 2, 4, 5, 6, 8, 9};
    return o;
  }
};
template <>
struct avg_point_fields<pcl::PointXYZI> {  // x y z | intensity
  static constexpr int count = 4;
  static const int* offsets() {
    static const int o[count] = {0, 1, 2, 4};
    return o;
  }
};

template <typename PointT>
class ApproximateVoxelGrid {
public:
  using Vector3f = Eigen::Matrix<float, 3, 1>;  // Eigen::Vector3f
  using PointCloud = pcl::PointCloud<PointT>;
  using PointCloudPtr = typename PointCloud::Ptr;
  using PointCloudConstPtr = typename PointCloud::ConstPtr;
  using Ptr = std::shared_ptr<ApproximateVoxelGrid<PointT>>;
  using ConstPtr = std::shared_ptr<const ApproximateVoxelGrid<PointT>>;

  explicit ApproximateVoxelGrid(int device = 0) : device_(device) {}

  void setLeafSize(const Vector3f& leaf_size) { setLeafSize(leaf_size(0), leaf_size(1), leaf_size(2)); }
  void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx, leaf_[1] = ly, leaf_[2] = lz; }
  Vector3f getLeafSize() const {
    Vector3f v;
    v(0) = leaf_[0], v(1) = leaf_[1], v(2) = leaf_[2];
    return v;
  }
  void setDownsampleAllData(bool downsample) { downsample_all_data_ = downsample; }
  bool getDownsampleAllData() const { return downsample_all_data_; }
  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  PointCloudConstPtr getInputCloud() const { return input_; }

  void filter(PointCloud& output) {
    const int n = input_ ? static_cast<int>(input_->size()) : 0;
    output.points.assign(static_cast<std::size_t>(n), PointT());
    const double leaf[3] = {leaf_[0], leaf_[1], leaf_[2]};
    int n_out = 0;
    const int rc = gorio_prep_approx_voxel_downsample(device_, n ? &input_->points[0].x : nullptr, n, static_cast<int>(sizeof(PointT)), avg_point_fields<PointT>::offsets(),
                                                      downsample_all_data_ ? avg_point_fields<PointT>::count : 3, leaf, n ? &output.points[0].x : nullptr,
                                                      static_cast<int>(sizeof(PointT)), n, &n_out);
    output.points.resize(rc < 0 ? 0 : static_cast<std::size_t>(n_out));
    output.width = static_cast<std::uint32_t>(output.points.size());
    output.height = 1;
    output.is_dense = false;
    if (rc < 0) throw std::runtime_error(std::string("gorio::ApproximateVoxelGrid (gorio_amd): ") + gorio_prep_last_error() + " [code " + std::to_string(rc) + "]");
  }

private:
  int device_;
  float leaf_[3] = {0.0f, 0.0f, 0.0f};  // PCL's constructor: leaf_size_ zero until setLeafSize (the ABI refuses it)
  bool downsample_all_data_ = true;
  PointCloudConstPtr input_;
};

}  // namespace gorio

#endif
