// Drop-in for the reference's fast_gicp/gicp/fast_vgicp.hpp (VGH:20-92) backed by the MI355X library libgorio_amd.so:
// FastGICP (fast_gicp.hpp) whose handle runs GORIO_METHOD_VGICP.  registrations.cpp:63-71 compiles unchanged against it.
// The Gaussian voxel map lives on the device with the target cloud: it is dropped whenever the target or its covariances change
// (voxelmap_.reset() of VG:50, 62) and reused otherwise (the reference rebuilds an equal map at every computeTransformation, VG:66-70).
#ifndef FAST_GICP_FAST_VGICP_HPP
#define FAST_GICP_FAST_VGICP_HPP

#include <fast_gicp/gicp/fast_gicp.hpp>
#include <fast_gicp/gicp/gicp_settings.hpp>

namespace fast_gicp {

template <typename PointSource, typename PointTarget>
class FastVGICP : public FastGICP<PointSource, PointTarget> {
public:
  using Scalar = float;
  using Matrix4 = typename pcl::Registration<PointSource, PointTarget, Scalar>::Matrix4;
  using PointCloudSource = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudSource;
  using PointCloudSourcePtr = typename PointCloudSource::Ptr;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = typename pcl::Registration<PointSource, PointTarget, Scalar>::PointCloudTarget;
  using PointCloudTargetPtr = typename PointCloudTarget::Ptr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
#if PCL_VERSION >= PCL_VERSION_CALC(1, 10, 0)
  using Ptr = pcl::shared_ptr<FastVGICP<PointSource, PointTarget>>;
  using ConstPtr = pcl::shared_ptr<const FastVGICP<PointSource, PointTarget>>;
#else
  using Ptr = boost::shared_ptr<FastVGICP<PointSource, PointTarget>>;
  using ConstPtr = boost::shared_ptr<const FastVGICP<PointSource, PointTarget>>;
#endif

protected:
  using pcl::Registration<PointSource, PointTarget, Scalar>::input_;
  using pcl::Registration<PointSource, PointTarget, Scalar>::target_;

public:
  explicit FastVGICP(int device = 0) : FastGICP<PointSource, PointTarget>(device) {  // VG:19-25
    this->reg_name_ = "FastVGICP";
    voxel_resolution_ = 1.0;
    search_method_ = NeighborSearchMethod::DIRECT1;
    voxel_mode_ = VoxelAccumulationMode::ADDITIVE;
  }
  virtual ~FastVGICP() override {}

  void setResolution(double resolution) { voxel_resolution_ = resolution; }                    // VG:31
  void setVoxelAccumulationMode(VoxelAccumulationMode mode) { voxel_mode_ = mode; }            // VG:41
  void setNeighborSearchMethod(NeighborSearchMethod method) { search_method_ = method; }       // VG:36

  // VG:46-53: clouds and covariances change sides; the voxel map of the old target goes with its cloud (gorio_apd_swap_source_and_target)
  virtual void swapSourceAndTarget() override { FastGICP<PointSource, PointTarget>::swapSourceAndTarget(); }
  // VG:56-63: the same pointer again is a no-op (the map stays); a new target drops the map with the cloud it was built from
  virtual void setInputTarget(const PointCloudTargetConstPtr& cloud) override {
    if (target_ == cloud) return;
    FastGICP<PointSource, PointTarget>::setInputTarget(cloud);
  }
  // parity hook: number of voxels of the map (builds it when stale), gorio_apd_get_voxelmap
  int voxelCount() {
    push_method();
    int nv = 0;
    this->check(gorio_apd_get_voxelmap(this->handle(), nullptr, nullptr, nullptr, nullptr, 0, &nv));
    return nv;
  }

protected:
  virtual void push_method() override {  // setResolution / setNeighborSearchMethod / setVoxelAccumulationMode -> gorio_apd_set_method
    this->check(this->select_method(GORIO_METHOD_VGICP, voxel_resolution_, static_cast<int>(search_method_), static_cast<int>(voxel_mode_)));
  }

  double voxel_resolution_;
  NeighborSearchMethod search_method_;
  VoxelAccumulationMode voxel_mode_;
};
}  // namespace fast_gicp

#endif
