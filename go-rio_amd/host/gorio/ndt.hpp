// Drop-in for pcl::NormalDistributionsTransform (pcl/registration/ndt.h), the class select_registration_method hands out for plain
// "NDT" (registrations.cpp:109-115), on top of the C ABI of include/gorio_ndt.h.  PCL's NDT is pclomp's with the KDTREE neighbourhood
// only (ndt_omp's README: "results will be completely the same as that of the original pcl::NDT"): every neighbourhood is
// target_cells_.radiusSearch(x_trans_pt, resolution_) over the leaf centroids.  So this class IS the pclomp drop-in (pclomp/ndt_omp.h) whose
// handle was created with gorio_ndt_set_radius_search on: the same setters, align, getFitnessScore and the same extras -- alignBatch,
// setInputTargetShared, calculateScoreBatch, setInputSourceFromScan / setInputTargetFromScan, setInputTargetSubmap -- and no
// setNeighborhoodSearchMethod, which PCL's class does not have.  The voxel map, the radius search, the derivative sums and the score
// run on the GPU; there is no CPU path (the constructor throws without a HIP device).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include <pclomp/ndt_omp.h>

namespace gorio {

template <typename PointSource, typename PointTarget>
class NormalDistributionsTransform : public pclomp::NormalDistributionsTransform<PointSource, PointTarget> {
  using Omp = pclomp::NormalDistributionsTransform<PointSource, PointTarget>;

 public:
  using Ptr = std::shared_ptr<NormalDistributionsTransform<PointSource, PointTarget>>;
  using ConstPtr = std::shared_ptr<const NormalDistributionsTransform<PointSource, PointTarget>>;
  using Matrix4 = typename pcl::Registration<PointSource, PointTarget>::Matrix4;
  using PointCloudSource = typename pcl::Registration<PointSource, PointTarget>::PointCloudSource;

  NormalDistributionsTransform() {  // pcl/registration/impl/ndt.hpp: the constructor's values are pclomp's (NDT:47-76)
    if (gorio_ndt_set_radius_search(this->handle(), 1) < 0) throw std::runtime_error(std::string("gorio::NormalDistributionsTransform: ") + gorio_ndt_last_error());
  }

  // PCL (and pclomp, NDTH:176-185) spell the outlier ratio's accessors this way
  double getOulierRatio() const { return this->getOutlierRatio(); }
  void setOulierRatio(double outlier_ratio) { this->setOutlierRatio(outlier_ratio); }

  // pcl::NormalDistributionsTransform has no neighbourhood choice: the radius search is what makes this class what it is
  void setNeighborhoodSearchMethod(pclomp::NeighborSearchMethod) = delete;

  // the batch members of the pclomp drop-in for objects of this class (they may be mixed with pclomp objects through Omp pointers)
  static void alignBatch(const std::vector<NormalDistributionsTransform*>& regs, const std::vector<Matrix4>& guesses, std::vector<PointCloudSource>* outputs = nullptr) {
    Omp::alignBatch(std::vector<Omp*>(regs.begin(), regs.end()), guesses, outputs);
  }
  static std::vector<double> calculateScoreBatch(const std::vector<NormalDistributionsTransform*>& regs, const std::vector<Matrix4>& transforms) {
    return Omp::calculateScoreBatch(std::vector<Omp*>(regs.begin(), regs.end()), transforms);
  }
  using Omp::alignBatch;
  using Omp::calculateScoreBatch;
};

}  // namespace gorio
