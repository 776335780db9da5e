// gorio::KeyframeStore<PointT>: the keyframe containers of the nodelets (the `keyframes` of apps/scan_matching_odometry_nodelet.cpp, "SMO",
// and of apps/radar_graph_slam_nodelet.cpp) with the clouds resident on the GPU, on top of the C ABI of include/gorio_keyframes.h.  A
// keyframe is added once -- from a pcl cloud, from the frame a gorio::ScanPreprocessor just produced, or from the source / target a
// registration object holds -- and is then named by its id: FastAPDGICP / FastGICP / FastVGICP::setInputSourceKeyframe,
// setInputTargetKeyframe and setInputTargetSubmap(store, ids, ...), pclomp::NormalDistributionsTransform::setInput*Keyframe and
// SCManager::makeAndSaveScancontextAndKeys(store, id) take it without another upload.
//
// The store keeps the host ConstPtr of every keyframe beside its id, because pcl::Registration::align() insists on input_ / target_ (and
// the nodelets publish and save keyframe clouds from the host).  There is no CPU fallback: without a HIP device the first add throws.
#ifndef GORIO_KEYFRAME_STORE_HPP
#define GORIO_KEYFRAME_STORE_HPP

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_keyframes.h>

namespace gorio {

template <typename PointT>
class KeyframeStore {
 public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudConstPtr = typename Cloud::ConstPtr;

  explicit KeyframeStore(int device = 0) {
    if (gorio_kf_create(&h_, device) != 0) throw std::runtime_error(std::string("gorio_kf_create: ") + gorio_kf_last_error());
  }
  ~KeyframeStore() { gorio_kf_destroy(h_); }
  KeyframeStore(const KeyframeStore&) = delete;
  KeyframeStore& operator=(const KeyframeStore&) = delete;

  // keyframe_cloud = filtered (SMO:481, 586): x, y, z, intensity and normal_x (the cluster label) go to the device once
  int add(const CloudConstPtr& cloud) {
    if (!cloud) throw std::invalid_argument("KeyframeStore::add: null cloud");
    const int n = static_cast<int>(cloud->size());
    const PointT* p = n ? cloud->points.data() : nullptr;
    int id = -1;
    check(gorio_kf_add(h_, p ? p->data : nullptr, p ? &p->intensity : nullptr, p ? &p->normal_x : nullptr, n, static_cast<int>(sizeof(PointT)), &id), "add");
    return remember(id, cloud);
  }
  // the frame a gorio::ScanPreprocessor just produced: the device cloud is shared, nothing is uploaded
  template <typename Preprocessor>
  int addFromScan(Preprocessor& pre) {
    if (!pre.last_scan()) throw std::runtime_error("KeyframeStore::addFromScan: the preprocessor's last process() produced no frame");
    int id = -1;
    check(gorio_kf_add_from_scan(h_, pre.handle(), &id), "addFromScan");
    return remember(id, pre.last_scan());
  }
  // SMO:586-588: the source / target a registration object holds, with the covariances and the search index its last align made
  template <typename Registration>
  int addFromSource(Registration& reg) { return add_from(reg, 0, reg.getInputSource(), "addFromSource"); }
  template <typename Registration>
  int addFromTarget(Registration& reg) { return add_from(reg, 1, reg.getInputTarget(), "addFromTarget"); }

  // the host cloud of a keyframe (kept after release(): the nodelets still publish it); throws std::out_of_range for an id never added
  const CloudConstPtr& cloud(int id) const { return clouds_.at(static_cast<std::size_t>(id)); }
  // keyframes.pop_front(): the store lets go of the device memory; objects that were given the keyframe keep it
  void release(int id) { check(gorio_kf_release(h_, id), "release"); }
  std::size_t size() const { return clouds_.size(); }
  gorio_kf_info_t info(int id) const {
    gorio_kf_info_t i;
    check(gorio_kf_info(h_, id, &i), "info");
    return i;
  }
  gorio_kf_t* handle() { return h_; }

 private:
  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("KeyframeStore::") + what + " (gorio_amd): " + gorio_kf_last_error() + " [code " + std::to_string(rc) + "]");
  }
  template <typename Registration>
  int add_from(Registration& reg, int which, const CloudConstPtr& cloud, const char* what) {
    if (!cloud) throw std::runtime_error(std::string("KeyframeStore::") + what + ": the registration holds no cloud on that side");
    const int n = static_cast<int>(cloud->size());
    int id = -1;
    check(gorio_kf_add_from_apd(h_, reg.handle(), which, n ? &cloud->points[0].intensity : nullptr, static_cast<int>(sizeof(PointT)), &id), what);
    return remember(id, cloud);
  }
  int remember(int id, const CloudConstPtr& cloud) {
    if (id != static_cast<int>(clouds_.size())) throw std::logic_error("KeyframeStore: ids out of step with the library");
    clouds_.push_back(cloud);
    return id;
  }
  gorio_kf_t* h_ = nullptr;
  std::vector<CloudConstPtr> clouds_;
};

}  // namespace gorio
#endif
