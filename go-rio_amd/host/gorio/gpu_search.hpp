// gorio::GpuSearch<PointT>: exact k-NN and radius queries against a cloud resident on the GPU, with the batch signatures of
// pcl::search::Search<PointT> (nearestKSearch / radiusSearch over a cloud and an index list), on top of the C ABI of
// include/gorio_search.h.  The cloud comes from a pcl cloud (uploaded once), or is SHARED with a registration object or a keyframe
// store: the same device points and the same index, no upload, no second index.
//
// Results are the ABI's: float squared distances of FLANN L2_Simple, ascending, equal distances in ascending index; a radius neighbour
// has d < float(radius * radius).  max_nn > 0 keeps the first max_nn of that order, which need not be the set PCL's kd-tree returns for
// the same max_nn (include/gorio_search.h).  There is no CPU fallback: without a HIP device the constructor throws.
#ifndef GORIO_GPU_SEARCH_HPP
#define GORIO_GPU_SEARCH_HPP

#include <cstddef>
#include <stdexcept>
#include <string>
#include <vector>

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_search.h>

namespace gorio {

template <typename PointT>
class GpuSearch {
 public:
  using PointCloud = pcl::PointCloud<PointT>;
  using PointCloudConstPtr = typename PointCloud::ConstPtr;

  explicit GpuSearch(int device = 0) {
    if (gorio_search_create(&h_, device) != 0) throw std::runtime_error(std::string("gorio_search_create: ") + gorio_search_last_error());
  }
  ~GpuSearch() { gorio_search_destroy(h_); }
  GpuSearch(const GpuSearch&) = delete;
  GpuSearch& operator=(const GpuSearch&) = delete;

  // pcl::search::Search::setInputCloud: the points go to the device once and the index is built
  void setInputCloud(const PointCloudConstPtr& cloud) {
    if (!cloud) throw std::invalid_argument("GpuSearch::setInputCloud: null cloud");
    const int n = static_cast<int>(cloud->size());
    check(gorio_search_set_cloud(h_, n ? cloud->points[0].data : nullptr, n, static_cast<int>(sizeof(PointT))), "setInputCloud");
    input_ = cloud;
  }
  // the source (which = 0) or target (1) a registration object (FastAPDGICP, FastGICP, FastVGICP, ...) holds now, shared
  template <typename Registration>
  void setInputCloud(Registration& reg, int which) {
    check(gorio_search_set_cloud_from_apd(h_, reg.handle(), which), "setInputCloud(registration)");
    input_ = which == 0 ? reg.getInputSource() : reg.getInputTarget();
  }
  // a keyframe of a gorio::KeyframeStore, shared
  template <typename Store>
  void setInputKeyframe(Store& store, int id) {
    check(gorio_search_set_cloud_from_keyframe(h_, store.handle(), id), "setInputKeyframe");
    input_ = store.cloud(id);
  }
  PointCloudConstPtr getInputCloud() const { return input_; }

  // pcl::search::Search::nearestKSearch(cloud, indices, k, ...): the queries are cloud[indices[i]], or the whole cloud when indices is empty
  void nearestKSearch(const PointCloud& cloud, const std::vector<int>& indices, int k, std::vector<std::vector<int>>& k_indices,
                      std::vector<std::vector<float>>& k_sqr_distances) const {
    const std::vector<float> q = gather(cloud, indices);
    const int nq = static_cast<int>(q.size() / 3);
    // one spare entry: no queries is legal (empty lists, as pcl::search::Search gives), and the ABI wants non-null outputs for any nq
    std::vector<int> idx(static_cast<std::size_t>(nq) * (k > 0 ? k : 0) + 1), cnt(static_cast<std::size_t>(nq) + 1);
    std::vector<float> sqd(idx.size());
    const float one[3] = {0.f, 0.f, 0.f};
    check(gorio_search_knn(h_, nq ? q.data() : one, nq, 12, k, idx.data(), sqd.data(), cnt.data()), "nearestKSearch");
    k_indices.assign(nq, {});
    k_sqr_distances.assign(nq, {});
    for (int i = 0; i < nq; ++i) {
      k_indices[i].assign(idx.begin() + static_cast<std::ptrdiff_t>(i) * k, idx.begin() + static_cast<std::ptrdiff_t>(i) * k + cnt[i]);
      k_sqr_distances[i].assign(sqd.begin() + static_cast<std::ptrdiff_t>(i) * k, sqd.begin() + static_cast<std::ptrdiff_t>(i) * k + cnt[i]);
    }
  }
  // pcl::search::Search::nearestKSearch(point, k, ...): forwards to the batch; returns the number of neighbours
  int nearestKSearch(const PointT& point, int k, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances) const {
    PointCloud one;
    one.points.push_back(point);
    std::vector<std::vector<int>> i;
    std::vector<std::vector<float>> d;
    nearestKSearch(one, std::vector<int>(), k, i, d);
    k_indices.swap(i[0]);
    k_sqr_distances.swap(d[0]);
    return static_cast<int>(k_indices.size());
  }

  // pcl::search::Search::radiusSearch(cloud, indices, radius, ..., max_nn)
  void radiusSearch(const PointCloud& cloud, const std::vector<int>& indices, double radius, std::vector<std::vector<int>>& k_indices,
                    std::vector<std::vector<float>>& k_sqr_distances, unsigned int max_nn = 0) const {
    const std::vector<float> q = gather(cloud, indices);
    const int nq = static_cast<int>(q.size() / 3);
    long long total = 0;
    const float one[3] = {0.f, 0.f, 0.f};
    check(gorio_search_radius(h_, nq ? q.data() : one, nq, 12, radius, static_cast<int>(max_nn), nullptr, &total), "radiusSearch");
    std::vector<long long> offs(static_cast<std::size_t>(nq) + 1);
    std::vector<int> idx(static_cast<std::size_t>(total));
    std::vector<float> sqd(static_cast<std::size_t>(total));
    check(gorio_search_radius_get(h_, offs.data(), idx.data(), sqd.data(), total), "radiusSearch");
    k_indices.assign(nq, {});
    k_sqr_distances.assign(nq, {});
    for (int i = 0; i < nq; ++i) {
      k_indices[i].assign(idx.begin() + offs[i], idx.begin() + offs[i + 1]);
      k_sqr_distances[i].assign(sqd.begin() + offs[i], sqd.begin() + offs[i + 1]);
    }
  }
  int radiusSearch(const PointT& point, double radius, std::vector<int>& k_indices, std::vector<float>& k_sqr_distances, unsigned int max_nn = 0) const {
    PointCloud one;
    one.points.push_back(point);
    std::vector<std::vector<int>> i;
    std::vector<std::vector<float>> d;
    radiusSearch(one, std::vector<int>(), radius, i, d, max_nn);
    k_indices.swap(i[0]);
    k_sqr_distances.swap(d[0]);
    return static_cast<int>(k_indices.size());
  }

  struct Counters {
    long long point_uploads, index_builds, result_downloads;
  };
  Counters counters() const {
    Counters c{0, 0, 0};
    check(gorio_search_get_counters(h_, &c.point_uploads, &c.index_builds, &c.result_downloads), "counters");
    return c;
  }
  gorio_search_t* handle() { return h_; }

 private:
  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("GpuSearch::") + what + " (gorio_amd): " + gorio_search_last_error() + " [code " + std::to_string(rc) + "]");
  }
  static std::vector<float> gather(const PointCloud& cloud, const std::vector<int>& indices) {
    const std::size_t nq = indices.empty() ? cloud.size() : indices.size();
    std::vector<float> q(3 * nq);
    for (std::size_t i = 0; i < nq; ++i) {
      const PointT& p = cloud.points[indices.empty() ? i : static_cast<std::size_t>(indices[i])];
      q[3 * i] = p.x, q[3 * i + 1] = p.y, q[3 * i + 2] = p.z;
    }
    return q;
  }
  gorio_search_t* h_ = nullptr;
  PointCloudConstPtr input_;
};

}  // namespace gorio
#endif
