// Drop-in for include/patchworkpp/patchworkpp.hpp of the Go-RIO sources (PWP): Params and PatchWorkpp<PointT> with the reference's
// constructor and estimate_ground signature, on top of the C ABI of include/gorio_ground.h.  The segmentation runs on the GPU; this
// class only gathers whole points into cloud_ground / cloud_nonground in the order the library returns.  What the library refuses
// -- RVPF, num_lpr < 1 or th_seeds <= 0 (a patch could have no seeds), more than 512 patches -- the constructor throws as
// std::runtime_error with the library's text; ego_vel is unused, as in the reference (PWP:761, 784).
#pragma once
#include <chrono>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Core>
#include <pcl/point_cloud.h>

#include "gorio_ground.h"

struct Params {  // PWP:86-168
  bool verbose, enable_RNR, enable_RVPF, enable_TGR;
  int num_iter, num_lpr, num_min_pts, num_zones, num_rings_of_interest;
  double RNR_ver_angle_thr, RNR_intensity_thr;
  double sensor_height, th_seeds, th_dist, th_seeds_v, th_dist_v, max_range, min_range, uprightness_thr, adaptive_seed_selection_margin, intensity_thr;
  std::vector<int> num_sectors_each_zone, num_rings_each_zone;
  int max_flatness_storage, max_elevation_storage;
  std::vector<double> elevation_thr, flatness_thr;

  Params() {
    gorio_ground_params p;
    gorio_ground_default_params(&p);
    verbose = false;
    enable_RNR = p.enable_RNR;
    enable_RVPF = p.enable_RVPF;
    enable_TGR = p.enable_TGR;
    num_iter = p.num_iter;
    num_lpr = p.num_lpr;
    num_min_pts = p.num_min_pts;
    num_zones = 4;
    num_rings_of_interest = GORIO_GROUND_RINGS_OF_INTEREST;
    RNR_ver_angle_thr = p.RNR_ver_angle_thr;
    RNR_intensity_thr = p.RNR_intensity_thr;
    sensor_height = p.sensor_height;
    th_seeds = p.th_seeds;
    th_dist = p.th_dist;
    th_seeds_v = p.th_seeds_v;
    th_dist_v = p.th_dist_v;
    max_range = p.max_range;
    min_range = p.min_range;
    uprightness_thr = p.uprightness_thr;
    adaptive_seed_selection_margin = p.adaptive_seed_selection_margin;
    intensity_thr = 0;
    num_sectors_each_zone.assign(p.num_sectors_each_zone, p.num_sectors_each_zone + 4);
    num_rings_each_zone.assign(p.num_rings_each_zone, p.num_rings_each_zone + 4);
    max_flatness_storage = p.max_flatness_storage;
    max_elevation_storage = p.max_elevation_storage;
    elevation_thr.assign(p.elevation_thr, p.elevation_thr + 4);
    flatness_thr.assign(p.flatness_thr, p.flatness_thr + 4);
  }
};

template <typename PointT>
class PatchWorkpp {
 public:
  PatchWorkpp() : PatchWorkpp(Params()) {}

  explicit PatchWorkpp(Params params, int device = 0) : params_(params) {
    if (params.num_zones != 4 || params.num_sectors_each_zone.size() != 4 || params.num_rings_each_zone.size() != 4)
      throw std::invalid_argument("Some parameters are wrong! Check the num_zones and num_rings/sectors_each_zone");  // PWP:221-223
    if (params.elevation_thr.size() != GORIO_GROUND_RINGS_OF_INTEREST || params.flatness_thr.size() != GORIO_GROUND_RINGS_OF_INTEREST)
      throw std::invalid_argument("elevation_thr and flatness_thr need 4 entries");
    gorio_ground_params p;
    gorio_ground_default_params(&p);
    p.enable_RNR = params.enable_RNR;
    p.enable_RVPF = params.enable_RVPF;
    p.enable_TGR = params.enable_TGR;
    p.num_iter = params.num_iter;
    p.num_lpr = params.num_lpr;
    p.num_min_pts = params.num_min_pts;
    p.RNR_ver_angle_thr = params.RNR_ver_angle_thr;
    p.RNR_intensity_thr = params.RNR_intensity_thr;
    p.sensor_height = params.sensor_height;
    p.th_seeds = params.th_seeds;
    p.th_dist = params.th_dist;
    p.th_seeds_v = params.th_seeds_v;
    p.th_dist_v = params.th_dist_v;
    p.max_range = params.max_range;
    p.min_range = params.min_range;
    p.uprightness_thr = params.uprightness_thr;
    p.adaptive_seed_selection_margin = params.adaptive_seed_selection_margin;
    for (int z = 0; z < 4; ++z) {
      p.num_sectors_each_zone[z] = params.num_sectors_each_zone[z];
      p.num_rings_each_zone[z] = params.num_rings_each_zone[z];
      p.elevation_thr[z] = params.elevation_thr[z];
      p.flatness_thr[z] = params.flatness_thr[z];
    }
    p.max_flatness_storage = params.max_flatness_storage;
    p.max_elevation_storage = params.max_elevation_storage;
    if (gorio_ground_create(&h_, device, &p) != 0) throw std::runtime_error(std::string("gorio_ground_create: ") + gorio_ground_last_error());
  }
  ~PatchWorkpp() { gorio_ground_destroy(h_); }
  PatchWorkpp(const PatchWorkpp&) = delete;
  PatchWorkpp& operator=(const PatchWorkpp&) = delete;

  // PWP:684-890
  void estimate_ground(pcl::PointCloud<PointT> cloud_in, Eigen::Vector3d ego_vel, pcl::PointCloud<PointT>& cloud_ground, pcl::PointCloud<PointT>& cloud_nonground,
                       double& time_taken, int id) {
    (void)ego_vel;
    const auto t0 = std::chrono::steady_clock::now();
    cloud_ground.points.clear();
    cloud_nonground.points.clear();
    const int n = (int)cloud_in.points.size();
    if (n > 0) {
      order_.resize(n);
      int ng = 0, no = 0;
      const PointT& p0 = cloud_in.points[0];
      if (gorio_ground_estimate(h_, &p0.x, &p0.intensity, n, (int)sizeof(PointT), id, order_.data(), &ng, &no) != 0)
        throw std::runtime_error(std::string("gorio_ground_estimate: ") + gorio_ground_last_error());
      cloud_ground.points.reserve(ng);
      cloud_nonground.points.reserve(no - ng);
      for (int i = 0; i < ng; ++i) cloud_ground.points.push_back(cloud_in.points[order_[i]]);
      for (int i = ng; i < no; ++i) cloud_nonground.points.push_back(cloud_in.points[order_[i]]);
    }
    time_taken = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }

  gorio_ground_t* handle() { return h_; }

 private:
  Params params_;
  gorio_ground_t* h_ = nullptr;
  std::vector<int> order_;
};
