// radar_graph_slam::InformationMatrixCalculator (include/radar_graph_slam/information_matrix_calculator.hpp and
// src/radar_graph_slam/information_matrix_calculator.cpp, "IMC", of the Go-RIO sources) on top of the C ABI of include/gorio_kf_edges.h.
// The reference builds a kd-tree over one keyframe's host cloud per edge (IMC:55-86); here the two clouds are keyframes of a
// gorio::KeyframeStore on the GPU, named by id, and the N edges of a keyframe queue (apps/radar_graph_slam_nodelet.cpp:585-591) or of a
// round of accepted loops (src/radar_graph_slam/loop_detector.cpp:315) are scored in ONE call.
//
//   reference signatures   calc_fitness_score(cloud1, cloud2, relpose, max_range) and calc_information_matrix(cloud1, cloud2, relpose) on
//                          host clouds: a private store, two uploads, one edge, release.  For code that has not moved to ids yet.
//   store forms            calc_information_matrix(store, id1, id2, relpose), and calc_information_matrices / calc_fitness_scores for a
//                          batch.  The store is taken by non-const reference: the call builds the keyframes' search indexes in it.
//
// Parameters, their defaults and the returned 6 x 6 matrix (IMC:47-49) are the reference's.  No ROS dependency: the class is built from
// a plain Params struct, and the reference's templated load(ParamServer&) is there for a node handle.  There is no CPU fallback: without
// a HIP device every scoring call throws (the use_const_inf_matrix branch needs none, as in the reference).
#ifndef GORIO_INFORMATION_MATRIX_CALCULATOR_HPP
#define GORIO_INFORMATION_MATRIX_CALCULATOR_HPP

#include <cstddef>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include <Eigen/Dense>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <gorio_keyframes.h>
#include <radar_graph_slam/keyframe_store.hpp>

namespace radar_graph_slam {

class InformationMatrixCalculator {
 public:
  using PointT = pcl::PointXYZINormal;
  using Store = gorio::KeyframeStore<PointT>;

  // the members of the reference, with the defaults of its constructor (IMC:15-24)
  struct Params {
    bool use_const_inf_matrix = false;
    double const_stddev_x = 0.5;
    double const_stddev_q = 0.1;
    double var_gain_a = 20.0;
    double min_stddev_x = 0.1;
    double max_stddev_x = 5.0;
    double min_stddev_q = 0.05;
    double max_stddev_q = 0.2;
    double fitness_score_thresh = 0.5;
  };
  // one edge of a batch: cloud1 (gets the kd-tree in the reference), cloud2 (moved by relpose)
  struct Edge {
    int id1;
    int id2;
    Eigen::Isometry3d relpose;
  };

  InformationMatrixCalculator() { set(Params()); }
  explicit InformationMatrixCalculator(const Params& p) { set(p); }
  ~InformationMatrixCalculator() {}

  // the reference's load(): every member from a parameter server (ros::NodeHandle::param), with the defaults of ITS header -- the
  // constructor's, except fitness_score_thresh = 2.5
  template <typename ParamServer>
  void load(ParamServer& params) {
    Params d;
    d.fitness_score_thresh = 2.5;
    use_const_inf_matrix = params.template param<bool>("use_const_inf_matrix", d.use_const_inf_matrix);
    const struct {
      const char* name;
      double* member;
      double fallback;
    } doubles[] = {{"const_stddev_x", &const_stddev_x, d.const_stddev_x}, {"const_stddev_q", &const_stddev_q, d.const_stddev_q}, {"var_gain_a", &var_gain_a, d.var_gain_a},
                   {"min_stddev_x", &min_stddev_x, d.min_stddev_x},       {"max_stddev_x", &max_stddev_x, d.max_stddev_x},       {"min_stddev_q", &min_stddev_q, d.min_stddev_q},
                   {"max_stddev_q", &max_stddev_q, d.max_stddev_q},       {"fitness_score_thresh", &fitness_score_thresh, d.fitness_score_thresh}};
    for (const auto& e : doubles) *e.member = params.template param<double>(e.name, e.fallback);
  }
  // ---- the reference's signatures, on host clouds
  static double calc_fitness_score(const pcl::PointCloud<PointT>::ConstPtr& cloud1, const pcl::PointCloud<PointT>::ConstPtr& cloud2, const Eigen::Isometry3d& relpose,
                                   double max_range = std::numeric_limits<double>::max()) {
    Store store;
    const int id1 = store.add(cloud1), id2 = store.add(cloud2);
    const double s = calc_fitness_scores(store, std::vector<Edge>{Edge{id1, id2, relpose}}, max_range)[0];
    store.release(id1);
    store.release(id2);
    return s;
  }
  Eigen::MatrixXd calc_information_matrix(const pcl::PointCloud<PointT>::ConstPtr& cloud1, const pcl::PointCloud<PointT>::ConstPtr& cloud2, const Eigen::Isometry3d& relpose) const {
    if (use_const_inf_matrix) return matrix(1.0 / const_stddev_x, 1.0 / const_stddev_q);  // IMC:30-35: neither cloud is looked at
    Store store;
    const int id1 = store.add(cloud1), id2 = store.add(cloud2);
    Eigen::MatrixXd inf = calc_information_matrix(store, id1, id2, relpose);
    store.release(id1);
    store.release(id2);
    return inf;
  }

  // ---- the same on keyframes of a store
  Eigen::MatrixXd calc_information_matrix(Store& store, int id1, int id2, const Eigen::Isometry3d& relpose) const {
    return calc_information_matrices(store, std::vector<Edge>{Edge{id1, id2, relpose}})[0];
  }
  // all edges in one call of the library; fitness_scores (optional) receives calc_fitness_score of every edge
  std::vector<Eigen::MatrixXd> calc_information_matrices(Store& store, const std::vector<Edge>& edges, std::vector<double>* fitness_scores = nullptr) const {
    const std::vector<gorio_kf_edge> tab = table(edges);
    gorio_inf_params p;
    p.use_const_inf_matrix = use_const_inf_matrix ? 1 : 0;
    p.const_stddev_x = const_stddev_x;
    p.const_stddev_q = const_stddev_q;
    p.var_gain_a = var_gain_a;
    p.min_stddev_x = min_stddev_x;
    p.max_stddev_x = max_stddev_x;
    p.min_stddev_q = min_stddev_q;
    p.max_stddev_q = max_stddev_q;
    p.fitness_score_thresh = fitness_score_thresh;
    std::vector<double> diag(2 * edges.size()), score(edges.size(), 0.0);
    check(gorio_kf_edge_information(store.handle(), &p, tab.data(), static_cast<int>(tab.size()), diag.data(), score.data()), "calc_information_matrices");
    std::vector<Eigen::MatrixXd> out;
    out.reserve(edges.size());
    for (std::size_t e = 0; e < edges.size(); ++e) out.push_back(matrix(diag[2 * e], diag[2 * e + 1]));
    if (fitness_scores) *fitness_scores = score;
    return out;
  }
  static std::vector<double> calc_fitness_scores(Store& store, const std::vector<Edge>& edges, double max_range = std::numeric_limits<double>::max()) {
    const std::vector<gorio_kf_edge> tab = table(edges);
    std::vector<double> score(edges.size(), 0.0);
    check(gorio_kf_edge_fitness(store.handle(), tab.data(), static_cast<int>(tab.size()), max_range, score.data(), nullptr), "calc_fitness_scores");
    return score;
  }

 private:
  void set(const Params& p) {
    use_const_inf_matrix = p.use_const_inf_matrix;
    const_stddev_x = p.const_stddev_x;
    const_stddev_q = p.const_stddev_q;
    var_gain_a = p.var_gain_a;
    min_stddev_x = p.min_stddev_x;
    max_stddev_x = p.max_stddev_x;
    min_stddev_q = p.min_stddev_q;
    max_stddev_q = p.max_stddev_q;
    fitness_score_thresh = p.fitness_score_thresh;
  }
  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("InformationMatrixCalculator::") + what + " (gorio_amd): " + gorio_kf_last_error() + " [code " + std::to_string(rc) + "]");
  }
  static std::vector<gorio_kf_edge> table(const std::vector<Edge>& edges) {
    std::vector<gorio_kf_edge> tab(edges.size());
    for (std::size_t e = 0; e < edges.size(); ++e) {
      tab[e].target_id = edges[e].id1;
      tab[e].source_id = edges[e].id2;
      const auto& m = edges[e].relpose.matrix();
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) tab[e].relpose[r * 4 + c] = m(r, c);
    }
    return tab;
  }
  // Identity(6, 6) with the top-left block divided by w_x and the bottom-right one by w_q (IMC:47-49), given the two quotients
  static Eigen::MatrixXd matrix(double inf_x, double inf_q) {
    Eigen::MatrixXd inf = Eigen::MatrixXd::Zero(6, 6);
    for (int i = 0; i < 3; ++i) {
      inf(i, i) = inf_x;
      inf(3 + i, 3 + i) = inf_q;
    }
    return inf;
  }

  bool use_const_inf_matrix;
  double const_stddev_x, const_stddev_q, var_gain_a, min_stddev_x, max_stddev_x, min_stddev_q, max_stddev_q, fitness_score_thresh;
};

}  // namespace radar_graph_slam

#endif  // GORIO_INFORMATION_MATRIX_CALCULATOR_HPP
