// The back end's edge scoring through radar_graph_slam::InformationMatrixCalculator (radar_graph_slam/information_matrix_calculator.hpp)
// over a queue of keyframes held in a gorio::KeyframeStore.  RGS = apps/radar_graph_slam_nodelet.cpp, LD = src/radar_graph_slam/
// loop_detector.cpp of the Go-RIO sources.
//   odometry edges (RGS:585-591): for keyframe k > 0, relative pose odom_k^-1 * odom_{k-1}, information of (cloud_k, cloud_{k-1}),
//                                 (5, 5) = 1.  Once edge by edge ("single"), once as ONE batch ("batch").
//   loop edges (LD:315):          two pairs (newest, 0) and (newest - 1, 1) with the relative pose of their odometry, both ways again.
//   host clouds ("host"):         the same edges through the reference's signatures on pcl clouds (a private store per call).
// Input: binary [int32 n_frames] then per frame [int32 n][16 x float64 odom, row-major][n x (x, y, z, label) float32].
// Output: one JSON line per edge and mode, every float as a hex float; the modes must print the same bits.
//
//   edge_information_sequence --weights score...   no device: prints the information (1 / w_x, 1 / w_q) the library's host arithmetic
//                                                  (csrc/edge_information.h) gives for each score under the default parameters, and
//                                                  under use_const_inf_matrix.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <radar_graph_slam/information_matrix_calculator.hpp>

#include "../../csrc/edge_information.h"

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Calc = radar_graph_slam::InformationMatrixCalculator;
using Store = Calc::Store;

struct Frame {
  Cloud::Ptr cloud;
  double odom[16];
};

static bool read_frame(std::FILE* f, Frame& fr) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return false;
  if (std::fread(fr.odom, 8, 16, f) != 16) return false;
  std::vector<float> buf((size_t)n * 4);
  if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return false;
  fr.cloud.reset(new Cloud());
  fr.cloud->resize(n);
  for (int i = 0; i < n; ++i) {
    PointT& p = fr.cloud->points[i];
    p.x = buf[4 * i];
    p.y = buf[4 * i + 1];
    p.z = buf[4 * i + 2];
    p.data[3] = 1.0f;
    p.normal_x = buf[4 * i + 3];
    p.intensity = 5.0f + buf[4 * i + 3];
  }
  return true;
}

// inverse(a) * b for rigid row-major 4 x 4, element by element (the driver also builds against the minimal Eigen stand-in)
static Eigen::Isometry3d relative(const double* a, const double* b) {
  double inv[16] = {0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) inv[r * 4 + c] = a[c * 4 + r];
  for (int r = 0; r < 3; ++r) inv[r * 4 + 3] = -(inv[r * 4] * a[3] + inv[r * 4 + 1] * a[7] + inv[r * 4 + 2] * a[11]);
  inv[15] = 1.0;
  Eigen::Isometry3d o;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += inv[r * 4 + k] * b[k * 4 + c];
      o.matrix()(r, c) = s;
    }
  return o;
}

static void print_edge(const char* mode, const char* kind, int i, int j, double score, const Eigen::MatrixXd& inf) {
  std::printf("{\"mode\": \"%s\", \"kind\": \"%s\", \"i\": %d, \"j\": %d, \"score\": \"%a\", \"inf\": \"", mode, kind, i, j, score);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) std::printf("%a%s", inf(r, c), (r == 5 && c == 5) ? "" : " ");
  std::printf("\"}\n");
}

static int weights(int argc, char** argv) {
  gorio_inf_params p;
  gorio_kf_default_inf_params(&p);
  gorio_inf_params pc = p;
  pc.use_const_inf_matrix = 1;
  for (int a = 2; a < argc; ++a) {
    const double x = std::strtod(argv[a], nullptr);
    double o[2], oc[2];
    gorio::edge_information_from_score(p, x, o);
    gorio::edge_information_from_score(pc, x, oc);
    std::printf("{\"score\": \"%a\", \"inf_x\": \"%a\", \"inf_q\": \"%a\", \"const_x\": \"%a\", \"const_q\": \"%a\"}\n", x, o[0], o[1], oc[0], oc[1]);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "--weights") == 0) return weights(argc, argv);
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s frames.bin | --weights score...\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames < 4) return 2;
  std::vector<Frame> frames(n_frames);
  for (Frame& fr : frames)
    if (!read_frame(f, fr)) return 2;
  std::fclose(f);
  try {
    const Calc calc;  // the constructor's defaults, as the nodelet (RGS:114)
    Store store;
    std::vector<int> ids;
    for (const Frame& fr : frames) ids.push_back(store.add(fr.cloud));

    struct Job {
      const char* kind;
      int i, j;  // frames: cloud1 = i, cloud2 = j
    };
    std::vector<Job> jobs;
    for (int k = 1; k < n_frames; ++k) jobs.push_back(Job{"odometry", k, k - 1});  // RGS:585-591
    const int last = n_frames - 1;
    jobs.push_back(Job{"loop", last, 0});  // LD:315: (current, previous)
    jobs.push_back(Job{"loop", last - 1, 1});
    jobs.push_back(Job{"loop", 0, last});
    jobs.push_back(Job{"loop", 1, last - 1});
    std::vector<Calc::Edge> edges;
    for (const Job& j : jobs) edges.push_back(Calc::Edge{ids[j.i], ids[j.j], relative(frames[j.i].odom, frames[j.j].odom)});

    auto finish = [](const Job& j, Eigen::MatrixXd inf) {
      if (std::strcmp(j.kind, "odometry") == 0) inf(5, 5) = 1.0;  // RGS:591
      return inf;
    };
    // edge by edge
    for (std::size_t e = 0; e < jobs.size(); ++e) {
      const double s = Calc::calc_fitness_scores(store, std::vector<Calc::Edge>{edges[e]})[0];
      print_edge("single", jobs[e].kind, jobs[e].i, jobs[e].j, s, finish(jobs[e], calc.calc_information_matrix(store, edges[e].id1, edges[e].id2, edges[e].relpose)));
    }
    // one batch
    {
      std::vector<double> scores;
      const std::vector<Eigen::MatrixXd> infs = calc.calc_information_matrices(store, edges, &scores);
      for (std::size_t e = 0; e < jobs.size(); ++e) print_edge("batch", jobs[e].kind, jobs[e].i, jobs[e].j, scores[e], finish(jobs[e], infs[e]));
    }
    // the reference's signatures on host clouds
    for (std::size_t e = 0; e < jobs.size(); ++e) {
      const Cloud::ConstPtr c1 = frames[jobs[e].i].cloud, c2 = frames[jobs[e].j].cloud;
      const double s = Calc::calc_fitness_score(c1, c2, edges[e].relpose);
      print_edge("host", jobs[e].kind, jobs[e].i, jobs[e].j, s, finish(jobs[e], calc.calc_information_matrix(c1, c2, edges[e].relpose)));
    }
    long long calls = 0, scored = 0, builds = 0, syncs = 0;
    gorio_kf_edge_counters(store.handle(), &calls, &scored, &builds, &syncs);
    std::printf("{\"mode\": \"counters\", \"edges\": %d, \"calls\": %lld, \"edges_scored\": %lld, \"index_builds\": %lld, \"synchronisations\": %lld}\n", (int)jobs.size(), calls, scored,
                builds, syncs);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-ins refuse instead of falling back to a CPU path
  }
  return 0;
}
