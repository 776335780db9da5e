// The Scan Context path of the back end through the drop-in SCManager (scan_context/Scancontext.h): makeAndSaveScancontextAndKeys
// for every keyframe (radar_graph_slam_nodelet.cpp:727-731), then per query keyframe detectLoopClosureID with the given candidate
// list (loop_detector.cpp:116, 192-208), and for every loop found the ICP check of loop_detector.cpp:209-236 with the drop-in
// fast_gicp::FastAPDGICP: all loops aligned in ONE alignBatch, scored in ONE getFitnessScoreBatch against
// historyKeyframeFitnessScore = 6 (loop_detector.cpp:76).
// Input: binary [int32 n_kf], per keyframe [int32 n][n x (x, y, z, intensity) float32], then per keyframe [int32 m][m int32 candidates].
// Output: one JSON line per keyframe: {"q", "loop", "yaw"} and, for a loop, "converged", "fitness", "accepted".
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <scan_context/Scancontext.h>

using PointT = pcl::PointXYZINormal;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;

static void configure(Reg& r) {  // registrations.cpp:38-51 with launch/ntu_loop3.launch:85-96
  r.setNumThreads(0);
  r.setTransformationEpsilon(0.1);
  r.setMaximumIterations(64);
  r.setMaxCorrespondenceDistance(2.0);
  r.setCorrespondenceRandomness(20);
  r.setDistVar(0.86);
  r.setAzimuthVar(0.5);
  r.setElevationVar(1.0);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s sequence.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_kf = 0;
  if (std::fread(&n_kf, 4, 1, f) != 1 || n_kf <= 0) return 2;
  std::vector<pcl::PointCloud<PointT>::Ptr> clouds;
  std::vector<radar_graph_slam::KeyFrame::Ptr> kfs;
  for (int k = 0; k < n_kf; ++k) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<float> buf((size_t)n * 4);
    if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return 2;
    pcl::PointCloud<PointT>::Ptr c(new pcl::PointCloud<PointT>());
    c->resize(n);
    for (int i = 0; i < n; ++i) {
      c->points[i].x = buf[4 * i];
      c->points[i].y = buf[4 * i + 1];
      c->points[i].z = buf[4 * i + 2];
      c->points[i].intensity = buf[4 * i + 3];
    }
    clouds.push_back(c);
    kfs.emplace_back(new radar_graph_slam::KeyFrame());
    kfs.back()->index = k;
  }
  std::vector<std::vector<radar_graph_slam::KeyFrame::Ptr>> cands(n_kf);
  for (int k = 0; k < n_kf; ++k) {
    int m = 0;
    if (std::fread(&m, 4, 1, f) != 1 || m < 0) return 2;
    std::vector<int> c(m);
    if (std::fread(c.data(), 4, m, f) != (size_t)m) return 2;
    for (int i : c) {
      if (i < 0 || i >= n_kf) return 2;
      cands[k].push_back(kfs[i]);
    }
  }
  std::fclose(f);
  try {
    SCManager sc;
    sc.setScDistThresh(0.5);  // launch/ntu_loop3.launch:137-138
    sc.setAzimuthRange(56.5);
    for (int k = 0; k < n_kf; ++k) sc.makeAndSaveScancontextAndKeys(*clouds[k]);
    std::vector<int> loop(n_kf, -1);
    std::vector<float> yaw(n_kf, 0.0f);
    std::vector<std::unique_ptr<Reg>> objs;
    std::vector<Reg*> regs;
    std::vector<int> which;
    for (int k = 0; k < n_kf; ++k) {
      if (cands[k].empty()) continue;  // LD:195-197
      const std::pair<int, float> r = sc.detectLoopClosureID(cands[k], kfs[k]);
      loop[k] = r.first;
      yaw[k] = r.second;
      if (r.first == -1) continue;
      objs.emplace_back(new Reg());
      configure(*objs.back());
      objs.back()->setInputTarget(clouds[r.first]);
      objs.back()->setInputSource(clouds[k]);
      regs.push_back(objs.back().get());
      which.push_back(k);
    }
    std::vector<double> fitness;
    if (!regs.empty()) {
      Reg::alignBatch(regs, std::vector<Reg::Matrix4>(regs.size(), Reg::Matrix4::Identity()));
      fitness = Reg::getFitnessScoreBatch(regs);
    }
    size_t j = 0;
    const float historyKeyframeFitnessScore = 6;
    for (int k = 0; k < n_kf; ++k) {
      std::printf("{\"q\": %d, \"loop\": %d, \"yaw\": %.9g", k, loop[k], yaw[k]);
      if (j < which.size() && which[j] == k) {
        const bool conv = regs[j]->hasConverged();
        std::printf(", \"converged\": %d, \"fitness\": %.17g, \"accepted\": %d", conv ? 1 : 0, fitness[j],
                    (conv && !(fitness[j] > historyKeyframeFitnessScore)) ? 1 : 0);
        ++j;
      }
      std::printf("}\n");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
