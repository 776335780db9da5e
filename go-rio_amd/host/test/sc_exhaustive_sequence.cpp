// The exhaustive members of the drop-in SCManager (scan_context/Scancontext.h, include/gorio_sc_pairs.h; an extension, the reference
// has none of them) over sc_sequence's input and keyframe order: makeAndSaveScancontextAndKeys for every keyframe, then per query
// keyframe detectLoopClosureIDExhaustive with the given candidate list.
// Input: binary [int32 n_kf], per keyframe [int32 n][n x (x, y, z, intensity) float32], then per keyframe [int32 m][m int32 candidates].
// Output (doubles as C99 hex floats, so a comparison is exact):
//   default   one JSON line per keyframe {"q", "loop", "yaw", "min_dist"}, then {"best": [[index, dist, shift], ...]} of bestMatches(10),
//             {"pairs": [[dist, shift], ...]} of distanceBtnScanContextBatch over (k, 7 k mod n) and {"matrix": {"dist", "shift"}} of
//             distanceMatrix(first 9 keyframes, last 9 keyframes)
//   --mine    bestMatches(10) turned into loop pairs (dist below SC_DIST_THRES), all aligned in ONE alignBatch and scored in ONE
//             getFitnessScoreBatch against historyKeyframeFitnessScore = 6 (loop_detector.cpp:76, 209-236): one JSON line per pair
//             {"q", "loop", "dist", "yaw", "converged", "fitness", "accepted"}
#include <cmath>
#include <cstdio>
#include <cstring>
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
  bool mine = false;
  const char* path = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--mine"))
      mine = true;
    else
      path = argv[i];
  }
  if (!path) {
    std::fprintf(stderr, "usage: %s [--mine] sequence.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(path, "rb");
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
    const std::vector<SCManager::BestMatch> best = sc.bestMatches(sc.NUM_EXCLUDE_RECENT);
    if (mine) {
      std::vector<std::unique_ptr<Reg>> objs;
      std::vector<Reg*> regs;
      std::vector<int> which;
      for (int k = 0; k < n_kf; ++k) {
        if (best[k].index < 0 || !(best[k].dist < sc.SC_DIST_THRES)) continue;
        objs.emplace_back(new Reg());
        configure(*objs.back());
        objs.back()->setInputTarget(clouds[best[k].index]);
        objs.back()->setInputSource(clouds[k]);
        regs.push_back(objs.back().get());
        which.push_back(k);
      }
      std::vector<double> fitness;
      if (!regs.empty()) {
        Reg::alignBatch(regs, std::vector<Reg::Matrix4>(regs.size(), Reg::Matrix4::Identity()));
        fitness = Reg::getFitnessScoreBatch(regs);
      }
      const float historyKeyframeFitnessScore = 6;
      for (size_t j = 0; j < which.size(); ++j) {
        const int k = which[j];
        const float deg = (float)(best[k].shift * sc.PC_UNIT_SECTOR_ANGLE);  // deg2rad(float degrees) (SC:18-21, 369)
        const float yaw = (float)((double)deg * M_PI / 180.0);
        const bool conv = regs[j]->hasConverged();
        std::printf("{\"q\": %d, \"loop\": %d, \"dist\": \"%a\", \"yaw\": %.9g, \"converged\": %d, \"fitness\": %.17g, \"accepted\": %d}\n", k, best[k].index, best[k].dist, yaw,
                    conv ? 1 : 0, fitness[j], (conv && !(fitness[j] > historyKeyframeFitnessScore)) ? 1 : 0);
      }
      return 0;
    }
    const int counter = sc.tree_making_period_conter;
    for (int k = 0; k < n_kf; ++k) {
      if (cands[k].empty()) continue;  // LD:195-197
      double md = 0.0;
      const std::pair<int, float> r = sc.detectLoopClosureIDExhaustive(cands[k], kfs[k], &md);
      std::printf("{\"q\": %d, \"loop\": %d, \"yaw\": %.9g, \"min_dist\": \"%a\"}\n", k, r.first, r.second, md);
    }
    if (sc.tree_making_period_conter != counter || !sc.polarcontext_invkeys_to_search_.empty()) return 4;  // stateless
    std::printf("{\"best\": [");
    for (int k = 0; k < n_kf; ++k) std::printf("%s[%d, \"%a\", %d]", k ? ", " : "", best[k].index, best[k].dist, best[k].shift);
    std::printf("]}\n");
    std::vector<std::pair<int, int>> pairs;
    for (int k = 0; k < n_kf; ++k) pairs.emplace_back(k, (7 * k) % n_kf);
    const std::vector<std::pair<double, int>> pd = sc.distanceBtnScanContextBatch(pairs);
    std::printf("{\"pairs\": [");
    for (int k = 0; k < n_kf; ++k) std::printf("%s[\"%a\", %d]", k ? ", " : "", pd[k].first, pd[k].second);
    std::printf("]}\n");
    std::vector<int> rows, cols;
    for (int k = 0; k < std::min(9, n_kf); ++k) rows.push_back(k), cols.push_back(n_kf - 1 - k);
    std::vector<double> md;
    std::vector<int> ms;
    sc.distanceMatrix(rows, cols, md, ms);
    std::printf("{\"matrix\": {\"dist\": [");
    for (size_t i = 0; i < md.size(); ++i) std::printf("%s\"%a\"", i ? ", " : "", md[i]);
    std::printf("], \"shift\": [");
    for (size_t i = 0; i < ms.size(); ++i) std::printf("%s%d", i ? ", " : "", ms[i]);
    std::printf("]}}\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
