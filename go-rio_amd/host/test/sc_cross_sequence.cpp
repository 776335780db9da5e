// The cross-database members of the drop-in SCManager (scan_context/Scancontext.h, include/gorio_sc_cross.h; an extension, the
// reference has none of them): two SCManagers filled from the two sessions of a sequence file, every keyframe of session 2 matched
// against the whole of session 1.
// Input: binary [int32 n1][int32 n2], then per keyframe of session 1 and then of session 2 [int32 n][n x (x, y, z, intensity) float32].
// Output (doubles as C99 hex floats, so a comparison is exact):
//   default   one JSON line per keyframe of session 2 {"q", "top": [[index, dist, shift], ...]} of topMatches(db = session 1, k = 3),
//             then {"pairs": [[dist, shift], ...]} of distanceBtnScanContextBatch(session 1, (k, 5 k mod n1)), {"matrix": {"dist", "shift"}}
//             of distanceMatrix(session 1, first 9 of session 2, last 9 of session 1), {"detect": [[loop, yaw, min_dist], ...]} of
//             detectLoopClosureIDAgainst(session 1, {n1 - 1, ..., 0}, q) per keyframe and {"triangle": [[[index, dist, shift], ...], ...]}
//             of session 1's topMatches(2, 10)
//   --mine    the entries of the top lists below SC_DIST_THRES become loop pairs, all aligned in ONE alignBatch and scored in ONE
//             getFitnessScoreBatch against historyKeyframeFitnessScore = 6 (loop_detector.cpp:76, 209-236): one JSON line per pair
//             {"q", "loop", "rank", "dist", "yaw", "converged", "fitness", "accepted"}
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

static void print_list(const std::vector<SCManager::BestMatch>& l) {
  std::printf("[");
  for (size_t j = 0; j < l.size(); ++j) std::printf("%s[%d, \"%a\", %d]", j ? ", " : "", l[j].index, l[j].dist, l[j].shift);
  std::printf("]");
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
    std::fprintf(stderr, "usage: %s [--mine] sessions.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  int n1 = 0, n2 = 0;
  if (std::fread(&n1, 4, 1, f) != 1 || std::fread(&n2, 4, 1, f) != 1 || n1 <= 0 || n2 <= 0) return 2;
  std::vector<pcl::PointCloud<PointT>::Ptr> clouds;
  for (int k = 0; k < n1 + n2; ++k) {
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
  }
  std::fclose(f);
  try {
    SCManager old_session, session;
    for (SCManager* m : {&old_session, &session}) {
      m->setScDistThresh(0.5);  // launch/ntu_loop3.launch:137-138
      m->setAzimuthRange(56.5);
    }
    for (int k = 0; k < n1; ++k) old_session.makeAndSaveScancontextAndKeys(*clouds[k]);
    for (int k = 0; k < n2; ++k) session.makeAndSaveScancontextAndKeys(*clouds[n1 + k]);
    std::vector<int> every(n2);
    for (int k = 0; k < n2; ++k) every[k] = k;
    const std::vector<std::vector<SCManager::BestMatch>> top = session.topMatches(old_session, every, {}, 3);
    if (mine) {
      std::vector<std::unique_ptr<Reg>> objs;
      std::vector<Reg*> regs;
      std::vector<std::pair<int, int>> which;  // (keyframe of session 2, rank)
      for (int k = 0; k < n2; ++k)
        for (size_t j = 0; j < top[k].size(); ++j) {
          if (!(top[k][j].dist < session.SC_DIST_THRES)) continue;
          objs.emplace_back(new Reg());
          configure(*objs.back());
          objs.back()->setInputTarget(clouds[top[k][j].index]);
          objs.back()->setInputSource(clouds[n1 + k]);
          regs.push_back(objs.back().get());
          which.emplace_back(k, (int)j);
        }
      std::vector<double> fitness;
      if (!regs.empty()) {
        Reg::alignBatch(regs, std::vector<Reg::Matrix4>(regs.size(), Reg::Matrix4::Identity()));
        fitness = Reg::getFitnessScoreBatch(regs);
      }
      const float historyKeyframeFitnessScore = 6;
      for (size_t p = 0; p < which.size(); ++p) {
        const SCManager::BestMatch& b = top[which[p].first][which[p].second];
        const float deg = (float)(b.shift * session.PC_UNIT_SECTOR_ANGLE);  // deg2rad(float degrees) (SC:18-21, 369)
        const float yaw = (float)((double)deg * M_PI / 180.0);
        const bool conv = regs[p]->hasConverged();
        std::printf("{\"q\": %d, \"loop\": %d, \"rank\": %d, \"dist\": \"%a\", \"yaw\": %.9g, \"converged\": %d, \"fitness\": %.17g, \"accepted\": %d}\n", which[p].first, b.index,
                    which[p].second, b.dist, yaw, conv ? 1 : 0, fitness[p], (conv && !(fitness[p] > historyKeyframeFitnessScore)) ? 1 : 0);
      }
      return 0;
    }
    for (int k = 0; k < n2; ++k) {
      std::printf("{\"q\": %d, \"top\": ", k);
      print_list(top[k]);
      std::printf("}\n");
    }
    std::vector<std::pair<int, int>> pairs;
    for (int k = 0; k < n2; ++k) pairs.emplace_back(k, (5 * k) % n1);
    const std::vector<std::pair<double, int>> pd = session.distanceBtnScanContextBatch(old_session, pairs);
    std::printf("{\"pairs\": [");
    for (int k = 0; k < n2; ++k) std::printf("%s[\"%a\", %d]", k ? ", " : "", pd[k].first, pd[k].second);
    std::printf("]}\n");
    std::vector<int> rows, cols;
    for (int k = 0; k < std::min(9, n2); ++k) rows.push_back(k);
    for (int k = 0; k < std::min(9, n1); ++k) cols.push_back(n1 - 1 - k);
    std::vector<double> md;
    std::vector<int> ms;
    session.distanceMatrix(old_session, rows, cols, md, ms);
    std::printf("{\"matrix\": {\"dist\": [");
    for (size_t i = 0; i < md.size(); ++i) std::printf("%s\"%a\"", i ? ", " : "", md[i]);
    std::printf("], \"shift\": [");
    for (size_t i = 0; i < ms.size(); ++i) std::printf("%s%d", i ? ", " : "", ms[i]);
    std::printf("]}}\n");
    std::vector<int> backwards(n1);
    for (int k = 0; k < n1; ++k) backwards[k] = n1 - 1 - k;
    std::printf("{\"detect\": [");
    for (int k = 0; k < n2; ++k) {
      double dmin = 0.0;
      const std::pair<int, float> r = session.detectLoopClosureIDAgainst(old_session, backwards, k, &dmin);
      std::printf("%s[%d, %.9g, \"%a\"]", k ? ", " : "", r.first, r.second, dmin);
    }
    std::printf("]}\n");
    const std::vector<std::vector<SCManager::BestMatch>> tri = old_session.topMatches(2, old_session.NUM_EXCLUDE_RECENT);
    std::printf("{\"triangle\": [");
    for (int k = 0; k < n1; ++k) {
      std::printf("%s", k ? ", " : "");
      print_list(tri[k]);
    }
    std::printf("]}\n");
    if (session.tree_making_period_conter != 0 || old_session.tree_making_period_conter != 0) return 4;  // stateless
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  return 0;
}
