// Drop-in for include/scan_context/Scancontext.h of the Go-RIO sources (SCH, with SC = src/radar_graph_slam/Scancontext.cpp):
// SCManager with the reference's surface, on top of the C ABI of include/gorio_sc.h.  makeAndSaveScancontextAndKeys and
// detectLoopClosureID run on the GPU against the library's keyframe database; the storage members mirror it on the host for
// callers that read them.  makeScancontext(cloud) goes through a second, private database.  The helpers that take caller-given
// matrices (make*Key, fastAlignUsingVkey, distDirectSC, distanceBtnScanContext) are O(800) and run here in the library's index
// order.  Without nanoflann there is no InvKeyTree: the snapshot lives in the library, polarcontext_invkeys_to_search_ mirrors it.
// distanceBtnScanContextBatch, distanceMatrix, bestMatches and detectLoopClosureIDExhaustive are extensions (include/gorio_sc_pairs.h),
// as are their forms that take a second SCManager, topMatches and detectLoopClosureIDAgainst (include/gorio_sc_cross.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <Eigen/Dense>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <radar_graph_slam/keyframe.hpp>

#include "gorio_sc.h"
#include "gorio_keyframes.h"

using Eigen::MatrixXd;
using SCPointType = pcl::PointXYZINormal;
using KeyMat = std::vector<std::vector<float>>;

inline MatrixXd circshift(MatrixXd& _mat, int _num_shift) {  // SC:42-62
  MatrixXd out(_mat.rows(), _mat.cols());
  for (int c = 0; c < _mat.cols(); ++c)
    for (int r = 0; r < _mat.rows(); ++r) out(r, (c + _num_shift) % _mat.cols()) = _mat(r, c);
  return out;
}

inline std::vector<float> eig2stdvec(MatrixXd _eigmat) { return std::vector<float>(_eigmat.data(), _eigmat.data() + _eigmat.size()); }  // SC:73-77

class SCManager {
 public:
  SCManager() { open(h_, params_); }
  ~SCManager() {
    if (h_) gorio_sc_destroy(h_);
    if (scratch_) gorio_sc_destroy(scratch_);
  }
  SCManager(const SCManager&) = delete;
  SCManager& operator=(const SCManager&) = delete;

  // The library holds the settings from creation, so a setter re-creates the (still empty) handle; changing a setting after
  // keyframes were added is refused, as LoopDetector sets both in its constructor (LD:88-89).
  void setScDistThresh(double thresh) {
    SC_DIST_THRES = thresh;
    params_.sc_dist_thresh = thresh;
    reopen();
  }
  void setAzimuthRange(double range) {
    PC_AZIMUTH_ANGLE_MAX = range;
    PC_AZIMUTH_ANGLE_MIN = -range;
    PC_UNIT_SECTOR_ANGLE = (PC_AZIMUTH_ANGLE_MAX - PC_AZIMUTH_ANGLE_MIN) / double(PC_NUM_SECTOR);
    params_.azimuth_range = range;
    reopen();
  }

  MatrixXd makeScancontext(pcl::PointCloud<SCPointType>& _scan_down) {
    if (!scratch_) open(scratch_, params_);
    const int idx = add(scratch_, _scan_down);
    MatrixXd desc(PC_NUM_RING, PC_NUM_SECTOR);
    fetch(scratch_, idx, &desc, nullptr, nullptr);
    return desc;
  }
  MatrixXd makeRingkeyFromScancontext(MatrixXd& _desc) {  // SC:219-229, index order
    MatrixXd k(_desc.rows(), 1);
    for (int r = 0; r < _desc.rows(); ++r) {
      double s = 0.0;
      for (int c = 0; c < _desc.cols(); ++c) s += _desc(r, c);
      k(r, 0) = s / (double)_desc.cols();
    }
    return k;
  }
  MatrixXd makeSectorkeyFromScancontext(MatrixXd& _desc) {  // SC:235-245, index order
    MatrixXd k(1, _desc.cols());
    for (int c = 0; c < _desc.cols(); ++c) {
      double s = 0.0;
      for (int r = 0; r < _desc.rows(); ++r) s += _desc(r, c);
      k(0, c) = s / (double)_desc.rows();
    }
    return k;
  }
  int fastAlignUsingVkey(MatrixXd& _vkey1, MatrixXd& _vkey2) {  // SC:104-122
    int arg = 0;
    double best = 10000000;
    for (int s = 0; s < _vkey1.cols(); ++s) {
      MatrixXd sh = circshift(_vkey2, s);
      double sq = 0.0;
      for (int j = 0; j < _vkey1.cols(); ++j) {
        const double d = _vkey1(0, j) - sh(0, j);
        sq += d * d;
      }
      const double n = std::sqrt(sq);
      if (n < best) {
        arg = s;
        best = n;
      }
    }
    return arg;
  }
  double distDirectSC(MatrixXd& _sc1, MatrixXd& _sc2) {  // SC:80-101
    int n_eff = 0;
    double sum = 0;
    for (int c = 0; c < _sc1.cols(); ++c) {
      double n1 = 0, n2 = 0, dot = 0;
      for (int r = 0; r < _sc1.rows(); ++r) {
        n1 += _sc1(r, c) * _sc1(r, c);
        n2 += _sc2(r, c) * _sc2(r, c);
        dot += _sc1(r, c) * _sc2(r, c);
      }
      n1 = std::sqrt(n1);
      n2 = std::sqrt(n2);
      if ((n1 == 0) | (n2 == 0)) continue;
      sum = sum + dot / (n1 * n2);
      n_eff = n_eff + 1;
    }
    return 1.0 - sum / n_eff;
  }
  std::pair<double, int> distanceBtnScanContext(MatrixXd& _sc1, MatrixXd& _sc2) {  // SC:127-160
    MatrixXd v1 = makeSectorkeyFromScancontext(_sc1), v2 = makeSectorkeyFromScancontext(_sc2);
    const int a = fastAlignUsingVkey(v1, v2);
    const int n = _sc1.cols();
    std::vector<int> space{a, (a + 1 + n) % n, (a - 1 + n) % n};
    std::sort(space.begin(), space.end());
    int arg = 0;
    double best = 10000000;
    for (int s : space) {
      MatrixXd sh = circshift(_sc2, s);
      const double d = distDirectSC(_sc1, sh);
      if (d < best) {
        arg = s;
        best = d;
      }
    }
    return std::make_pair(best, arg);
  }

  // User-side API
  void makeAndSaveScancontextAndKeys(pcl::PointCloud<SCPointType>& _scan_down) {  // SC:255-269, the descriptor made on the GPU
    const int idx = add(h_, _scan_down);
    MatrixXd sc(PC_NUM_RING, PC_NUM_SECTOR), ring(PC_NUM_RING, 1), sector(1, PC_NUM_SECTOR);
    fetch(h_, idx, &sc, &ring, &sector);
    polarcontexts_.push_back(sc);
    polarcontext_invkeys_.push_back(ring);
    polarcontext_vkeys_.push_back(sector);
    polarcontext_invkeys_mat_.push_back(eig2stdvec(ring));
  }
  // the same for a keyframe resident in a gorio::KeyframeStore (extra; radar_graph_slam_nodelet.cpp:727-731): packed on the device, no upload
  template <typename Store>
  void makeAndSaveScancontextAndKeys(Store& store, int id) {
    int idx = -1;
    check(gorio_sc_add_keyframes(h_, store.handle(), &id, 1, &idx), "makeAndSaveScancontextAndKeys");
    MatrixXd sc(PC_NUM_RING, PC_NUM_SECTOR), ring(PC_NUM_RING, 1), sector(1, PC_NUM_SECTOR);
    fetch(h_, idx, &sc, &ring, &sector);
    polarcontexts_.push_back(sc);
    polarcontext_invkeys_.push_back(ring);
    polarcontext_vkeys_.push_back(sector);
    polarcontext_invkeys_mat_.push_back(eig2stdvec(ring));
  }
  std::pair<int, float> detectLoopClosureID(const std::vector<radar_graph_slam::KeyFrame::Ptr>& candidate_keyframes, const radar_graph_slam::KeyFrame::Ptr& new_keyframe) {
    std::vector<int> cand;
    for (auto& k : candidate_keyframes) cand.push_back((int)k->index);
    int loop_id = -1;
    float yaw = 0.0f;
    double min_dist = 0.0;
    check(gorio_sc_detect(h_, (int)new_keyframe->index, cand.data(), (int)cand.size(), &loop_id, &yaw, &min_dist, nullptr), "detectLoopClosureID");
    int n = 0, m = 0;
    check(gorio_sc_get_state(h_, &n, &tree_making_period_conter, &m, nullptr, 0), "detectLoopClosureID");
    std::vector<int> snap(m);
    check(gorio_sc_get_state(h_, nullptr, nullptr, nullptr, snap.data(), m), "detectLoopClosureID");
    polarcontext_invkeys_to_search_.clear();
    for (int i : snap) polarcontext_invkeys_to_search_.push_back(polarcontext_invkeys_mat_.at(i));
    return {loop_id, yaw};
  }

  // ---- Exhaustive matching (include/gorio_sc_pairs.h).  An EXTENSION: the reference has none of these members.  Each keeps the
  // reference's distance (distanceBtnScanContext of two stored keyframes, the first unshifted); the detect also keeps the early
  // return, the recent-keyframe filter, the strict minimum in list order, the threshold and the yaw, and drops the tree, its counter
  // and its snapshot (tree_making_period_conter and polarcontext_invkeys_to_search_ are left alone).
  struct BestMatch {
    int index;    // -1: no candidate, or none below 1e7
    double dist;  // 1e7 then
    int shift;
  };
  // distanceBtnScanContext(polarcontexts_[first], polarcontexts_[second]) for every listed pair, in one launch
  std::vector<std::pair<double, int>> distanceBtnScanContextBatch(const std::vector<std::pair<int, int>>& pairs) {
    std::vector<int> q, c;
    for (auto& p : pairs) q.push_back(p.first), c.push_back(p.second);
    std::vector<double> d(pairs.size());
    std::vector<int> s(pairs.size());
    check(gorio_sc_distance_pairs(h_, q.data(), c.data(), (int)pairs.size(), d.data(), s.data()), "distanceBtnScanContextBatch");
    std::vector<std::pair<double, int>> out;
    for (size_t k = 0; k < pairs.size(); ++k) out.emplace_back(d[k], s[k]);
    return out;
  }
  // every (row, column) pair, row-major: dist / shift [rows.size() * cols.size()]
  void distanceMatrix(const std::vector<int>& rows, const std::vector<int>& cols, std::vector<double>& dist, std::vector<int>& shift) {
    dist.assign(rows.size() * cols.size(), 0.0);
    shift.assign(rows.size() * cols.size(), 0);
    check(gorio_sc_distance_matrix(h_, rows.data(), (int)rows.size(), cols.data(), (int)cols.size(), dist.data(), shift.data()), "distanceMatrix");
  }
  // the whole database against itself
  void distanceMatrix(std::vector<double>& dist, std::vector<int>& shift) {
    const size_t n = polarcontexts_.size();
    dist.assign(n * n, 0.0);
    shift.assign(n * n, 0);
    check(gorio_sc_distance_matrix(h_, nullptr, (int)n, nullptr, (int)n, dist.data(), shift.data()), "distanceMatrix");
  }
  // per listed keyframe r the best of the keyframes 0 .. r - min_gap (ties to the lower index), the matrix never materialised
  std::vector<BestMatch> bestMatches(const std::vector<int>& rows, int min_gap) { return best(rows.data(), (int)rows.size(), min_gap); }
  std::vector<BestMatch> bestMatches(int min_gap) { return best(nullptr, (int)polarcontexts_.size(), min_gap); }
  // detectLoopClosureID with every candidate scored instead of the tree's 3
  std::pair<int, float> detectLoopClosureIDExhaustive(const std::vector<radar_graph_slam::KeyFrame::Ptr>& candidate_keyframes, const radar_graph_slam::KeyFrame::Ptr& new_keyframe,
                                                      double* min_dist_out = nullptr) {
    std::vector<int> cand;
    for (auto& k : candidate_keyframes) cand.push_back((int)k->index);
    const int query = (int)new_keyframe->index, n = (int)cand.size();
    const int* list = cand.data();
    int loop_id = -1;
    float yaw = 0.0f;
    double min_dist = 0.0;
    check(gorio_sc_detect_exhaustive(h_, 1, &query, &list, &n, &loop_id, &yaw, &min_dist), "detectLoopClosureIDExhaustive");
    if (min_dist_out) *min_dist_out = min_dist;
    return {loop_id, yaw};
  }

  // ---- Matching against ANOTHER SCManager, and the K best per keyframe (include/gorio_sc_cross.h).  An EXTENSION as well: the
  // reference holds one SCManager per run.  This manager is the query side (the first, unshifted argument of distanceBtnScanContext),
  // `db` the database side, which is only read (`db` may be *this); SC_DIST_THRES is this manager's.  Both need the same azimuth range.
  // distanceBtnScanContext(polarcontexts_[first], db.polarcontexts_[second]) for every listed pair, in one launch
  std::vector<std::pair<double, int>> distanceBtnScanContextBatch(const SCManager& db, const std::vector<std::pair<int, int>>& pairs) {
    std::vector<int> q, c;
    for (auto& p : pairs) q.push_back(p.first), c.push_back(p.second);
    std::vector<double> d(pairs.size());
    std::vector<int> s(pairs.size());
    check(gorio_sc_cross_distance_pairs(h_, db.h_, q.data(), c.data(), (int)pairs.size(), d.data(), s.data()), "distanceBtnScanContextBatch");
    std::vector<std::pair<double, int>> out;
    for (size_t k = 0; k < pairs.size(); ++k) out.emplace_back(d[k], s[k]);
    return out;
  }
  // every (row of this manager, column of db) pair, row-major: dist / shift [rows.size() * cols.size()]
  void distanceMatrix(const SCManager& db, const std::vector<int>& rows, const std::vector<int>& cols, std::vector<double>& dist, std::vector<int>& shift) {
    dist.assign(rows.size() * cols.size(), 0.0);
    shift.assign(rows.size() * cols.size(), 0);
    check(gorio_sc_cross_distance_matrix(h_, rows.data(), (int)rows.size(), db.h_, cols.data(), (int)cols.size(), dist.data(), shift.data()), "distanceMatrix");
  }
  // per listed keyframe rows[i] its (up to) k best among db's keyframes 0 .. col_end[i] - 1 (col_end empty: all of db), ascending in
  // (dist, index), the matrix never materialised; fewer than k entries where fewer score below 1e7
  std::vector<std::vector<BestMatch>> topMatches(const SCManager& db, const std::vector<int>& rows, const std::vector<int>& col_end, int k) {
    if (!col_end.empty() && col_end.size() != rows.size()) throw std::logic_error("SCManager::topMatches: one col_end per row");
    return top(db, rows.data(), (int)rows.size(), col_end.empty() ? nullptr : col_end.data(), k);
  }
  // the same-database triangle: every keyframe r against the keyframes 0 .. r - min_gap
  std::vector<std::vector<BestMatch>> topMatches(int k, int min_gap) {
    if (min_gap < 1) throw std::logic_error("SCManager::topMatches: min_gap must be >= 1");
    std::vector<int> col_end(polarcontexts_.size());
    for (size_t r = 0; r < col_end.size(); ++r) col_end[r] = std::max(0, (int)r - min_gap + 1);
    return top(*this, nullptr, (int)col_end.size(), col_end.data(), k);
  }
  // detectLoopClosureID's decision over the listed keyframes of db, every one scored, in list order: (loop id or -1, yaw).  No early
  // return and no recent-keyframe filter: the indices of two sessions are unrelated.
  std::pair<int, float> detectLoopClosureIDAgainst(const SCManager& db, const std::vector<int>& candidate_indices, int query_index, double* min_dist_out = nullptr) {
    const int n = (int)candidate_indices.size();
    const int* list = candidate_indices.data();
    int loop_id = -1;
    float yaw = 0.0f;
    double min_dist = 0.0;
    check(gorio_sc_cross_detect(h_, db.h_, 1, &query_index, &list, &n, &loop_id, &yaw, &min_dist), "detectLoopClosureIDAgainst");
    if (min_dist_out) *min_dist_out = min_dist;
    return {loop_id, yaw};
  }

  const Eigen::MatrixXd& getConstRefRecentSCD(void) { return polarcontexts_.back(); }

 public:
  const double LIDAR_HEIGHT = 1.2;
  double PC_AZIMUTH_ANGLE_MAX = 56.5;
  double PC_AZIMUTH_ANGLE_MIN = -56.6;
  const int PC_NUM_RING = GORIO_SC_RINGS;
  const int PC_NUM_SECTOR = GORIO_SC_SECTORS;
  const double PC_MAX_RADIUS = GORIO_SC_MAX_RADIUS;
  double PC_UNIT_SECTOR_ANGLE = (PC_AZIMUTH_ANGLE_MAX - PC_AZIMUTH_ANGLE_MIN) / double(PC_NUM_SECTOR);
  const double PC_UNIT_RINGGAP = PC_MAX_RADIUS / double(PC_NUM_RING);
  const int NUM_EXCLUDE_RECENT = GORIO_SC_EXCLUDE_RECENT;
  const int NUM_CANDIDATES_FROM_TREE = GORIO_SC_CANDIDATES;
  const double SEARCH_RATIO = 0.1;
  double SC_DIST_THRES = 0.5;
  const int TREE_MAKING_PERIOD_ = GORIO_SC_TREE_PERIOD;
  int tree_making_period_conter = 0;

  std::vector<double> polarcontexts_timestamp_;
  std::vector<Eigen::MatrixXd> polarcontexts_;
  std::vector<Eigen::MatrixXd> polarcontext_invkeys_;
  std::vector<Eigen::MatrixXd> polarcontext_vkeys_;
  KeyMat polarcontext_invkeys_mat_;
  KeyMat polarcontext_invkeys_to_search_;

 private:
  gorio_sc_t* h_ = nullptr;
  gorio_sc_t* scratch_ = nullptr;
  gorio_sc_params params_ = {0.5, 56.5};  // SC_DIST_THRES (SCH:125); the in-class -56.6 is asymmetric, so until setAzimuthRange the
                                          // library holds the symmetric 56.5 every launch file sets

  static void check(int rc, const char* what) {
    if (rc < 0) throw std::runtime_error(std::string("SCManager::") + what + ": " + gorio_sc_last_error());
  }
  std::vector<BestMatch> best(const int* rows, int n_rows, int min_gap) {
    std::vector<int> idx(n_rows), shift(n_rows);
    std::vector<double> dist(n_rows);
    check(gorio_sc_best_matches(h_, rows, n_rows, min_gap, idx.data(), dist.data(), shift.data()), "bestMatches");
    std::vector<BestMatch> out(n_rows);
    for (int i = 0; i < n_rows; ++i) out[i] = BestMatch{idx[i], dist[i], shift[i]};
    return out;
  }
  std::vector<std::vector<BestMatch>> top(const SCManager& db, const int* rows, int n_rows, const int* col_end, int k) {
    const size_t slots = (size_t)n_rows * (size_t)std::max(k, 0);
    std::vector<int> idx(slots), shift(slots);
    std::vector<double> dist(slots);
    check(gorio_sc_cross_top_matches(h_, rows, n_rows, db.h_, col_end, k, idx.data(), dist.data(), shift.data()), "topMatches");
    std::vector<std::vector<BestMatch>> out(n_rows);
    for (int i = 0; i < n_rows; ++i)
      for (int j = 0; j < k && idx[(size_t)i * k + j] >= 0; ++j) out[i].push_back(BestMatch{idx[(size_t)i * k + j], dist[(size_t)i * k + j], shift[(size_t)i * k + j]});
    return out;
  }
  static void open(gorio_sc_t*& h, const gorio_sc_params& p) { check(gorio_sc_create(&h, 0, &p), "SCManager"); }
  void reopen() {
    int n = 0;
    check(gorio_sc_get_state(h_, &n, nullptr, nullptr, nullptr, 0), "set");
    if (n) throw std::logic_error("SCManager: settings change after keyframes were added");
    gorio_sc_destroy(h_);
    h_ = nullptr;
    open(h_, params_);
    if (scratch_) gorio_sc_destroy(scratch_);
    scratch_ = nullptr;
  }
  static int add(gorio_sc_t* h, pcl::PointCloud<SCPointType>& c) {
    const int n = (int)c.size();
    const float* x = n ? &c.points[0].x : nullptr;
    const float* in = n ? &c.points[0].intensity : nullptr;
    const int stride = (int)sizeof(SCPointType);
    int first = -1;
    check(gorio_sc_add_scans(h, 1, &x, &in, &n, &stride, &first), "makeAndSaveScancontextAndKeys");
    return first;
  }
  static void fetch(gorio_sc_t* h, int idx, MatrixXd* desc, MatrixXd* ring, MatrixXd* sector) {
    std::vector<double> d(GORIO_SC_RINGS * GORIO_SC_SECTORS), r(GORIO_SC_RINGS), s(GORIO_SC_SECTORS);
    check(gorio_sc_get_descriptor(h, idx, d.data(), r.data(), s.data()), "getDescriptor");
    for (int i = 0; i < GORIO_SC_RINGS; ++i) {
      for (int j = 0; j < GORIO_SC_SECTORS; ++j)
        if (desc) (*desc)(i, j) = d[i * GORIO_SC_SECTORS + j];
      if (ring) (*ring)(i, 0) = r[i];
    }
    for (int j = 0; j < GORIO_SC_SECTORS; ++j)
      if (sector) (*sector)(0, j) = s[j];
  }
};
