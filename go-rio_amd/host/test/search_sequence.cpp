// gorio::GpuSearch over one cloud and one set of queries: the batch overloads, the single-point overloads and the form that shares the
// target of a FastAPDGICP must agree with each other (an empty query cloud gives empty lists) and with the expected values the caller passes in (tests/search_restatement.py).
// Input: binary [int32 n][n x (x, y, z) float32][int32 nq][nq x (x, y, z) float32][int32 k][float64 radius][int32 max_nn]
//        [nq x k int32 idx][nq x k float32 sqd][nq int32 count][(nq + 1) int64 offsets][total int32 idx][total float32 sqd].
// Output: one JSON line; every "..._ok" must be 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <gorio/gpu_search.hpp>

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;
using Lists = std::vector<std::vector<int>>;
using DLists = std::vector<std::vector<float>>;

template <typename T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
static Cloud::Ptr to_cloud(const std::vector<float>& xyz) {
  Cloud::Ptr c(new Cloud());
  c->resize(xyz.size() / 3);
  for (size_t i = 0; i < c->size(); ++i) {
    PointT& p = c->points[i];
    p.x = xyz[3 * i], p.y = xyz[3 * i + 1], p.z = xyz[3 * i + 2];
    p.data[3] = 1.0f;
  }
  return c;
}
static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), sizeof(float) * a.size()) == 0);
}
static bool same(const Lists& ai, const DLists& ad, const Lists& bi, const DLists& bd) {
  if (ai.size() != bi.size() || ad.size() != bd.size() || ai.size() != ad.size()) return false;
  for (size_t q = 0; q < ai.size(); ++q)
    if (ai[q] != bi[q] || !same_bits(ad[q], bd[q])) return false;
  return true;
}

static int run(int argc, char** argv) {
  if (argc < 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t n = 0, nq = 0, k = 0, max_nn = 0;
  double radius = 0.0;
  std::vector<float> xyz, q, e_sqd, er_sqd;
  std::vector<int32_t> e_idx, e_cnt, er_idx;
  std::vector<int64_t> er_offs;
  bool ok = std::fread(&n, 4, 1, f) == 1 && read_vec(f, xyz, (size_t)n * 3) && std::fread(&nq, 4, 1, f) == 1 && read_vec(f, q, (size_t)nq * 3) && std::fread(&k, 4, 1, f) == 1 &&
            std::fread(&radius, 8, 1, f) == 1 && std::fread(&max_nn, 4, 1, f) == 1 && read_vec(f, e_idx, (size_t)nq * k) && read_vec(f, e_sqd, (size_t)nq * k) &&
            read_vec(f, e_cnt, (size_t)nq) && read_vec(f, er_offs, (size_t)nq + 1);
  ok = ok && read_vec(f, er_idx, (size_t)er_offs[nq]) && read_vec(f, er_sqd, (size_t)er_offs[nq]);
  std::fclose(f);
  if (!ok) return 2;
  Lists want_i(nq), want_ri(nq);
  DLists want_d(nq), want_rd(nq);
  for (int i = 0; i < nq; ++i) {
    want_i[i].assign(e_idx.begin() + (size_t)i * k, e_idx.begin() + (size_t)i * k + e_cnt[i]);
    want_d[i].assign(e_sqd.begin() + (size_t)i * k, e_sqd.begin() + (size_t)i * k + e_cnt[i]);
    want_ri[i].assign(er_idx.begin() + er_offs[i], er_idx.begin() + er_offs[i + 1]);
    want_rd[i].assign(er_sqd.begin() + er_offs[i], er_sqd.begin() + er_offs[i + 1]);
  }
  const Cloud::Ptr cloud = to_cloud(xyz), queries = to_cloud(q);

  gorio::GpuSearch<PointT> gs;
  gs.setInputCloud(cloud);
  // ---- batch overloads against the expected values
  Lists ki, ri;
  DLists kd, rd;
  gs.nearestKSearch(*queries, std::vector<int>(), k, ki, kd);
  gs.radiusSearch(*queries, std::vector<int>(), radius, ri, rd, (unsigned int)max_nn);
  const bool knn_ok = same(ki, kd, want_i, want_d), radius_ok = same(ri, rd, want_ri, want_rd);
  // ---- an index list picks its queries
  std::vector<int> pick;
  for (int i = nq - 1; i >= 0; i -= 2) pick.push_back(i);
  Lists pi, pri;
  DLists pd, prd;
  gs.nearestKSearch(*queries, pick, k, pi, pd);
  gs.radiusSearch(*queries, pick, radius, pri, prd, (unsigned int)max_nn);
  bool pick_ok = pi.size() == pick.size() && pri.size() == pick.size();
  for (size_t j = 0; pick_ok && j < pick.size(); ++j)
    pick_ok = pi[j] == ki[pick[j]] && same_bits(pd[j], kd[pick[j]]) && pri[j] == ri[pick[j]] && same_bits(prd[j], rd[pick[j]]);
  // ---- single-point overloads forward to the batch
  bool single_ok = true;
  for (int i = 0; i < nq && i < 16; ++i) {
    std::vector<int> si, sri;
    std::vector<float> sd, srd;
    const int c1 = gs.nearestKSearch(queries->points[i], k, si, sd);
    const int c2 = gs.radiusSearch(queries->points[i], radius, sri, srd, (unsigned int)max_nn);
    single_ok = single_ok && c1 == (int)ki[i].size() && si == ki[i] && same_bits(sd, kd[i]) && c2 == (int)ri[i].size() && sri == ri[i] && same_bits(srd, rd[i]);
  }
  // ---- no queries at all: empty lists, as pcl::search::Search gives
  const Cloud none;
  Lists ni(3), nri(3);
  DLists nd(3), nrd(3);
  gs.nearestKSearch(none, std::vector<int>(), k, ni, nd);
  gs.radiusSearch(none, std::vector<int>(), radius, nri, nrd, (unsigned int)max_nn);
  const bool empty_ok = ni.empty() && nd.empty() && nri.empty() && nrd.empty();
  // ---- the target of a registration object, shared: nothing is uploaded, no index is built through the search handle
  Reg reg;
  reg.setInputTarget(cloud);
  gorio::GpuSearch<PointT> shared;
  shared.setInputCloud(reg, 1);
  Lists si2, sri2;
  DLists sd2, srd2;
  shared.nearestKSearch(*queries, std::vector<int>(), k, si2, sd2);
  shared.radiusSearch(*queries, std::vector<int>(), radius, sri2, srd2, (unsigned int)max_nn);
  const auto c = shared.counters();
  const bool shared_ok = same(si2, sd2, ki, kd) && same(sri2, srd2, ri, rd) && c.point_uploads == 0 && c.index_builds == 0 && shared.getInputCloud() == cloud;
  const auto own = gs.counters();
  std::printf("{\"n\": %d, \"nq\": %d, \"k\": %d, \"knn_ok\": %d, \"radius_ok\": %d, \"pick_ok\": %d, \"single_ok\": %d, \"shared_ok\": %d, \"empty_ok\": %d, \"own_uploads\": %lld, \"own_builds\": %lld}\n", n, nq, k,
              knn_ok, radius_ok, pick_ok, single_ok, shared_ok, empty_ok, own.point_uploads, own.index_builds);
  return (knn_ok && radius_ok && pick_ok && single_ok && shared_ok && empty_ok) ? 0 : 1;
}

int main(int argc, char** argv) {
  try {
    return run(argc, argv);
  } catch (const std::exception& e) {  // no CPU fallback: without a HIP device the first object throws
    std::fprintf(stderr, "search_sequence: %s\n", e.what());
    return 3;
  }
}
