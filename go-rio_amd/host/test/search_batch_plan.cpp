// Stand-alone driver of the host-side planning of a BATCH of radius queries (go-rio_amd/csrc/search_plan.h): the wave table, the jobs'
// bases into the shared grids and the shared found offsets, the key segments of the one query sort, job_of, and the merged table of long
// segments.  Links nothing of HIP or the library; the Makefile also builds it with the sanitizers.  One JSON line per case;
// tests/test_search_batch_plan.py recomputes every number, the merged long segments from per-job make_plan.
#include <cstdio>
#include <vector>

#include "../../csrc/search_plan.h"

namespace sp = gorio::search_plan;

template <class T>
static void print_list(const char* name, const std::vector<T>& v, bool last = false) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
  std::printf("]%s", last ? "" : ", ");
}

static void layout_case(const char* name, const std::vector<sp::BatchJobShape>& jobs) {
  const int count = (int)jobs.size();
  sp::BatchLayout b;
  const bool ok = sp::make_batch_layout(jobs.data(), count, b);
  std::vector<int> nq, self, active, wjob, wwave, owner_of_wave, owner_of_query;
  for (const sp::BatchJobShape& j : jobs) nq.push_back(j.nq), self.push_back(j.self ? 1 : 0), active.push_back(j.active ? 1 : 0);
  for (const sp::WaveRef& w : b.wave_tab) wjob.push_back(w.job), wwave.push_back(w.wave);
  // job_of over every item of both grids
  for (int w = 0; ok && w < b.wave_first[count]; ++w) owner_of_wave.push_back(sp::job_of(b.wave_first.data(), count, w));
  for (int q = 0; ok && q < b.query_first[count]; ++q) owner_of_query.push_back(sp::job_of(b.query_first.data(), count, q));
  std::printf("{\"case\": \"%s\", \"ok\": %d, ", name, ok ? 1 : 0);
  print_list("nq", nq);
  print_list("self", self);
  print_list("active", active);
  print_list("wave_job", wjob);
  print_list("wave_in_job", wwave);
  print_list("wave_first", b.wave_first);
  print_list("query_first", b.query_first);
  print_list("offs_first", b.offs_first);
  print_list("key_seg", b.key_seg);
  print_list("key_jobs", b.key_jobs);
  print_list("key_first", b.key_first);
  print_list("owner_of_wave", owner_of_wave);
  print_list("owner_of_query", owner_of_query);
  std::printf("\"max_key_pow2\": %d, \"key_items\": %lld}\n", b.max_key_pow2, b.key_items);
}

// per-job neighbour counts -> per-job plans -> the merged long-segment table
static void merge_case(const char* name, const std::vector<std::vector<int>>& counts, int max_nn) {
  const int count = (int)counts.size();
  std::vector<sp::Plan> plans((size_t)count);
  std::vector<long long> job_slot_keys, job_max_pow2, job_n_long;
  bool ok = true;
  for (int j = 0; j < count; ++j) {
    const int nq = (int)counts[j].size();
    std::vector<long long> fo((size_t)nq + 1), ko((size_t)nq + 1);
    ok = ok && sp::offsets_from_counts(counts[j].data(), nq, max_nn, fo.data(), ko.data()) && sp::make_plan(fo.data(), nq, max_nn, plans[j]);
    job_slot_keys.push_back(plans[j].slot_keys), job_max_pow2.push_back(plans[j].max_pow2), job_n_long.push_back((long long)plans[j].long_segs.size());
  }
  sp::BatchLongPlan m;
  sp::merge_long_segs(plans.data(), count, m);
  std::vector<long long> job, query, src, slot, out, len, npow2, kept, own_slot;
  for (const sp::BatchLongSeg& s : m.segs) {
    job.push_back(s.job), query.push_back(s.seg.query), src.push_back(s.seg.src), slot.push_back(s.seg.slot), out.push_back(s.seg.out), len.push_back(s.seg.len),
        npow2.push_back(s.seg.npow2), kept.push_back(s.seg.kept);
  }
  for (int j = 0; j < count; ++j)
    for (const sp::LongSeg& s : plans[j].long_segs) own_slot.push_back(s.slot);  // the slots inside the job's own plan
  std::printf("{\"case\": \"%s\", \"ok\": %d, \"max_nn\": %d, ", name, ok ? 1 : 0, max_nn);
  std::printf("\"counts\": [");
  for (int j = 0; j < count; ++j) {
    std::printf("%s[", j ? ", " : "");
    for (size_t i = 0; i < counts[j].size(); ++i) std::printf("%s%d", i ? ", " : "", counts[j][i]);
    std::printf("]");
  }
  std::printf("], ");
  print_list("job_slot_keys", job_slot_keys);
  print_list("job_max_pow2", job_max_pow2);
  print_list("job_n_long", job_n_long);
  print_list("job", job);
  print_list("query", query);
  print_list("src", src);
  print_list("slot", slot);
  print_list("own_slot", own_slot);
  print_list("out", out);
  print_list("len", len);
  print_list("npow2", npow2);
  print_list("kept", kept);
  std::printf("\"slot_keys\": %lld, \"max_pow2\": %d}\n", m.slot_keys, m.max_pow2);
}

int main() {
  using J = sp::BatchJobShape;
  layout_case("wave_edges", {J{0, false, false}, J{1, false, true}, J{63, false, true}, J{64, true, true}, J{65, false, true}});
  layout_case("all_empty", {J{0, false, false}, J{0, true, false}, J{17, false, false}});
  layout_case("no_job", {});
  layout_case("empty_between", {J{130, false, true}, J{0, false, false}, J{300, true, false}, J{5000, false, true}, J{64, true, true}, J{9, false, false}});
  layout_case("one", {J{257, false, true}});
  merge_case("two_long_jobs", {{3, 5000, 0, 4097}, {7, 1}, {9000, 4096, 20000}, {}}, 0);
  merge_case("two_long_jobs_cut", {{3, 5000, 0, 4097}, {7, 1}, {9000, 4096, 20000}, {}}, 4100);
  merge_case("no_long", {{1, 2, 3}, {4096}}, 0);
  return 0;
}
