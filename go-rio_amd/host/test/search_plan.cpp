// Stand-alone driver of the host-side planning of the radius queries (go-rio_amd/csrc/search_plan.h): CSR offsets, segment classes,
// slots of the long segments, capacity arithmetic.  Links nothing of HIP or the library; the Makefile also builds it with the sanitizers.
// One JSON line per case; tests/test_search_plan.py recomputes every number.
#include <cstdio>
#include <vector>

#include "../../csrc/search_plan.h"

namespace sp = gorio::search_plan;

static void print_ll(const char* name, const std::vector<long long>& v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? ", " : "", v[i]);
  std::printf("]");
}

// the counts of a case: a deterministic mix of empty, short, boundary and long segments
static std::vector<int> counts_of(int which) {
  switch (which) {
    case 0: return {};
    case 1: return {0, 0, 0};
    case 2: return {3, 0, 7, 1, 12, 0, 5};
    case 3: return {sp::kSegLdsMax - 1, sp::kSegLdsMax, sp::kSegLdsMax + 1, 0, 2 * sp::kSortTileKeys, 2 * sp::kSortTileKeys + 1, 9000, 1};
    default: {
      std::vector<int> c(1000);
      unsigned int s = 12345u;
      for (int& v : c) {
        s = s * 1664525u + 1013904223u;
        v = (int)((s >> 16) % 40u);
        if ((s & 1023u) == 0) v = 5000 + (int)((s >> 10) % 20000u);
      }
      return c;
    }
  }
}

static void run_case(int which, int max_nn) {
  const std::vector<int> cnt = counts_of(which);
  const int nq = (int)cnt.size();
  std::vector<long long> fo((size_t)nq + 1), ko((size_t)nq + 1);
  const bool ok = sp::offsets_from_counts(cnt.data(), nq, max_nn, fo.data(), ko.data());
  sp::Plan plan;
  const bool planned = ok && sp::make_plan(fo.data(), nq, max_nn, plan);
  std::printf("{\"case\": %d, \"max_nn\": %d, \"ok\": %d, \"planned\": %d, ", which, max_nn, ok ? 1 : 0, planned ? 1 : 0);
  print_ll("found_offs", fo);
  std::printf(", ");
  print_ll("kept_offs", ko);
  std::vector<long long> cls, q, src, slot, out, len, npow2, kept;
  for (int c : cnt) cls.push_back((long long)sp::classify(c));
  for (const sp::LongSeg& s : plan.long_segs) {
    q.push_back(s.query), src.push_back(s.src), slot.push_back(s.slot), out.push_back(s.out), len.push_back(s.len), npow2.push_back(s.npow2), kept.push_back(s.kept);
  }
  std::printf(", ");
  print_ll("class", cls);
  std::printf(", ");
  print_ll("long_query", q);
  std::printf(", ");
  print_ll("long_src", src);
  std::printf(", ");
  print_ll("long_slot", slot);
  std::printf(", ");
  print_ll("long_out", out);
  std::printf(", ");
  print_ll("long_len", len);
  std::printf(", ");
  print_ll("long_npow2", npow2);
  std::printf(", ");
  print_ll("long_kept", kept);
  std::printf(", \"found_total\": %lld, \"kept_total\": %lld, \"slot_keys\": %lld, \"max_pow2\": %d, \"n_lds\": %d}\n", plan.found_total, plan.kept_total, plan.slot_keys,
              plan.max_pow2, plan.n_lds);
}

int main() {
  for (int which = 0; which < 5; ++which)
    for (int max_nn : {0, 1, 7, 5000}) run_case(which, max_nn);
  // refusals: a total beyond 2^31 - 1, a negative count, offsets that do not start at 0 or descend
  {
    std::vector<int> big(3, 1 << 30);
    std::vector<long long> fo(4), ko(4);
    const bool a = sp::offsets_from_counts(big.data(), 3, 0, fo.data(), ko.data());
    std::vector<int> two(2, 1 << 30);
    const bool a2 = sp::offsets_from_counts(two.data(), 2, 0, fo.data(), ko.data());  // 2^31 exactly: one too many
    std::vector<int> fits = {(1 << 30), (1 << 30) - 1};
    const bool a3 = sp::offsets_from_counts(fits.data(), 2, 0, fo.data(), ko.data());  // 2^31 - 1: the largest total
    std::vector<int> neg = {1, -1};
    const bool b = sp::offsets_from_counts(neg.data(), 2, 0, fo.data(), ko.data());
    sp::Plan p;
    const long long bad0[3] = {1, 2, 3}, desc[3] = {0, 5, 4}, over[2] = {0, sp::kMaxTotal + 1};
    const long long huge[2] = {0, sp::kMaxTotal};
    const bool c = sp::make_plan(bad0, 2, 0, p), d = sp::make_plan(desc, 2, 0, p), e = sp::make_plan(over, 1, 0, p), f = sp::make_plan(huge, 1, 0, p);
    std::printf("{\"case\": \"refusals\", \"total_3x2e30\": %d, \"total_2e31\": %d, \"total_2e31m1\": %d, \"negative\": %d, \"start\": %d, \"descending\": %d, \"over\": %d, \"one_segment_2e31m1\": %d}\n",
                a, a2, a3, b, c, d, e, f);
  }
  std::printf("{\"case\": \"arith\", \"slot_1\": %d, \"slot_4097\": %d, \"slot_2e30\": %d, \"slot_2e30p1\": %d, \"grown_0\": %zu, \"grown_800\": %zu, \"cap_eq\": %d, \"cap_less\": %d, \"kept_0_5\": %d, \"kept_9_5\": %d, \"kept_9_0\": %d}\n",
              sp::slot_size(1), sp::slot_size(4097), sp::slot_size(1LL << 30), sp::slot_size((1LL << 30) + 1), sp::grown(0), sp::grown(800), sp::capacity_ok(10, 10) ? 1 : 0,
              sp::capacity_ok(9, 10) ? 1 : 0, sp::kept_of(0, 5), sp::kept_of(9, 5), sp::kept_of(9, 0));
  return 0;
}
