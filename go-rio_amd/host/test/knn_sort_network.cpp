// Stand-alone check of the comparator network knn_collect_kernel sorts its buffered keys with (csrc/knn_sort_network.h): host code only.
//   1. 0/1 principle, every one of the 2^24 inputs of zeros and ones, 64 of them per machine word (min = and, max = or): kept output t
//      must be a one exactly when the input has at least 24 - t ones.  A network that passes leaves the t-th smallest of ANY input at
//      output t, for every kept t.
//   2. the kernel's own inputs: cnt = 0 .. 24 distinct (distance, index) keys, the other rows the padding value, in random order, equal
//      distances included: the first 20 outputs against std::sort.
// Prints one JSON line; tests/test_knn_sort_network.py runs it plain and under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../csrc/knn_sort_network.h"

using gorio::kKnnSortKeep;
using gorio::kKnnSortWidth;

static long zero_one_failures() {
  // word of the lanes (the low six input bits) whose own ones count is at least k
  uint64_t at_least[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int l = 0; l < 64; ++l)
    for (int k = 0; k < 8; ++k)
      if (__builtin_popcount((unsigned)l) >= k) at_least[k] |= 1ull << l;
  uint64_t low[6];
  for (int w = 0; w < 6; ++w) {
    low[w] = 0;
    for (int l = 0; l < 64; ++l)
      if ((l >> w) & 1) low[w] |= 1ull << l;
  }
  long failures = 0;
  for (uint32_t block = 0; block < (1u << (kKnnSortWidth - 6)); ++block) {
    uint64_t v[kKnnSortWidth];
    for (int w = 0; w < 6; ++w) v[w] = low[w];
    for (int w = 6; w < kKnnSortWidth; ++w) v[w] = ((block >> (w - 6)) & 1u) ? ~0ull : 0ull;
    gorio::knn_sort_network(v, [](uint64_t& lo, uint64_t& hi) {
      const uint64_t a = lo & hi, b = lo | hi;
      lo = a;
      hi = b;
    });
    const int ones_high = __builtin_popcount(block);
    for (int t = 0; t < kKnnSortKeep; ++t) {
      const int need = kKnnSortWidth - t - ones_high;  // ones the lane itself must bring for output t to be a one
      const uint64_t expect = need <= 0 ? ~0ull : need > 6 ? 0ull : at_least[need];
      failures += __builtin_popcountll(v[t] ^ expect);
    }
  }
  return failures;
}

static long padded_failures(long* cases) {
  const uint64_t pad = 0x7f8000007fffffffull;  // (+inf, int max): what knn_collect_kernel reads a row past cnt as
  std::mt19937_64 rng(20);
  long failures = 0;
  *cases = 0;
  for (int cnt = 0; cnt <= kKnnSortWidth; ++cnt) {
    for (int trial = 0; trial < 2000; ++trial) {
      uint64_t v[kKnnSortWidth], ref[kKnnSortWidth];
      const int distinct = 1 + (int)(rng() % 6);  // few distinct distances: many ties, resolved on the index
      for (int r = 0; r < kKnnSortWidth; ++r) {
        const float d = (trial & 1) ? (float)(rng() % distinct) * 0.25f : (float)(rng() % 1000003) * 1e-3f;
        uint32_t bits;
        std::memcpy(&bits, &d, sizeof(bits));
        v[r] = r < cnt ? ((uint64_t)bits << 32) | (uint32_t)(r * 7919u + (uint32_t)(rng() % 7919u)) : pad;  // the index alone makes a key distinct
      }
      std::shuffle(v, v + cnt, rng);
      std::memcpy(ref, v, sizeof(v));
      std::sort(ref, ref + kKnnSortWidth);
      gorio::knn_sort_network(v, [](uint64_t& lo, uint64_t& hi) {
        const bool swap = hi < lo;
        const uint64_t a = swap ? hi : lo, b = swap ? lo : hi;
        lo = a;
        hi = b;
      });
      failures += std::memcmp(v, ref, sizeof(uint64_t) * kKnnSortKeep) != 0;
      ++*cases;
    }
  }
  return failures;
}

int main() {
  const long zo = zero_one_failures();
  long cases = 0;
  const long pf = padded_failures(&cases);
  std::printf("{\"width\": %d, \"keep\": %d, \"comparators\": %d, \"zero_one_inputs\": %ld, \"zero_one_failures\": %ld, \"padded_cases\": %ld, \"padded_failures\": %ld}\n",
              kKnnSortWidth, kKnnSortKeep, gorio::kKnnSortComparators, 1l << kKnnSortWidth, zo, cases, pf);
  return zo == 0 && pf == 0 ? 0 : 1;
}
