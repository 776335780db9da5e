// search_plan.h -- host-side planning of the radius queries of apd_search.hip (include/gorio_search.h): the CSR offsets, which sort
// every query's segment of neighbours takes, and the capacity arithmetic.  Host code only, nothing of HIP: apd_search.hip includes it, and
// host/test/search_plan.cpp runs it alone (and under the sanitizers).
//
// A radius call finds found[q] neighbours per query and keeps kept[q] = found[q], or min(found[q], max_nn) when max_nn > 0.  The device
// holds the found neighbours as 64-bit keys (float bits of d) << 32 | index in one array, query q at [found_offs[q], found_offs[q + 1]),
// sorts every segment ascending and emits the first kept[q] keys of it to [kept_offs[q], kept_offs[q + 1]) of the result.
//   segment of 0 keys             nothing to do
//   1 .. kSegLdsMax keys          one workgroup sorts it inside LDS (kSegLdsMax * 8 bytes = 32 KiB of the CU's 160 KiB)
//   more                          a LONG segment: copied into a slot of its own in a padded buffer, the slot a power of two of at least one
//                                 sort tile (the tiled sort sorts power-of-two arrays, all long segments in one set of launches), padding
//                                 keys ~0 behind the real ones
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gorio {
namespace search_plan {

constexpr long long kMaxTotal = 2147483647LL;  // 2^31 - 1 found neighbours per call
constexpr int kSegLdsMax = 4096;               // keys of the longest segment that is sorted inside LDS
constexpr int kSortTileKeys = 4096;            // keys per tile of the tiled sort (kSortTile, apd_index.hip)

inline int kept_of(int found, int max_nn) { return (max_nn > 0 && found > max_nn) ? max_nn : found; }

// Exclusive scans of found[] and kept[] (what search_scan_kernel computes on the device), nq + 1 entries each.  false (nothing else is
// promised about the outputs) when a count is negative or the found total exceeds kMaxTotal.
inline bool offsets_from_counts(const int* found, int nq, int max_nn, long long* found_offs, long long* kept_offs) {
  long long f = 0, k = 0;
  for (int q = 0; q < nq; ++q) {
    if (found[q] < 0) return false;
    found_offs[q] = f;
    kept_offs[q] = k;
    f += found[q];
    k += kept_of(found[q], max_nn);
    if (f > kMaxTotal) return false;
  }
  found_offs[nq] = f;
  kept_offs[nq] = k;
  return true;
}

enum SegClass { kSegEmpty = 0, kSegLds = 1, kSegLong = 2 };
inline SegClass classify(long long len) { return len <= 0 ? kSegEmpty : (len <= kSegLdsMax ? kSegLds : kSegLong); }

// slot size of a long segment: the power of two >= len, at least one sort tile; 0 when it would not fit an int
inline int slot_size(long long len) {
  long long p = kSortTileKeys;
  while (p < len) p <<= 1;
  return p > (1LL << 30) ? 0 : (int)p;
}

// One long segment as the device sees it (the kernels of apd_search.hip read an array of these).
struct LongSeg {
  long long src;   // first key of the segment in the found array
  long long slot;  // first key of its slot in the padded buffer
  long long out;   // first entry of the query's result
  int len;         // keys found
  int npow2;       // slot size
  int kept;        // keys emitted
  int query;
};

struct Plan {
  std::vector<LongSeg> long_segs;
  long long found_total = 0, kept_total = 0;
  long long slot_keys = 0;  // size of the padded buffer
  int max_pow2 = 0;         // largest slot (0: no long segment)
  int n_lds = 0;            // segments the LDS kernel sorts
};

// The plan from the found offsets (nq + 1 entries, as the device scanned them).  false when the offsets are not ascending from 0, the
// total exceeds kMaxTotal or a slot cannot be sized.
inline bool make_plan(const long long* found_offs, int nq, int max_nn, Plan& p) {
  p = Plan();
  if (nq < 0 || found_offs[0] != 0) return false;
  long long kept = 0;
  for (int q = 0; q < nq; ++q) {
    const long long len = found_offs[q + 1] - found_offs[q];
    if (len < 0 || found_offs[q + 1] > kMaxTotal) return false;
    const int k = kept_of((int)len, max_nn);
    const SegClass c = classify(len);
    if (c == kSegLds) ++p.n_lds;
    if (c == kSegLong) {
      const int slot = slot_size(len);
      if (slot == 0) return false;
      p.long_segs.push_back(LongSeg{found_offs[q], p.slot_keys, kept, (int)len, slot, k, q});
      p.slot_keys += slot;
      if (slot > p.max_pow2) p.max_pow2 = slot;
    }
    kept += k;
  }
  p.found_total = found_offs[nq];
  p.kept_total = kept;
  return true;
}

// elements to allocate for a buffer that must hold `need`: an eighth more, so that calls of slowly growing size do not reallocate
inline size_t grown(size_t need) { return need + need / 8 + 16; }

// entries the caller's arrays must hold for gorio_search_radius_get
inline bool capacity_ok(long long capacity, long long total) { return capacity >= total; }

}  // namespace search_plan
}  // namespace gorio
