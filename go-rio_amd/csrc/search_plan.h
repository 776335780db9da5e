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

// ---- a BATCH of radius calls (search_radius_batch_core of apd_search.hip): several jobs, each a call of its own against a cloud of its
// own, run by one set of launches.  Every job keeps the buffers of its own search state (found counts, keys, result), so its offsets stay
// 64-bit counts of its own neighbours; what the jobs share is the launch grids, the found offsets the host reads back in one copy, the
// query-key segments of one tiled sort and the table and slots of the long segments.
//   count / fill     one wave per 64 queries, the jobs' waves one after the other: wave w of the launch is wave_tab[w] = (job, wave in job)
//   segment sort     one workgroup per query, the jobs' queries one after the other: workgroup g belongs to job_of(query_first, count, g)
//   found offsets    job j's nq + 1 offsets at offs_first[j] of the shared buffer
//   query keys       job j's segment (a power of two, >= one sort tile) is segment key_seg[j] of the one tiled sort, or -1: a job with
//                    self queries needs no keys.  The sort takes the passes of the largest segment (max_key_pow2).
// A job that is not `active` (no query, or an empty cloud) takes part in none of it.
struct BatchJobShape {
  int nq;      // queries (self queries: the size of the cloud)
  bool self;   // the queries are the cloud's own points
  bool active;
};
struct WaveRef {
  int job, wave;
};
struct BatchLayout {
  std::vector<WaveRef> wave_tab;
  std::vector<int> wave_first, query_first, key_seg;  // count + 1, count + 1, count
  std::vector<long long> offs_first;                  // count + 1
  std::vector<int> key_jobs;                          // the jobs of the key segments, in segment order
  std::vector<int> key_first;                         // segments + 1: the first 256-key block of every segment in the key launch
  int max_key_pow2 = 0;                               // 0: no job has cross queries
  long long key_items = 0;                            // workgroups of 256 threads the key launch takes: the segments' sizes / 256 added up
};

inline int key_pow2(int nq) {
  int p = kSortTileKeys;
  while (p < nq) p <<= 1;
  return p;
}

// false when the batch does not fit the int grids of its launches
inline bool make_batch_layout(const BatchJobShape* jobs, int count, BatchLayout& b) {
  b = BatchLayout();
  b.wave_first.assign((size_t)count + 1, 0);
  b.query_first.assign((size_t)count + 1, 0);
  b.offs_first.assign((size_t)count + 1, 0);
  b.key_seg.assign((size_t)count, -1);
  long long waves = 0, queries = 0, offs = 0;
  for (int j = 0; j < count; ++j) {
    b.wave_first[j] = (int)waves;
    b.query_first[j] = (int)queries;
    b.offs_first[j] = offs;
    if (!jobs[j].active || jobs[j].nq <= 0) continue;
    const int nw = (jobs[j].nq + 63) / 64;
    waves += nw;
    queries += jobs[j].nq;
    offs += (long long)jobs[j].nq + 1;
    if (waves > kMaxTotal || queries > kMaxTotal) return false;
    for (int w = 0; w < nw; ++w) b.wave_tab.push_back(WaveRef{j, w});
    if (!jobs[j].self) {
      const int p = key_pow2(jobs[j].nq);
      b.key_seg[j] = (int)b.key_jobs.size();
      b.key_jobs.push_back(j);
      b.key_first.push_back((int)b.key_items);
      b.key_items += p / 256;
      if (b.key_items > kMaxTotal) return false;
      if (p > b.max_key_pow2) b.max_key_pow2 = p;
    }
  }
  b.wave_first[count] = (int)waves;
  b.query_first[count] = (int)queries;
  b.offs_first[count] = offs;
  b.key_first.push_back((int)b.key_items);
  return true;
}

// the job of item x of a launch whose jobs own [first[j], first[j + 1]): the last j with first[j] <= x (jobs without items share their
// successor's start and are never the answer).  count >= 1, 0 <= x < first[count].  Plain integer code: the kernels of apd_search.hip run
// the same function over the device copy of `first` (IntPtr: their scalar-load pointer).
template <class IntPtr>
#ifdef __HIPCC__
__host__ __device__
#endif
inline int job_of(IntPtr first, int count, int x) {
  int lo = 0, hi = count;  // first[lo] <= x < first[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (first[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// One long segment of a batch: the segment as its job's plan has it (src / out count inside the job's own buffers), the slot moved into
// the ONE padded buffer all jobs share.
struct BatchLongSeg {
  LongSeg seg;
  int job;
  int pad_;
};
struct BatchLongPlan {
  std::vector<BatchLongSeg> segs;
  long long slot_keys = 0;
  int max_pow2 = 0;
};
inline void merge_long_segs(const Plan* plans, int count, BatchLongPlan& m) {
  m = BatchLongPlan();
  for (int j = 0; j < count; ++j) {
    for (const LongSeg& s : plans[j].long_segs) {
      BatchLongSeg b{s, j, 0};
      b.seg.slot += m.slot_keys;
      m.segs.push_back(b);
    }
    m.slot_keys += plans[j].slot_keys;
    if (plans[j].max_pow2 > m.max_pow2) m.max_pow2 = plans[j].max_pow2;
  }
}

// elements to allocate for a buffer that must hold `need`: an eighth more, so that calls of slowly growing size do not reallocate
inline size_t grown(size_t need) { return need + need / 8 + 16; }

// entries the caller's arrays must hold for gorio_search_radius_get
inline bool capacity_ok(long long capacity, long long total) { return capacity >= total; }

}  // namespace search_plan
}  // namespace gorio
