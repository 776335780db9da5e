// knn_sort_network.h -- the fixed comparator network knn_collect_kernel<20> sorts its buffered keys with (apd_index.hip), in one text for
// the device code and for the host test (go-rio_amd/host/test/knn_sort_network.cpp).  Depends on nothing.
//
// The network takes kKnnSortWidth = 24 values (K + 4, the rows of the kernel's LDS buffer) and leaves the kKnnSortKeep = 20 smallest,
// ascending, in positions 0 .. 19; positions 20 .. 23 hold the other four in no particular order.  It is Batcher's merge exchange
// (Knuth, TAOCP 3, 5.2.2 Algorithm M) for 24 inputs, 127 comparators, without the one comparator (21, 22) of its last stage that feeds
// no kept output: 126 comparators, each {a, b} with a < b putting the smaller value at a.  A comparator network sorts every input if it
// sorts every input of zeros and ones, and that holds output by output, so the test's pass over all 2^24 of them is a proof.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GORIO_SORTNET_FN __host__ __device__ __forceinline__
#else
#define GORIO_SORTNET_FN inline
#endif

namespace gorio {

constexpr int kKnnSortWidth = 24;
constexpr int kKnnSortKeep = 20;

struct KnnComparator {
  unsigned char a, b;
};

constexpr KnnComparator kKnnSortNetwork[] = {
    {0, 16},  {1, 17},  {2, 18},  {3, 19},  {4, 20},  {5, 21},  {6, 22},  {7, 23},  {0, 8},   {1, 9},   {2, 10},  {3, 11},  {4, 12},  {5, 13},
    {6, 14},  {7, 15},  {8, 16},  {9, 17},  {10, 18}, {11, 19}, {12, 20}, {13, 21}, {14, 22}, {15, 23}, {0, 4},   {1, 5},   {2, 6},   {3, 7},
    {8, 12},  {9, 13},  {10, 14}, {11, 15}, {16, 20}, {17, 21}, {18, 22}, {19, 23}, {4, 16},  {5, 17},  {6, 18},  {7, 19},  {4, 8},   {5, 9},
    {6, 10},  {7, 11},  {12, 16}, {13, 17}, {14, 18}, {15, 19}, {0, 2},   {1, 3},   {4, 6},   {5, 7},   {8, 10},  {9, 11},  {12, 14}, {13, 15},
    {16, 18}, {17, 19}, {20, 22}, {21, 23}, {2, 16},  {3, 17},  {6, 20},  {7, 21},  {2, 8},   {3, 9},   {6, 12},  {7, 13},  {10, 16}, {11, 17},
    {14, 20}, {15, 21}, {2, 4},   {3, 5},   {6, 8},   {7, 9},   {10, 12}, {11, 13}, {14, 16}, {15, 17}, {18, 20}, {19, 21}, {0, 1},   {2, 3},
    {4, 5},   {6, 7},   {8, 9},   {10, 11}, {12, 13}, {14, 15}, {16, 17}, {18, 19}, {20, 21}, {22, 23}, {1, 16},  {3, 18},  {5, 20},  {7, 22},
    {1, 8},   {3, 10},  {5, 12},  {7, 14},  {9, 16},  {11, 18}, {13, 20}, {15, 22}, {1, 4},   {3, 6},   {5, 8},   {7, 10},  {9, 12},  {11, 14},
    {13, 16}, {15, 18}, {17, 20}, {19, 22}, {1, 2},   {3, 4},   {5, 6},   {7, 8},   {9, 10},  {11, 12}, {13, 14}, {15, 16}, {17, 18}, {19, 20}};
constexpr int kKnnSortComparators = (int)(sizeof(kKnnSortNetwork) / sizeof(kKnnSortNetwork[0]));
constexpr bool knn_sort_network_in_range() {
  for (int i = 0; i < kKnnSortComparators; ++i)
    if (!(kKnnSortNetwork[i].a < kKnnSortNetwork[i].b && kKnnSortNetwork[i].b < kKnnSortWidth)) return false;
  return true;
}
static_assert(knn_sort_network_in_range(), "every comparator {a, b} has a < b < kKnnSortWidth");

// Runs the network over v with exchange(lo, hi) as the comparator: it must leave min(lo, hi) in lo and max(lo, hi) in hi.  The
// positions are template constants, so v stays in registers on the device.
template <int I = 0, typename T, typename Exchange>
GORIO_SORTNET_FN void knn_sort_network(T (&v)[kKnnSortWidth], Exchange&& exchange) {
  if constexpr (I < kKnnSortComparators) {
    exchange(v[kKnnSortNetwork[I].a], v[kKnnSortNetwork[I].b]);
    knn_sort_network<I + 1>(v, exchange);
  }
}

}  // namespace gorio
