// batch_rounds.h -- the round table of the lock-step batched aligns (GICP_OMP, ICP, FastGICPMultiPoints): which workgroup of a round's
// launch works on which block of which job, and the capacity arithmetic.  Host code only, nothing of HIP: apd_batch_rounds.hip includes it,
// and host/test/batch_round_table.cpp runs it alone (and under the sanitizers).
//
// A round holds one job per pending handle.  Job k owns nwg[k] workgroups of the round's main launch, [first[k], first[k] + nwg[k]); its
// blocks b < nblk[k] <= nwg[k] each own the partial slot first[k] + b, the workgroups behind them write no partial (ICP's padding of the
// index-ordered copy).  The table the device reads is one byte array:
//   [Job x njobs][BlockRef x wg][BlockRef x second]
// first list    job 0's nwg[0] refs (0, 0) .. (0, nwg[0] - 1), then job 1's, ...: entry i is workgroup i of the main launch
// second list   behind the first: the nblk blocks of the MARKED jobs only, in job order (ICP's reciprocal launch)
// Jobs [0, n_leading) form the leading class, the others the trailing one; the trailing refs start at lead_wg, so a launch of
// wg - lead_wg workgroups over refs + lead_wg covers exactly them (GICP_OMP: the updates lead, the evaluations trail).
// What the kernels rely on, for every ref of either list: 0 <= job < njobs and 0 <= blk < nwg[job].
#pragma once
#include <climits>
#include <cstddef>

namespace gorio {
namespace batch_rounds {

struct alignas(8) BlockRef {
  int job, blk;  // blk: job-local
};
static_assert(sizeof(BlockRef) == 8 && alignof(BlockRef) == 8, "size and alignment of int2: the kernels fetch a ref as one 8-byte word");

struct JobShape {
  int nblk;     // blocks that own a partial slot
  int nwg;      // workgroups of the main launch, >= nblk
  bool marked;  // the job's blocks go on the second list too
};

struct Round {
  int njobs = 0;
  int n_leading = 0;  // jobs of the leading class
  int lead_wg = 0;    // their workgroups
  int wg = 0;         // workgroups of the main launch = refs of the first list = partial slots in use
  int second = 0;     // refs of the second list
  size_t bytes(size_t job_size) const { return job_size * (size_t)njobs + sizeof(BlockRef) * ((size_t)wg + (size_t)second); }
};

// first[njobs] and refs[wg + second] from the shapes.  refs must hold max_refs() of the call's all-pending round.
inline Round plan_round(const JobShape* shape, int njobs, int n_leading, int* first, BlockRef* refs) {
  Round r;
  r.njobs = njobs;
  r.n_leading = n_leading < njobs ? n_leading : njobs;
  for (int k = 0; k < njobs; ++k) {
    first[k] = r.wg;
    for (int b = 0; b < shape[k].nwg; ++b) refs[r.wg + b] = BlockRef{k, b};
    r.wg += shape[k].nwg;
  }
  r.lead_wg = r.n_leading < njobs ? first[r.n_leading] : r.wg;
  for (int k = 0; k < njobs; ++k)
    if (shape[k].marked)
      for (int b = 0; b < shape[k].nblk; ++b) refs[r.wg + r.second++] = BlockRef{k, b};
  return r;
}

// Capacity: everything is reserved once per call for the largest possible round, every handle pending -- `count` jobs and total_wg
// workgroups (the sum of nwg over ALL handles); a second list can at most repeat the first.  Buffers grow by a quarter.
inline size_t max_refs(size_t total_wg, bool second_list) { return second_list ? 2 * total_wg : total_wg; }
inline size_t table_bytes(size_t job_size, size_t count, size_t total_wg, bool second_list) { return job_size * count + sizeof(BlockRef) * max_refs(total_wg, second_list); }
inline size_t grown(size_t x) { return x + x / 4; }
// The refusal: slot indices and byte offsets derived from them stay ints, so a batch whose all-pending round needs more than
// INT_MAX / divisor workgroups is refused before anything is reserved.  It fires at the first total ABOVE the cap, not at the cap.
inline size_t wg_cap(int divisor) { return (size_t)INT_MAX / (size_t)divisor; }
inline bool too_many_wg(size_t total_wg, int divisor) { return total_wg > wg_cap(divisor); }

}  // namespace batch_rounds
}  // namespace gorio
