// Stand-alone driver of csrc/batch_rounds.h (the round table of the lock-step batched aligns): host code only, nothing of HIP or the
// library.  One JSON line per case; tests/test_batch_round_table.py recomputes every number from the rules the header states.
#include <cstdio>
#include <vector>

#include "../../csrc/batch_rounds.h"

using namespace gorio::batch_rounds;

struct Handle {
  int n;       // source points
  int spad;    // length of the index-ordered copy (0: none); workgroups cover max(n, spad)
  int marked;  // on the second list
};

static void print_list(const char* key, const std::vector<int>& v) {
  std::printf(", \"%s\": [", key);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%d", i ? ", " : "", v[i]);
  std::printf("]");
}

// A call over `all` handles of which `pending` (indices into all, the leading class first) have a job in the round.
static void run_case(const char* name, const std::vector<Handle>& all, const std::vector<int>& pending, int n_leading, bool second_list, size_t job_size) {
  size_t total_wg = 0;
  for (const Handle& h : all) total_wg += (size_t)((h.n > h.spad ? h.n : h.spad) + 255) / 256;
  const int njobs = (int)pending.size();
  std::vector<JobShape> shape(njobs);
  std::vector<int> n, spad, marked, nblk, nwg;
  for (int k = 0; k < njobs; ++k) {
    const Handle& h = all[pending[k]];
    shape[k] = JobShape{(h.n + 255) / 256, ((h.n > h.spad ? h.n : h.spad) + 255) / 256, h.marked != 0};
    n.push_back(h.n), spad.push_back(h.spad), marked.push_back(h.marked), nblk.push_back(shape[k].nblk), nwg.push_back(shape[k].nwg);
  }
  std::vector<int> first(njobs);
  std::vector<BlockRef> refs(max_refs(total_wg, second_list));  // exactly the reserved size: the sanitizers see a write past it
  const Round r = plan_round(shape.data(), njobs, n_leading, first.data(), refs.data());
  std::vector<int> rj, rb;
  for (int i = 0; i < r.wg + r.second; ++i) rj.push_back(refs[i].job), rb.push_back(refs[i].blk);
  std::vector<int> all_n, all_spad;
  for (const Handle& h : all) all_n.push_back(h.n), all_spad.push_back(h.spad);
  std::printf("{\"case\": \"%s\", \"njobs\": %d, \"n_leading_in\": %d, \"second_list\": %d, \"job_size\": %zu", name, r.njobs, n_leading, second_list ? 1 : 0, job_size);
  print_list("all_n", all_n), print_list("all_spad", all_spad);
  print_list("n", n), print_list("spad", spad), print_list("marked", marked), print_list("nblk", nblk), print_list("nwg", nwg), print_list("first", first);
  print_list("ref_job", rj), print_list("ref_blk", rb);
  std::printf(", \"n_leading\": %d, \"lead_wg\": %d, \"wg\": %d, \"second\": %d, \"bytes\": %zu, \"reserved\": %zu, \"grown\": %zu}\n", r.n_leading, r.lead_wg, r.wg, r.second,
              r.bytes(job_size), table_bytes(job_size, all.size(), total_wg, second_list), grown(table_bytes(job_size, all.size(), total_wg, second_list)));
}

int main() {
  static_assert(sizeof(BlockRef) == 8 && alignof(BlockRef) == 8, "int2");
  run_case("block_edges", {{1, 0, 0}, {255, 0, 0}, {256, 0, 0}, {257, 0, 0}}, {0, 1, 2, 3}, 4, false, 128);
  run_case("padding_blocks", {{3, 512, 0}, {257, 512, 0}, {700, 0, 0}}, {0, 1, 2}, 3, true, 176);
  run_case("second_list", {{300, 512, 1}, {600, 1024, 0}, {3, 512, 1}, {257, 0, 0}}, {0, 1, 2, 3}, 4, true, 176);
  run_case("second_list_subset", {{300, 512, 1}, {600, 1024, 1}, {3, 512, 1}, {257, 0, 0}}, {0, 2, 3}, 3, true, 176);
  run_case("two_classes", {{257, 0, 0}, {1, 0, 0}, {513, 0, 0}, {256, 0, 0}, {1000, 0, 0}}, {1, 3, 0, 2, 4}, 2, false, 240);
  run_case("all_trailing", {{257, 0, 0}, {1, 0, 0}}, {0, 1}, 0, false, 240);
  run_case("one_job", {{257, 0, 0}, {5, 0, 0}}, {1}, 1, false, 128);
  run_case("no_job", {{257, 0, 0}, {5, 0, 0}}, {}, 0, false, 128);
  for (int divisor : {16, 32}) {
    const size_t cap = wg_cap(divisor);
    std::printf("{\"case\": \"overflow_%d\", \"divisor\": %d, \"cap\": %zu, \"below\": %d, \"at_cap\": %d, \"above\": %d, \"far_above\": %d}\n", divisor, divisor, cap,
                too_many_wg(cap - 1, divisor) ? 1 : 0, too_many_wg(cap, divisor) ? 1 : 0, too_many_wg(cap + 1, divisor) ? 1 : 0, too_many_wg((size_t)1 << 40, divisor) ? 1 : 0);
  }
  return 0;
}
