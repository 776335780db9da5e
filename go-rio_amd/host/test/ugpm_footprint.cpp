// ugpm_footprint.cpp -- the rule that picks the instantiations of the GP solver kernels (solver_sizes, csrc/ugpm_windows.h) alone on
// the host (no HIP, no library).  For every number of states given on the command line it prints one JSON line with what the rule
// returns, sized and with the full capacities, and with the header's own statements of what a window needs.
// tests/test_ugpm_footprint.py builds it plain and with -fsanitize=address,undefined and checks the output against a restatement of
// block_cholesky's and blocked_lower_solve16's index arithmetic.
//   ugpm_footprint S_first S_last -> {"S":..,"sized":{..},"full":{..},"need":{..}} per S
#include <cstdio>
#include <cstdlib>

#include "../../csrc/ugpm_windows.h"

using namespace gorio;
using namespace gorio::windows;

static void print_sizes(const char* name, const SolverSizes& z) {
  std::printf("\"%s\":{\"gram_rows\":%d,\"gram_kmax\":%d,\"lm_rows\":%d,\"solve_kmax\":%d}", name, z.gram_rows, z.gram_kmax, z.lm_rows, z.solve_kmax);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: ugpm_footprint S_first S_last\n");
    return 2;
  }
  const int s0 = std::atoi(argv[1]), s1 = std::atoi(argv[2]);
  std::printf("{\"instantiations\":{\"gram\":[[%d,%d],[%d,%d],[%d,%d]],\"lm\":[%d,%d],\"solve\":[%d,%d]},\"max_states\":%d}\n", kGramRowsSmall, kGramKmax, kGramRows, kGramKmax,
              kCholRowsFull, kSolveKmaxFull, kLmRowsSmall, kCholRowsFull, kSolveKmaxSmall, kSolveKmaxFull, kMaxStates);
  for (int S = s0; S <= s1; ++S) {
    std::printf("{\"S\":%d,", S);
    print_sizes("sized", solver_sizes(S, false));
    std::printf(",");
    print_sizes("full", solver_sizes(S, true));
    std::printf(",\"need\":{\"gram_rows\":%d,\"lm_rows\":%d,\"gram_blocks\":%d,\"solve_blocks\":%d}}\n", gram_rows_needed(S), lm_rows_needed(S), solve16_blocks_needed(S),
                solve16_blocks_needed(6 * S));
  }
  return 0;
}
