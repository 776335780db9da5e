// Stand-alone driver of the resumable Gauss-Newton shell of FastGICPMultiPoints (go-rio_amd/csrc/gicp_mp_machine.h).  Links nothing of HIP
// or the library; the Makefile also builds it with the sanitizers.  It reads cases from the file named on the command line -- per case the
// guess, the limits and, pass by pass, the 28 sums a pass produced -- feeds them to an MpMachine and prints, as bits, the pose the machine
// asked every pass at and what it ended with.  tests/test_gicp_mp_machine.py writes the file from tests/gicp_mp_restatement.py and
// compares every bit.
//   case <name> <max_iterations> <rotation_epsilon> <transformation_epsilon> <passes>
//   <16 floats of the guess>
//   <28 doubles> per pass                         (numbers as C99 hex floats, "nan" and "inf" included)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../csrc/gicp_mp_machine.h"

static bool next_number(FILE* f, double* v) {
  char tok[128];
  if (std::fscanf(f, "%127s", tok) != 1) return false;
  char* end = nullptr;
  *v = std::strtod(tok, &end);
  return end && *end == '\0';
}

static unsigned int fbits(float v) {
  unsigned int u;
  std::memcpy(&u, &v, 4);
  return u;
}
static unsigned long long dbits(double v) {
  unsigned long long u;
  std::memcpy(&u, &v, 8);
  return u;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: gicp_mp_machine <cases file>\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  char word[128], name[128];
  while (std::fscanf(f, "%127s", word) == 1) {
    if (std::strcmp(word, "case") != 0) {
      std::fprintf(stderr, "expected 'case', got '%s'\n", word);
      return 2;
    }
    int max_it = 0, passes = 0;
    double rot = 0.0, trans = 0.0, v = 0.0;
    if (std::fscanf(f, "%127s %d", name, &max_it) != 2 || !next_number(f, &rot) || !next_number(f, &trans) || std::fscanf(f, "%d", &passes) != 1 || passes < 0) {
      std::fprintf(stderr, "bad case header\n");
      return 2;
    }
    float guess[16];
    for (int i = 0; i < 16; ++i) {
      if (!next_number(f, &v)) return 2;
      guess[i] = (float)v;
    }
    std::vector<double> sums((size_t)28 * passes);
    for (double& s : sums)
      if (!next_number(f, &s)) return 2;
    gorio_mp::MpMachine mc;
    mc.begin(guess, max_it, rot, trans);
    std::printf("{\"case\": \"%s\", \"poses\": [", name);
    int fed = 0;
    while (!mc.done() && fed < passes) {
      float T12[12];
      mc.next_pose(T12);
      std::printf("%s[", fed ? ", " : "");
      for (int i = 0; i < 12; ++i) std::printf("%s%u", i ? ", " : "", fbits(T12[i]));
      std::printf("]");
      mc.consume(sums.data() + (size_t)28 * fed);
      ++fed;
    }
    float T[16];
    double H[36];
    int conv = -1, nr = -1, nlin = -1;
    mc.results(T, H, &conv, &nr, &nlin);
    std::printf("], \"fed\": %d, \"done\": %d, \"end\": %d, \"converged\": %d, \"nr_iterations\": %d, \"n_linearize\": %d, \"T\": [", fed, mc.done() ? 1 : 0, (int)mc.end, conv, nr, nlin);
    for (int i = 0; i < 16; ++i) std::printf("%s%u", i ? ", " : "", fbits(T[i]));
    std::printf("], \"H\": [");
    for (int i = 0; i < 36; ++i) std::printf("%s%llu", i ? ", " : "", dbits(H[i]));
    std::printf("]}\n");
  }
  std::fclose(f);
  return 0;
}
