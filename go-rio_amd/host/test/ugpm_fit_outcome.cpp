// ugpm_fit_outcome.cpp -- two pieces of host logic of the UGPM back end alone on the host (no HIP, no library):
//  * fit_outcome (csrc/ugpm_windows.h): which windows of a batch whose fits were enqueued without a look at the done flags have to
//    run again, and the iteration budget the batch leaves for the next one;
//  * ata_cut (csrc/ugpm_device.h): how the output tiles of a J^T J are cut into workgroups, with and without the zero columns.
// Reads commands from a text file and prints one JSON line per command.  tests/test_ugpm_fit_outcome.py builds it plain and with
// -fsanitize=address,undefined and checks the output.
//   batch N, then N lines "host_status is_lpm device_status need_rot need_vel" -> {"rerun":[...],"need":[r,v]}
//   cut n zero_col tpg -> {"ntile":..,"q_zero":..,"ng_dense":..,"ng_skip":..,"lo":[..],"hi":[..],"skips":[..]}
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../csrc/ugpm_windows.h"

using namespace gorio;
using namespace gorio::windows;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: ugpm_fit_outcome commands.txt\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  char cmd[16];
  while (std::fscanf(f, "%15s", cmd) == 1) {
    if (!std::strcmp(cmd, "batch")) {
      int n = 0;
      if (std::fscanf(f, "%d", &n) != 1 || n < 0) return 2;
      std::vector<HostWin> hw(n);
      std::vector<int> ints(kWinInts * (size_t)n, -12345);  // words fit_outcome has no business reading stand out
      for (int i = 0; i < n; ++i) {
        int hs, lpm, ds, n0, n1;
        if (std::fscanf(f, "%d %d %d %d %d", &hs, &lpm, &ds, &n0, &n1) != 5) return 2;
        hw[i].status = hs;
        hw[i].is_lpm = lpm != 0;
        int* w = ints.data() + kWinInts * (size_t)i;
        w[16] = ds; w[kLmiNeed] = n0; w[kLmiNeed + 1] = n1;
      }
      const FitOutcome o = fit_outcome(ints.data(), hw);
      std::printf("{\"rerun\":[");
      for (size_t k = 0; k < o.rerun.size(); ++k) std::printf("%s%d", k ? "," : "", o.rerun[k]);
      std::printf("],\"need\":[%d,%d]}\n", o.need[0], o.need[1]);
    } else if (!std::strcmp(cmd, "cut")) {
      int n, zc, tpg;
      if (std::fscanf(f, "%d %d %d", &n, &zc, &tpg) != 3) return 2;
      const AtaCut c = ata_cut(n, zc, tpg);
      std::printf("{\"ntile\":%d,\"q_zero\":%d,\"ng_dense\":%d,\"ng_skip\":%d", c.ntile, c.q_zero, c.ng_dense, c.ng_skip);
      for (int what = 0; what < 3; ++what) {
        std::printf(",\"%s\":[", what == 0 ? "lo" : (what == 1 ? "hi" : "skips"));
        for (int g = 0; g < c.groups(); ++g) std::printf("%s%d", g ? "," : "", what == 0 ? c.q_lo(g) : (what == 1 ? c.q_hi(g) : (int)c.skips(g)));
        std::printf("]");
      }
      std::printf("}\n");
    } else {
      std::fprintf(stderr, "unknown command %s\n", cmd);
      return 2;
    }
  }
  std::fclose(f);
  return 0;
}
