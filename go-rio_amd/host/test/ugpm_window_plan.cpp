// ugpm_window_plan.cpp -- the window bookkeeping of the UGPM back end (csrc/ugpm_windows.h) alone on the host: no HIP, no library.
// Reads windows from a file and prints one JSON line per window: the plan (status, S, state rate, sample slices, state time line, slab
// size), the layout carve() gives a real slab, the staged input block byte for byte, and for LPM windows the merged time line with the
// layout of its scratch.  tests/test_ugpm_window_plan.py builds it plain and with -fsanitize=address,undefined and checks the output.
//
// File: int32 n_windows, then per window int32[7] {n_gyr, n_vel, n_infer, type, correlate, overlap, n_groups}, double[6] {gyr_var,
// vel_var, start_t, min_freq, quantum, state_freq}, gyr_t[n_gyr], gyr[3 n_gyr], vel_t[n_vel], vel[3 n_vel], infer_t[n_infer],
// int32 group_sizes[n_groups].
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../csrc/ugpm_windows.h"

using namespace gorio;
using namespace gorio::windows;

namespace {

struct LpmLayout {  // the pointer members of ug::LpmOutWin that carve_lpm fills
  const double *gyr_t, *gyr, *vel_t, *vel, *infer_t, *tl;
  const int *kind, *kidx, *qpos, *qorder, *qrot;
  double *E, *B, *cov3, *dRdt, *dRdbw, *velr, *d_bw, *d_dt, *dp_shift;
};

template <typename T>
bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

void print_hex(const char* key, const std::vector<double>& v) {
  std::printf(",\"%s\":\"", key);
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t k = 0; k < v.size() * sizeof(double); ++k) std::printf("%02x", p[k]);
  std::printf("\"");
}

void print_ints(const char* key, const std::vector<int>& v) {
  std::printf(",\"%s\":[", key);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%d", k ? "," : "", v[k]);
  std::printf("]");
}

template <typename T>
void print_offsets(const char* key, const T* base, const std::vector<std::pair<const char*, const T*>>& fields) {
  std::printf(",\"%s\":{", key);
  bool first = true;
  for (const auto& f : fields) {
    if (!f.second) continue;  // not carved (Jc / Ac without correlate)
    std::printf("%s\"%s\":%ld", first ? "" : ",", f.first, (long)(f.second - base));
    first = false;
  }
  std::printf("}");
}

void report_ugpm(const gorio_ugpm_window& w, const HostWin& h) {
  std::printf(",\"S\":%d,\"state_freq\":%.17g,\"g0\":%d,\"G\":%d,\"v0\":%d,\"V\":%d,\"ws_doubles\":%zu", h.S, h.state_freq, h.g0, h.G, h.v0, h.V, h.ws_doubles);
  print_hex("state_t", h.state_t);
  std::vector<double> slab(h.ws_doubles), staged(input_slot(w, h), -1.0), out(1);
  UgpmWin u;
  std::memset(&u, 0, sizeof(u));
  const size_t used = carve(w, h, u, slab.data(), staged.data(), out.data());
  std::printf(",\"used\":%zu,\"input_doubles\":%zu", used, input_doubles(w, h));
  print_offsets<double>("in", staged.data(), {{"gyr_t", u.gyr_t}, {"gyr", u.gyr}, {"vel_t", u.vel_t}, {"vel", u.vel}, {"infer_t", u.infer_t}, {"state_t", u.state_t}});
  print_offsets<double>("ws", slab.data(),
                        {{"Rq", u.Rq}, {"Rstart", u.Rstart}, {"velr", u.velr}, {"dp", u.dp}, {"r0", u.r0}, {"r1", u.r1}, {"s_dr", u.s_dr}, {"s_vel", u.s_vel}, {"hyper", u.hyper},
                         {"d_r_dt_local", u.d_r_dt_local}, {"d_r_dt_local_shift", u.d_r_dt_local_shift}, {"delta_r_time", u.delta_r_time}, {"delta_r_bw", u.delta_r_bw},
                         {"d_r_bw_local_shift", u.d_r_bw_local_shift}, {"Kinv", u.Kinv}, {"KKinv", u.KKinv}, {"KintKinv", u.KintKinv}, {"var", u.var}, {"wgp", u.wgp}, {"sstd", u.sstd},
                         {"KsKinv", u.KsKinv}, {"KsIntKinv", u.KsIntKinv}, {"KgyrIntKinv", u.KgyrIntKinv}, {"KvelKinv", u.KvelKinv}, {"Jrot", u.Jrot}, {"Jvel", u.Jvel}, {"res", u.res},
                         {"res_new", u.res_new}, {"JtJ", u.JtJ}, {"lhs", u.lhs}, {"lmv", u.lmv}, {"sample_tmp", u.sample_tmp}, {"sample_tmp_c", u.sample_tmp_c}, {"Jc", u.Jc}, {"Ac", u.Ac},
                         {"dsc", u.dsc}, {"alpha", u.alpha}, {"state_r", u.state_r}, {"d_state_bw", u.d_state_bw}, {"d_d_r_dt", u.d_d_r_dt}, {"d_vel_bv", u.d_vel_bv},
                         {"d_vel_bw", u.d_vel_bw}, {"d_vel_dt", u.d_vel_dt}, {"lmc", u.lmc}});
  // the input slot as the batch call fills it: the padding, the samples, the state time line
  for (size_t k = staged.size() - 4; k < staged.size(); ++k) staged[k] = 0.0;
  double* s = stage_samples(staged.data(), w, h.g0, h.G, h.v0, h.V);
  std::copy(h.state_t.begin(), h.state_t.end(), s);
  print_hex("staged", staged);
}

void report_lpm(const gorio_ugpm_window& w) {
  LpmHost L;
  build_lpm_timeline(w, L);
  const size_t T = L.tl.size();
  LpmLayout u;
  std::memset(&u, 0, sizeof(u));
  const LpmSize sz = carve_lpm(w, T, u, nullptr, nullptr, nullptr);
  std::vector<double> staged(sz.in, -1.0), scratch(sz.scratch);
  std::vector<int> tables(sz.ints, -1);
  const LpmSize used = carve_lpm(w, T, u, staged.data(), scratch.data(), tables.data());
  std::printf(",\"T\":%zu,\"start_index\":%d,\"dt_index\":%d,\"size\":[%zu,%zu,%zu],\"used\":[%zu,%zu,%zu]", T, L.start_index, L.dt_index, sz.in, sz.scratch, sz.ints, used.in,
              used.scratch, used.ints);
  print_ints("kind", L.kind);
  print_ints("kidx", L.kidx);
  print_ints("qpos", L.qpos);
  print_ints("qorder", L.qorder);
  print_ints("qrot", L.qrot);
  print_offsets<double>("in", staged.data(), {{"gyr_t", u.gyr_t}, {"gyr", u.gyr}, {"vel_t", u.vel_t}, {"vel", u.vel}, {"infer_t", u.infer_t}, {"tl", u.tl}});
  print_offsets<int>("ints", tables.data(), {{"kind", u.kind}, {"kidx", u.kidx}, {"qpos", u.qpos}, {"qorder", u.qorder}, {"qrot", u.qrot}});
  print_offsets<double>("ws", scratch.data(),
                        {{"E", u.E}, {"B", u.B}, {"cov3", u.cov3}, {"dRdt", u.dRdt}, {"dRdbw", u.dRdbw}, {"velr", u.velr}, {"d_bw", u.d_bw}, {"d_dt", u.d_dt}, {"dp_shift", u.dp_shift}});
  std::copy(L.tl.begin(), L.tl.end(), stage_samples(staged.data(), w, 0, w.n_gyr, 0, w.n_vel));
  stage_lpm_tables(tables.data(), L);
  print_hex("staged", staged);
  print_ints("tables", tables);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: ugpm_window_plan windows.bin\n");
    return 2;
  }
  FILE* f = std::fopen(argv[1], "rb");
  int n_windows = 0;
  if (!f || std::fread(&n_windows, sizeof(int), 1, f) != 1) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  for (int i = 0; i < n_windows; ++i) {
    int hdr[7];
    double opt[6];
    std::vector<double> gyr_t, gyr, vel_t, vel, infer_t;
    std::vector<int> groups;
    bool ok = std::fread(hdr, sizeof(int), 7, f) == 7 && std::fread(opt, sizeof(double), 6, f) == 6;
    for (int k = 0; ok && k < 3; ++k) ok = hdr[k] >= 0;
    ok = ok && hdr[6] >= 0 && read_n(f, gyr_t, hdr[0]) && read_n(f, gyr, 3 * (size_t)hdr[0]) && read_n(f, vel_t, hdr[1]) && read_n(f, vel, 3 * (size_t)hdr[1]) &&
         read_n(f, infer_t, hdr[2]) && read_n(f, groups, hdr[6]);
    if (!ok) {
      std::fprintf(stderr, "window %d: short or malformed record\n", i);
      return 2;
    }
    gorio_ugpm_window w;
    std::memset(&w, 0, sizeof(w));
    w.gyr_t = gyr_t.data(); w.gyr = gyr.data(); w.n_gyr = hdr[0];
    w.vel_t = vel_t.data(); w.vel = vel.data(); w.n_vel = hdr[1];
    w.infer_t = infer_t.data(); w.n_infer = hdr[2];
    w.type = hdr[3]; w.correlate = hdr[4]; w.overlap = hdr[5];
    w.group_sizes = groups.empty() ? nullptr : groups.data(); w.n_groups = hdr[6];
    w.gyr_var = opt[0]; w.vel_var = opt[1]; w.start_t = opt[2]; w.min_freq = opt[3]; w.quantum = opt[4]; w.state_freq = opt[5];
    HostWin h;
    std::string err;
    const int status = plan_window(w, h, err);
    std::printf("{\"status\":%d,\"h_status\":%d,\"err\":\"%s\",\"is_lpm\":%d", status, h.status, err.c_str(), h.is_lpm ? 1 : 0);
    if (status == 0 && h.is_lpm) report_lpm(w);
    else if (status == 0) report_ugpm(w, h);
    std::printf("}\n");
  }
  std::fclose(f);
  return 0;
}
