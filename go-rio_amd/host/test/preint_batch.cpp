// ugpm::VelPreintegration::batch against single constructions: K requests (UGPM, LPM and chunked ones mixed) are constructed one by
// one, as the back end does per keyframe (radar_graph_slam_nodelet.cpp:497-513), and once more through ONE VelPreintegration::batch.
// Input: binary [int32 K], then per request [int32 n_g][n_g x (t, wx, wy, wz) double][int32 n_v][n_v x (t, vx, vy, vz) double]
// [double start_t][int32 type (0 LPM, 1 UGPM)][double quantum][int32 n_groups] and per group [int32 size][size x double stamps].
// Output: one JSON line per request and mode with every record of get(i, j, 0, 0) and the inflated covariance of get(i, j).
// With a second argument "errors" the requests are expected to contain a failing one: the line reports the exception type of the first
// failing single construction (and its index) and the type and message of the batch's exception.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <VelInt/preint.h>

using ugpm::VelPreintegration;

static bool read_samples(std::FILE* f, std::vector<ugpm::DataSample>& out) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return false;
  for (int i = 0; i < n; ++i) {
    double r[4];
    if (std::fread(r, 8, 4, f) != 4) return false;
    ugpm::DataSample s;
    s.t = r[0]; s.data[0] = r[1]; s.data[1] = r[2]; s.data[2] = r[3];
    out.push_back(s);
  }
  return true;
}

static void print_meas(const ugpm::PreintMeas& m) {
  std::printf("[");
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) std::printf("%.17g, ", m.delta_R(r, c));
  for (int r = 0; r < 3; ++r) std::printf("%.17g, ", m.delta_p(r, 0));
  std::printf("%.17g, %.17g", m.dt, m.dt_sq_half);
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) std::printf(", %.17g", m.cov(r, c));
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) std::printf(", %.17g, %.17g, %.17g", m.d_delta_R_d_bw(r, c), m.d_delta_p_d_bw(r, c), m.d_delta_p_d_bv(r, c));
    std::printf(", %.17g, %.17g", m.d_delta_R_d_t(r, 0), m.d_delta_p_d_t(r, 0));
  }
  std::printf("]");
}

static void print(const char* mode, size_t k, VelPreintegration& p, const std::vector<std::vector<double> >& infer_t) {
  std::printf("{\"mode\": \"%s\", \"k\": %zu, \"records\": [", mode, k);
  for (size_t i = 0; i < infer_t.size(); ++i)
    for (size_t j = 0; j < infer_t[i].size(); ++j) {
      if (i || j) std::printf(", ");
      print_meas(p.get(static_cast<int>(i), static_cast<int>(j), 0.0, 0.0));
    }
  std::printf("], \"inflated\": [");
  for (size_t i = 0; i < infer_t.size(); ++i)
    for (size_t j = 0; j < infer_t[i].size(); ++j) {
      if (i || j) std::printf(", ");
      print_meas(p.get(static_cast<int>(i), static_cast<int>(j)));  // default bias stds (PRE:55)
    }
  // the other two overloads refuse on an object of the first constructor (PRE:1769-1781)
  int refused = 0;
  try { p.get(0); } catch (const std::range_error&) { ++refused; }
  try { p.get(); } catch (const std::range_error&) { ++refused; }
  std::printf("], \"overloads_refused\": %d}\n", refused);
}

// the exception type a construction throws, most derived first
template <typename F>
static std::string thrown(F&& f, std::string* what = nullptr) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    if (what) *what = e.what();
    return "invalid_argument";
  } catch (const std::range_error& e) {
    if (what) *what = e.what();
    return "range_error";
  } catch (const std::runtime_error& e) {
    if (what) *what = e.what();
    return "runtime_error";
  }
  return "";
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s requests.bin [errors]\n", argv[0]);
    return 2;
  }
  const bool errors = argc > 2 && std::strcmp(argv[2], "errors") == 0;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int K = 0;
  if (std::fread(&K, 4, 1, f) != 1 || K <= 0) return 2;
  std::vector<VelPreintegration::BatchArgs> args(K);
  for (int k = 0; k < K; ++k) {
    VelPreintegration::BatchArgs& a = args[k];
    if (!read_samples(f, a.imu_data.gyr) || !read_samples(f, a.imu_data.vel)) return 2;
    a.imu_data.gyr_var = 1.74532925e-03;  // RGS:476
    a.imu_data.vel_var = 1e-6;            // RGS:493
    int type = 1, n_groups = 0;
    if (std::fread(&a.start_t, 8, 1, f) != 1 || std::fread(&type, 4, 1, f) != 1 || std::fread(&a.opt.quantum, 8, 1, f) != 1 || std::fread(&n_groups, 4, 1, f) != 1) return 2;
    a.opt.type = type ? ugpm::UGPM : ugpm::LPM;
    for (int g = 0; g < n_groups; ++g) {
      int sz = 0;
      if (std::fread(&sz, 4, 1, f) != 1 || sz < 0) return 2;
      std::vector<double> grp(sz);
      if (std::fread(grp.data(), 8, sz, f) != (size_t)sz) return 2;
      a.infer_t.push_back(grp);
    }
  }
  std::fclose(f);

  auto single = [&](int k) { return VelPreintegration(args[k].imu_data, args[k].start_t, args[k].infer_t, args[k].opt, args[k].prior, true, args[k].overlap, args[k].device); };
  if (errors) {
    int bad = -1;
    std::string single_type, single_what;
    for (int k = 0; k < K && bad < 0; ++k) {
      single_type = thrown([&] { single(k); }, &single_what);
      if (!single_type.empty()) bad = k;
    }
    if (single_what.find("no usable HIP device") != std::string::npos) {
      std::fprintf(stderr, "%s\n", single_what.c_str());
      return 3;
    }
    std::string batch_what;
    const std::string batch_type = thrown([&] { VelPreintegration::batch(args); }, &batch_what);
    std::string esc;
    for (char c : batch_what) esc += (c == '"' || c == '\\') ? ' ' : c;
    std::printf("{\"single_index\": %d, \"single_error\": \"%s\", \"batch_error\": \"%s\", \"batch_message\": \"%s\"}\n", bad, single_type.c_str(), batch_type.c_str(), esc.c_str());
    return 0;
  }
  try {
    for (int k = 0; k < K; ++k) {
      VelPreintegration p = single(k);
      print("single", k, p, args[k].infer_t);
    }
    std::vector<VelPreintegration> batch = VelPreintegration::batch(args);
    for (int k = 0; k < K; ++k) print("batch", k, batch[k], args[k].infer_t);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-in refuses instead of falling back to a CPU path
  }
  return 0;
}
