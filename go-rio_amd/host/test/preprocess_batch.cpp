// gorio::ScanPreprocessor::processBatch against process_packed: the messages of a file go (A) through one processBatch call over one object
// per message and (B) through process_packed of a second set of objects, one after another; both draw their RANSAC samples from
// std::mt19937 engines with one seed.  A second frame sends the messages through the same objects in rotated order, so each object's
// Patchwork++ state takes part.  For every frame and message the driver prints
//   <A|B> <frame> <message> <status> <n_ground> <n_clusters> <sha256 of v_r, sigma_v_r and the published cloud, or - without a cloud> <text of a refusal>
// and the caller compares the A lines with the B lines.
//
// Input (binary), the format of preprocess_sequence: [int32 F][double R[9]][int32 dynamic_object_removal][int32 outlier_method]
//                 [int32 have_ang_vel][double ang_vel[3]][uint32 seed], then per message [int32 n][n x (x, y, z, power, doppler) float].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include <pcl/point_types.h>
#include <radar_preprocessing/scan_preprocessor.hpp>

using PointT = pcl::PointXYZINormal;
using Pre = gorio::ScanPreprocessor<PointT>;

// SHA-256 (FIPS 180-4)
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  unsigned char buf[64];
  uint64_t len = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const unsigned char* p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u,
        0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du,
        0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu,
        0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u,
        0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g), t1 = hh + S1 + ch + K[i] + w[i];
      const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & b) ^ (a & c) ^ (b & c), t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
  void update(const void* data, std::size_t n) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (std::size_t i = 0; i < n; ++i) {
      buf[len++ % 64] = p[i];
      if (len % 64 == 0) block(buf);
    }
  }
  std::string hex() {
    const uint64_t bits = len * 8;
    const unsigned char one = 0x80, zero = 0;
    update(&one, 1);
    while (len % 64 != 56) update(&zero, 1);
    unsigned char be[8];
    for (int i = 0; i < 8; ++i) be[i] = (unsigned char)(bits >> (56 - 8 * i));
    update(be, 8);
    char out[65];
    for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

static void print(char side, int frame, int msg, const Pre::Result& r, const Pre& pre) {
  std::string digest = "-";
  if (r.full_scan) {
    Sha256 s;
    s.update(r.v_r, sizeof(r.v_r));
    s.update(r.sigma_v_r, sizeof(r.sigma_v_r));
    for (const PointT& p : r.full_scan->points) {
      const float v[6] = {p.x, p.y, p.z, p.intensity, p.curvature, p.normal_x};
      s.update(v, sizeof(v));
    }
    digest = s.hex();
    if (pre.last_scan() != r.full_scan) digest += "(last_scan differs)";
  } else if (pre.last_scan()) {
    digest = "-(last_scan set)";
  }
  std::printf("%c %d %d %d %d %d %s %s\n", side, frame, msg, r.status, r.n_ground, r.n_clusters, digest.c_str(), r.message.c_str());
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s scans.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int F = 0, dor = 0, method = 0, have_w = 0;
  double R[9], w[3];
  unsigned int seed = 0;
  if (std::fread(&F, 4, 1, f) != 1 || F < 0 || std::fread(R, 8, 9, f) != 9 || std::fread(&dor, 4, 1, f) != 1 || std::fread(&method, 4, 1, f) != 1 ||
      std::fread(&have_w, 4, 1, f) != 1 || std::fread(w, 8, 3, f) != 3 || std::fread(&seed, 4, 1, f) != 1)
    return 2;
  std::vector<std::vector<float>> msgs(F);
  for (int s = 0; s < F; ++s) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    msgs[s].resize(5 * (std::size_t)n);
    if (n && std::fread(msgs[s].data(), 4, msgs[s].size(), f) != msgs[s].size()) return 2;
  }
  std::fclose(f);
  try {
    gorio_scan_params P = Pre::defaults();
    std::memcpy(P.rotation, R, sizeof(R));
    P.enable_dynamic_object_removal = dor;
    P.outlier_method = method;
    std::vector<std::unique_ptr<Pre>> a, b;
    std::vector<Pre*> ap;
    for (int s = 0; s < F; ++s) {
      a.emplace_back(new Pre(P));
      b.emplace_back(new Pre(P));
      ap.push_back(a.back().get());
    }
    std::mt19937 rngA(seed), rngB(seed);
    for (int frame = 0; frame < 2; ++frame) {
      std::vector<const float*> raw(F);
      std::vector<int> n(F);
      std::vector<const double*> av(F, have_w ? w : nullptr);
      for (int s = 0; s < F; ++s) {
        const std::vector<float>& m = msgs[(s + frame) % F];  // object s: message s, then message s + 1
        raw[s] = m.empty() ? nullptr : m.data();
        n[s] = (int)(m.size() / 5);
      }
      const std::vector<Pre::Result> ra = Pre::processBatch(ap, raw, n, av, rngA);
      for (int s = 0; s < F; ++s) print('A', frame, s, ra[s], *a[s]);
      for (int s = 0; s < F; ++s) print('B', frame, s, b[s]->process_packed(raw[s], n[s], av[s], rngB), *b[s]);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "preprocess_batch: %s\n", e.what());
    return 3;
  }
  return 0;
}
