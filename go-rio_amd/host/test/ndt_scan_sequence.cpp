// Replays the front end with the factory's default registration (registrations.cpp:27, 102-135: NDT_OMP): a sequence of raw radar
// messages through gorio::ScanPreprocessor, each frame registered against the frame before it (the keyframe) and scored with
// getFitnessScore (scan_matching_odometry_nodelet.cpp:675), then one scan-to-submap step (scan_matching_odometry_nodelet.cpp:602-618)
// over the last keyframes.  Two pclomp::NormalDistributionsTransform objects see the same frames:
//   route A  setInputSourceFromScan / setInputTargetFromScan (the frame stays on the device), setInputTargetSubmap;
//   route B  setInputSource / setInputTarget with pre.last_scan(), and setInputTarget with the assembled submap cloud.
// Input (binary, the format of preprocess_sequence): [int32 F][double R[9]][int32 dynamic_object_removal][int32 outlier_method]
//                 [int32 have_ang_vel][double ang_vel[3]][uint32 seed], then per message [int32 n][n x (x, y, z, power, doppler) float].
// argv[2] = resolution, argv[3] = voxel leaf of the submap step (0: none).
// Output: one JSON line per frame and route, and one per route for the submap step: the pose as the bit patterns of its 16 floats, the
// fitness score and the transformation probability with 17 significant digits, and the pipeline's counters before and after the
// route's registration work of that frame.  Exit code 3 without a GPU.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <random>
#include <string>
#include <vector>

#include <pcl/point_types.h>
#include <pclomp/ndt_omp.h>
#include <radar_preprocessing/scan_preprocessor.hpp>

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Ndt = pclomp::NormalDistributionsTransform<PointT, PointT>;
using Pre = gorio::ScanPreprocessor<PointT>;

struct Counters {
  long long uploads = 0, builds = 0, downloads = 0;
};

static Counters counters(Pre& pre) {
  Counters c;
  gorio_scan_get_counters(pre.handle(), &c.uploads, &c.builds, &c.downloads);
  return c;
}

static void configure(Ndt& r, double resolution) {  // registrations.cpp:117-134
  r.setTransformationEpsilon(0.01);
  r.setMaximumIterations(64);
  r.setResolution((float)resolution);
  r.setNeighborhoodSearchMethod(pclomp::DIRECT7);
}

struct Match {
  int aligned = 0, converged = 0, iterations = 0;
  float T[16] = {0};
  double probability = 0.0, fitness = 0.0;
};

static Match match(Ndt& r) {
  Match m;
  Cloud out;
  r.align(out);
  m.aligned = 1;
  m.converged = r.hasConverged();
  m.iterations = r.getFinalNumIteration();
  m.probability = r.getTransformationProbability();
  const Eigen::Matrix4f T = r.getFinalTransformation();
  for (int q = 0; q < 4; ++q)
    for (int c = 0; c < 4; ++c) m.T[4 * q + c] = T(q, c);
  m.fitness = r.getFitnessScore();
  return m;
}

static void print_line(const char* route, int frame, int submap, int status, int n, const Match& m, const Counters& before, const Counters& after) {
  std::printf("{\"route\": \"%s\", \"frame\": %d, \"submap\": %d, \"status\": %d, \"n\": %d, \"aligned\": %d, \"converged\": %d, \"iterations\": %d, \"probability\": %.17g, \"fitness\": %.17g, ",
              route, frame, submap, status, n, m.aligned, m.converged, m.iterations, m.probability, m.fitness);
  std::printf("\"T_bits\": [");
  for (int q = 0; q < 16; ++q) {
    std::uint32_t u;
    std::memcpy(&u, &m.T[q], 4);
    std::printf("%u%s", u, q == 15 ? "" : ", ");
  }
  std::printf("], \"before\": [%lld, %lld, %lld], \"after\": [%lld, %lld, %lld]}\n", before.uploads, before.builds, before.downloads, after.uploads, after.builds, after.downloads);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s scans.bin resolution submap_voxel_leaf\n", argv[0]);
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
  const double resolution = std::atof(argv[2]), leaf = std::atof(argv[3]);
  const double* ang_vel = have_w ? w : nullptr;
  try {
    Ndt regA, regB;  // first: without a HIP device this is where the run ends
    configure(regA, resolution);
    configure(regB, resolution);
    gorio_scan_params P = Pre::defaults();
    std::memcpy(P.rotation, R, sizeof(R));
    P.enable_dynamic_object_removal = dor;
    P.outlier_method = method;
    Pre pre(P);
    std::mt19937 rng(seed);
    std::vector<Cloud::ConstPtr> keyframes;
    bool have_target = false;
    for (int s = 0; s < F; ++s) {
      const int n = (int)(msgs[s].size() / 5);
      const auto r = pre.process_packed(msgs[s].data(), n, ang_vel, rng);
      Match a, b;
      const Counters c0 = counters(pre);
      Counters c1 = c0, c2 = c0;
      int n_out = 0;
      if (r.status == GORIO_SCAN_OK) {
        n_out = (int)r.full_scan->size();
        // ---- route A: the frame never leaves the device
        if (have_target) {
          regA.setInputSourceFromScan(pre);
          a = match(regA);
        }
        regA.setInputTargetFromScan(pre);  // this frame is the next keyframe
        c1 = counters(pre);
        // ---- route B: the host cloud process() returned, uploaded again
        if (have_target) {
          regB.setInputSource(pre.last_scan());
          b = match(regB);
        }
        regB.setInputTarget(pre.last_scan());
        c2 = counters(pre);
        have_target = true;
        keyframes.push_back(pre.last_scan());
      }
      print_line("A", s, 0, r.status, n_out, a, c0, c1);
      print_line("B", s, 0, r.status, n_out, b, c1, c2);
    }
    // ---- scan-to-submap: the last frame that was matched against the last (up to) three keyframes, each moved by a relative pose
    if (keyframes.size() >= 2) {
      const std::size_t k = std::min<std::size_t>(3, keyframes.size());
      std::vector<Cloud::ConstPtr> clouds(keyframes.end() - k, keyframes.end());
      std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> poses(k);
      for (std::size_t q = 0; q < k; ++q) {
        poses[q].setIdentity();
        poses[q](0, 3) = 0.15 * (double)(k - 1 - q);  // odom_q^-1 * odom_newest: the newest keyframe sits at the identity
        poses[q](1, 3) = -0.05 * (double)(k - 1 - q);
      }
      const Counters c0 = counters(pre);  // both objects still hold the last frame as their source
      const Cloud::ConstPtr assembled = regA.setInputTargetSubmap(clouds, poses, leaf);
      const Match a = match(regA);
      const Counters c1 = counters(pre);
      regB.setInputTarget(assembled);
      const Match b = match(regB);
      const Counters c2 = counters(pre);
      print_line("A", F, 1, GORIO_SCAN_OK, (int)assembled->size(), a, c0, c1);
      print_line("B", F, 1, GORIO_SCAN_OK, (int)assembled->size(), b, c1, c2);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ndt_scan_sequence: %s\n", e.what());
    return 3;
  }
  return 0;
}
