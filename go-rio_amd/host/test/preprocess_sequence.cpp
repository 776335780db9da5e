// Replays the preprocessing nodelet's cloud_callback (apps/preprocessing_nodelet_ntu.cpp:370-581, "PREP") over a sequence of raw radar
// messages twice: (A) through gorio::ScanPreprocessor -- the device-resident pipeline of include/gorio_scan.h -- and (B) through the
// single calls of include/gorio_prep.h / gorio_ground.h with the stages that have no call of their own (gate and rotation, deskew,
// distance filter) and every compaction done on the host, as a caller had to write it before the pipeline existed.  Both draw their
// RANSAC samples from std::mt19937 engines with one seed, both carry one Patchwork++ state over the sequence.  From the second frame on
// each frame is also registered against the one before it: (A) FastAPDGICP::setInputSourceFromScan / setInputTargetFromScan, (B)
// setInputSource / setInputTarget with the host cloud.
//
// Input (binary): [int32 F][double R[9]][int32 dynamic_object_removal][int32 outlier_method][int32 have_ang_vel][double ang_vel[3]]
//                 [uint32 seed], then per message [int32 n][n x (x, y, z, power, doppler) float].
// Output (binary, argv[2]): per message, for A then for B: [int32 status][int32 n_out][int32 n_ground][int32 n_clusters][double v_r[3]]
//                 [double sigma_v_r[3]][n_out x (x, y, z, intensity, doppler, label) float][int32 aligned][float T[16]][int32 converged]
//                 (T and converged are zeros when aligned is 0).
// `preprocess_sequence scans.bin --time REPS` instead times both sequences per frame (interleaved, after 5 warm-up rounds over the
// sequence) and prints medians with the 10th / 90th percentile in microseconds, split by stage.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <random>
#include <string>
#include <vector>

#include <pcl/point_types.h>
#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <radar_preprocessing/scan_preprocessor.hpp>

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;
using Clock = std::chrono::steady_clock;

struct Frame {
  int status = GORIO_SCAN_EMPTY, n_ground = 0, n_clusters = 0;
  double v_r[3] = {0, 0, 0}, sigma[3] = {0, 0, 0};
  Cloud::Ptr cloud;
};

struct StageTimes {  // microseconds per named stage, in first-use order
  std::vector<std::string> names;
  std::map<std::string, std::vector<double>> us;
  bool on = false;
  void add(const std::string& k, Clock::time_point t0) {
    if (!on) return;
    if (!us.count(k)) names.push_back(k);
    us[k].push_back(std::chrono::duration<double, std::micro>(Clock::now() - t0).count());
  }
};

static std::vector<PointT> compact(const std::vector<PointT>& in, const std::vector<unsigned char>& keep) {
  std::vector<PointT> out;
  for (std::size_t i = 0; i < in.size(); ++i)
    if (keep[i]) out.push_back(in[i]);
  return out;
}

// (B): the callback through the single calls.  `ground` carries the Patchwork++ state.
static Frame single_calls(const float* raw5, int n, const gorio_scan_params& P, const double* ang_vel, std::mt19937& rng, gorio_ground_t* ground, StageTimes& tm) {
  Frame f;
  auto t0 = Clock::now();
  // PREP:381-412: power gate, finite test, rotation in double summed left to right and rounded once
  std::vector<PointT> pts;
  for (int i = 0; i < n; ++i) {
    const float* r = raw5 + 5 * (std::size_t)i;
    if (!(r[3] > P.power_threshold) || !std::isfinite(r[0]) || !std::isfinite(r[1]) || !std::isfinite(r[2])) continue;
    const double x = r[0], y = r[1], z = r[2];
    PointT p;
    p.x = (float)((P.rotation[0] * x + P.rotation[1] * y) + P.rotation[2] * z);
    p.y = (float)((P.rotation[3] * x + P.rotation[4] * y) + P.rotation[5] * z);
    p.z = (float)((P.rotation[6] * x + P.rotation[7] * y) + P.rotation[8] * z);
    p.intensity = r[3];
    p.curvature = r[4];
    pts.push_back(p);
  }
  tm.add("B gate + rotate (host)", t0);
  if (pts.empty()) return f;
  // PREP:421-449
  t0 = Clock::now();
  int nv = 0, zero = 0, ok = 0;
  const int st = (int)sizeof(PointT);
  if (gorio_prep_ego_velocity(0, &pts[0].x, &pts[0].intensity, &pts[0].curvature, (int)pts.size(), st, &P.reve, nullptr, 0, f.v_r, f.sigma, nullptr, nullptr, &nv, &zero, &ok) < 0)
    throw std::runtime_error(gorio_prep_last_error());
  const std::vector<unsigned int> samples = gorio::draw_ransac_samples(P.reve, nv, rng);
  std::vector<unsigned char> inlier(pts.size(), 0);
  if (gorio_prep_ego_velocity(0, &pts[0].x, &pts[0].intensity, &pts[0].curvature, (int)pts.size(), st, &P.reve, samples.empty() ? nullptr : samples.data(),
                              (int)samples.size() / P.reve.n_ransac_points, f.v_r, f.sigma, inlier.data(), nullptr, &nv, &zero, &ok) < 0)
    throw std::runtime_error(gorio_prep_last_error());
  tm.add("B gorio_prep_ego_velocity (x2: count, solve)", t0);
  if (ok) {
    if (std::sqrt(f.v_r[0] * f.v_r[0] + f.v_r[1] * f.v_r[1] + f.v_r[2] * f.v_r[2]) < 0.05) {
      f.status = GORIO_SCAN_ZERO_VELOCITY;
      return f;
    }
  } else {
    for (int q = 0; q < 3; ++q) f.v_r[q] = f.sigma[q] = 0.0;
    std::fill(inlier.begin(), inlier.end(), 0);
  }
  t0 = Clock::now();
  if (P.enable_dynamic_object_removal) pts = compact(pts, inlier);  // PREP:464-478
  if (pts.empty()) return f;
  if (P.deskew && ang_vel) {  // PREP:705-716, the operation order of Eigen's Quaternionf as csrc/apd_scan.hip states it
    const float wx = -(float)ang_vel[0], wy = -(float)ang_vel[1], wz = -(float)ang_vel[2];
    const int size = (int)pts.size();
    for (int i = 0; i < size; ++i) {
      const double half = (P.scan_period * (double)i / (double)size) / 2.0;
      const float qx = (float)(half * (double)wx), qy = (float)(half * (double)wy), qz = (float)(half * (double)wz), qw = 1.0f;
      const float n2 = ((qx * qx + qy * qy) + qz * qz) + qw * qw;
      const float ix = -qx / n2, iy = -qy / n2, iz = -qz / n2, iw = qw / n2;
      const float vx = pts[i].x, vy = pts[i].y, vz = pts[i].z;
      float ux = iy * vz - iz * vy, uy = iz * vx - ix * vz, uz = ix * vy - iy * vx;
      ux = ux + ux;
      uy = uy + uy;
      uz = uz + uz;
      const float cx = iy * uz - iz * uy, cy = iz * ux - ix * uz, cz = ix * uy - iy * ux;
      pts[i].x = (vx + iw * ux) + cx;
      pts[i].y = (vy + iw * uy) + cy;
      pts[i].z = (vz + iw * uz) + cz;
    }
  }
  {  // PREP:643-647
    std::vector<unsigned char> keep(pts.size());
    for (std::size_t i = 0; i < pts.size(); ++i) {
      const float x = pts[i].x, y = pts[i].y, z = pts[i].z;
      const double d = (double)std::sqrt((x * x + y * y) + z * z), zd = (double)z;
      keep[i] = d > P.distance_near && d < P.distance_far && zd < P.z_high && zd > P.z_low;
    }
    pts = compact(pts, keep);
  }
  tm.add("B removal, deskew, distance filter (host)", t0);
  if (pts.empty()) return f;
  if (P.outlier_method != GORIO_SCAN_OUTLIER_NONE) {  // PREP:503
    t0 = Clock::now();
    std::vector<unsigned char> keep(pts.size());
    int kept = 0;
    const int rc = P.outlier_method == GORIO_SCAN_OUTLIER_STATISTICAL
                       ? gorio_prep_statistical_outlier_mask(0, &pts[0].x, (int)pts.size(), st, P.mean_k, P.stddev_mul, keep.data(), &kept, nullptr)
                       : gorio_prep_radius_outlier_mask(0, &pts[0].x, (int)pts.size(), st, P.radius, P.min_neighbors, keep.data(), &kept);
    if (rc < 0) {
      f.status = GORIO_SCAN_REFUSED;
      return f;
    }
    pts = compact(pts, keep);
    tm.add("B outlier mask + host compaction", t0);
    if (pts.empty()) return f;
  }
  if (P.ground) {  // PREP:505-518
    t0 = Clock::now();
    std::vector<int> order(pts.size());
    int ng = 0, no = 0;
    if (gorio_ground_estimate(ground, &pts[0].x, &pts[0].intensity, (int)pts.size(), st, 1, order.data(), &ng, &no) < 0) throw std::runtime_error(gorio_ground_last_error());
    std::vector<PointT> full(no);
    for (int j = 0; j < no; ++j) full[j] = pts[order[j]];
    pts.swap(full);
    f.n_ground = ng;
    tm.add("B gorio_ground_estimate + host gather", t0);
    if (pts.empty()) return f;
  }
  t0 = Clock::now();
  if (gorio_prep_dbscan_labels(0, &pts[0].x, (int)pts.size(), st, P.dbscan_eps, P.dbscan_core_min_pts, P.dbscan_min_cluster_size, P.dbscan_max_cluster_size, &pts[0].normal_x, st,
                               &f.n_clusters) < 0)
    throw std::runtime_error(gorio_prep_last_error());
  tm.add("B gorio_prep_dbscan_labels", t0);
  f.cloud.reset(new Cloud());
  f.cloud->points.swap(pts);
  f.status = GORIO_SCAN_OK;
  return f;
}

static void configure(Reg& r) {  // scan_matching_odometry_nodelet.cpp with the launch files' values
  r.setMaxCorrespondenceDistance(2.0);
  r.setTransformationEpsilon(0.1);
  r.setMaximumIterations(32);
}

struct Aligned {
  int done = 0, converged = 0;
  float T[16] = {0};
};

static void write_frame(std::FILE* o, const Frame& f, const Aligned& a) {
  const int n_out = f.cloud ? (int)f.cloud->size() : 0;
  const int head[4] = {f.status, n_out, f.n_ground, f.n_clusters};
  std::fwrite(head, 4, 4, o);
  std::fwrite(f.v_r, 8, 3, o);
  std::fwrite(f.sigma, 8, 3, o);
  for (int i = 0; i < n_out; ++i) {
    const PointT& p = f.cloud->points[i];
    const float r[6] = {p.x, p.y, p.z, p.intensity, p.curvature, p.normal_x};
    std::fwrite(r, 4, 6, o);
  }
  std::fwrite(&a.done, 4, 1, o);
  std::fwrite(a.T, 4, 16, o);
  std::fwrite(&a.converged, 4, 1, o);
}

static Aligned align(Reg& r) {
  Aligned a;
  Cloud out;
  r.align(out);
  a.done = 1;
  a.converged = r.hasConverged();
  const auto T = r.getFinalTransformation();
  for (int q = 0; q < 4; ++q)
    for (int c = 0; c < 4; ++c) a.T[q * 4 + c] = T(q, c);
  return a;
}

static void report(const StageTimes& tm) {
  for (const std::string& k : tm.names) {
    std::vector<double> v = tm.us.at(k);
    std::sort(v.begin(), v.end());
    const std::size_t m = v.size();
    std::printf("%-48s median %9.1f us   p10 %9.1f   p90 %9.1f   (%zu samples)\n", k.c_str(), v[m / 2], v[m / 10], v[(9 * m) / 10], m);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s scans.bin out.bin | %s scans.bin --time REPS\n", argv[0], argv[0]);
    return 2;
  }
  const bool timing = std::strcmp(argv[2], "--time") == 0;
  const int reps = timing ? (argc > 3 ? std::atoi(argv[3]) : 30) : 1;
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
  const double* ang_vel = have_w ? w : nullptr;
  try {
    gorio_scan_params P = gorio::ScanPreprocessor<PointT>::defaults();
    std::memcpy(P.rotation, R, sizeof(R));
    P.enable_dynamic_object_removal = dor;
    P.outlier_method = method;
    Reg regA, regB;  // first: without a HIP device this is where the run ends
    gorio::ScanPreprocessor<PointT> pre(P);
    gorio_ground_t* ground = nullptr;
    if (gorio_ground_create(&ground, 0, &P.ground_params) != 0) throw std::runtime_error(std::string("gorio_ground_create: ") + gorio_ground_last_error());
    configure(regA);
    configure(regB);
    std::mt19937 rngA(seed), rngB(seed);
    StageTimes tm;
    if (!timing) {
      std::FILE* o = std::fopen(argv[2], "wb");
      if (!o) return 2;
      bool have_target = false;
      for (int s = 0; s < F; ++s) {
        const int n = (int)(msgs[s].size() / 5);
        Frame a;
        const auto r = pre.process_packed(msgs[s].data(), n, ang_vel, rngA);
        a.status = r.status;
        a.n_ground = r.n_ground;
        a.n_clusters = r.n_clusters;
        std::memcpy(a.v_r, r.v_r, sizeof(a.v_r));
        std::memcpy(a.sigma, r.sigma_v_r, sizeof(a.sigma));
        a.cloud = r.full_scan;
        Frame b = single_calls(msgs[s].data(), n, P, ang_vel, rngB, ground, tm);
        Aligned ra, rb;
        if (a.status == GORIO_SCAN_OK && b.status == GORIO_SCAN_OK) {
          if (have_target) {
            regA.setInputSourceFromScan(pre);
            regB.setInputSource(b.cloud);
            ra = align(regA);
            rb = align(regB);
          }
          regA.setInputTargetFromScan(pre);
          regB.setInputTarget(b.cloud);
          have_target = true;
        }
        write_frame(o, a, ra);
        write_frame(o, b, rb);
        std::fprintf(stderr, "message %d: A status %d, %d points; B status %d, %d points\n", s, a.status, a.cloud ? (int)a.cloud->size() : 0, b.status, b.cloud ? (int)b.cloud->size() : 0);
      }
      std::fclose(o);
    } else {
      // one frame = the preprocessing and the hand-off to a registration object as its source.  gorio_apd_set_source only uploads: it
      // leaves the search index of the cloud to the first align, while the cloud (A) hands over carries the index DBSCAN built.
      const int warm = 5;
      for (int rep = 0; rep < warm + reps; ++rep) {
        tm.on = rep >= warm;
        for (int s = 0; s < F; ++s) {
          const int n = (int)(msgs[s].size() / 5);
          const float* m = msgs[s].data();
          // ---- A, through the C ABI the class wraps (the class would also download the cloud for publishing)
          auto tA = Clock::now(), t0 = tA;
          int ng = 0, nv = 0;
          gorio_scan_result r;
          if (gorio_scan_load(pre.handle(), m, m + 3, m + 4, n, 20, &ng, &nv) < 0) throw std::runtime_error(gorio_scan_last_error());
          tm.add("A gorio_scan_load", t0);
          t0 = Clock::now();
          const std::vector<unsigned int> smp = gorio::draw_ransac_samples(P.reve, nv, rngA);
          if (gorio_scan_run(pre.handle(), smp.empty() ? nullptr : smp.data(), (int)smp.size() / P.reve.n_ransac_points, ang_vel, &r) < 0) throw std::runtime_error(gorio_scan_last_error());
          tm.add("A gorio_scan_run", t0);
          if (r.status != GORIO_SCAN_OK) throw std::runtime_error("timing: a message produced no frame");
          t0 = Clock::now();
          if (gorio_apd_set_source_from_scan(regA.handle(), pre.handle()) < 0) throw std::runtime_error(gorio_apd_last_error(regA.handle()));
          tm.add("A gorio_apd_set_source_from_scan", t0);
          tm.add("A TOTAL load + run + hand-off", tA);
          // ---- B
          auto tB = Clock::now();
          Frame b = single_calls(m, n, P, ang_vel, rngB, ground, tm);
          if (b.status != GORIO_SCAN_OK) throw std::runtime_error("timing: a message produced no frame (single calls)");
          t0 = Clock::now();
          if (gorio_apd_set_source(regB.handle(), &b.cloud->points[0].x, &b.cloud->points[0].normal_x, (int)b.cloud->size(), (int)sizeof(PointT)) < 0)
            throw std::runtime_error(gorio_apd_last_error(regB.handle()));
          tm.add("B gorio_apd_set_source", t0);
          tm.add("B TOTAL single calls + set_source", tB);
        }
      }
      report(tm);
      long long up = 0, ib = 0, dl = 0;
      gorio_scan_get_counters(pre.handle(), &up, &ib, &dl);
      std::printf("A counters over %d frames: point_uploads %lld, index_builds %lld, point_downloads %lld\n", (warm + reps) * F, up, ib, dl);
    }
    gorio_ground_destroy(ground);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "preprocess_sequence: %s\n", e.what());
    return 3;
  }
  return 0;
}
