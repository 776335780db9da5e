// The front end's keyframe handling (scan_matching_odometry_nodelet.cpp:423-618, "SMO") and loop-closure verification
// (loop_detector.cpp:222-236, 391-422, "LD") over a short sequence, through the drop-in classes, twice:
//   host:  the reference pattern -- every keyframe is a pcl cloud; setInputTarget(keyframe) for the next scan-to-scan target,
//          setInputTargetSubmap(clouds, ...) for the scan-to-submap target, setInputSource / setInputTarget(cloud) per loop candidate,
//          makeAndSaveScancontextAndKeys(cloud);
//   store: the same steps with the keyframes resident in a gorio::KeyframeStore -- addFromSource after the align that made the
//          keyframe, setInputTargetKeyframe, setInputTargetSubmap(store, ids, ...), setInput*Keyframe per loop candidate,
//          makeAndSaveScancontextAndKeys(store, id).
// Per frame: align against the scan-to-scan target (guess = the previous result, SMO:430-479), align against the submap, the keyframe
// decision (SMO:560-584 with thresholds given on the command line), and for a new keyframe the new targets (SMO:586-618, at most ten
// keyframes in the submap).  Then the newest keyframe against every earlier one (LD).
// Input: binary [int32 n_frames] then per frame [int32 n][n x (x, y, z, label) float32]; intensity is 5 + label.
// Output: one JSON line per step and mode; the two modes must print the same values.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include <fast_gicp/gicp/fast_apdgicp.hpp>
#include <radar_graph_slam/keyframe_store.hpp>
#include <scan_context/Scancontext.h>

using PointT = pcl::PointXYZINormal;
using Cloud = pcl::PointCloud<PointT>;
using Reg = fast_gicp::FastAPDGICP<PointT, PointT>;
using Store = gorio::KeyframeStore<PointT>;
using PoseVector = std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>;

static void configure(Reg& r) {  // registrations.cpp:38-51 with launch/ntu_loop3.launch:85-96
  r.setNumThreads(0);
  r.setTransformationEpsilon(0.1);
  r.setMaximumIterations(64);
  r.setMaxCorrespondenceDistance(2.0);
  r.setCorrespondenceRandomness(20);
  r.setDistVar(0.86);
  r.setAzimuthVar(0.5);
  r.setElevationVar(1.0);
}

static Cloud::Ptr read_cloud(std::FILE* f) {
  int n = 0;
  if (std::fread(&n, 4, 1, f) != 1 || n < 0) return nullptr;
  std::vector<float> buf((size_t)n * 4);
  if (std::fread(buf.data(), 4, buf.size(), f) != buf.size()) return nullptr;
  Cloud::Ptr c(new Cloud());
  c->resize(n);
  for (int i = 0; i < n; ++i) {
    PointT& p = c->points[i];
    p.x = buf[4 * i];
    p.y = buf[4 * i + 1];
    p.z = buf[4 * i + 2];
    p.data[3] = 1.0f;
    p.normal_x = buf[4 * i + 3];
    p.intensity = 5.0f + buf[4 * i + 3];
  }
  return c;
}

// rigid 4 x 4 helpers on Eigen::Matrix4d, element by element (the driver also builds against the minimal Eigen stand-in)
static Eigen::Matrix4d mul(const Eigen::Matrix4d& a, const Eigen::Matrix4d& b) {
  Eigen::Matrix4d o;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += a(r, k) * b(k, c);
      o(r, c) = s;
    }
  return o;
}
static Eigen::Matrix4d rigid_inverse(const Eigen::Matrix4d& a) {
  Eigen::Matrix4d o = Eigen::Matrix4d::Identity();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) o(r, c) = a(c, r);
  }
  for (int r = 0; r < 3; ++r) o(r, 3) = -(o(r, 0) * a(0, 3) + o(r, 1) * a(1, 3) + o(r, 2) * a(2, 3));
  return o;
}
static Eigen::Matrix4d widen(const Eigen::Matrix4f& a) {
  Eigen::Matrix4d o;
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) o(r, c) = (double)a(r, c);
  return o;
}

struct Probe : Reg {  // nr_iterations_ is protected in pcl::Registration
  static int iterations(const Reg& r) { return r.*(&Probe::nr_iterations_); }
};

static void print_align(const char* mode, const char* step, int i, int j, Reg& r, double fitness, int n_target) {
  const Eigen::Matrix4f T = r.getFinalTransformation();
  std::printf("{\"mode\": \"%s\", \"step\": \"%s\", \"i\": %d, \"j\": %d, \"converged\": %d, \"nr_iterations\": %d, \"fitness\": %.17g, \"n_target\": %d, \"T\": [", mode, step, i, j,
              r.hasConverged() ? 1 : 0, Probe::iterations(r), fitness, n_target);
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 4; ++b) std::printf("%.9g%s", T(a, b), (a == 3 && b == 3) ? "" : ", ");
  std::printf("]}\n");
}

// one pass over the sequence; store == nullptr: the host pattern
static void run(const char* mode, const std::vector<Cloud::Ptr>& frames, double delta_trans, double delta_angle, double leaf, Store* store) {
  Reg s2s, s2m, loop;
  configure(s2s);
  configure(s2m);
  configure(loop);
  SCManager sc;
  std::vector<int> kf_frame, kf_id;  // keyframes: the frame each one is, and its id in the store
  PoseVector kf_odom;
  Eigen::Matrix4f prev = Eigen::Matrix4f::Identity();
  Eigen::Matrix4d keyframe_pose = Eigen::Matrix4d::Identity();
  bool have_submap = false;
  int n_submap = 0;

  auto new_keyframe = [&](int k, const Eigen::Matrix4d& odom, bool from_source) {
    // SMO:586-588: keyframe_cloud = filtered; registration->setInputTarget(keyframe_cloud)
    int id = -1;
    if (store) {
      id = from_source ? store->addFromSource(s2s) : store->add(frames[k]);  // the source of the align that made it: covariances and index are there
      s2s.setInputTargetKeyframe(*store, id);
    } else {
      s2s.setInputTarget(frames[k]);
    }
    kf_frame.push_back(k);
    kf_id.push_back(id);
    kf_odom.push_back(odom);
    // RGS:727-731
    if (store) sc.makeAndSaveScancontextAndKeys(*store, id);
    else {
      Cloud copy = *frames[k];
      sc.makeAndSaveScancontextAndKeys(copy);
    }
    double ring_sum = 0.0;
    for (int q = 0; q < sc.polarcontext_invkeys_.back().rows(); ++q) ring_sum += sc.polarcontext_invkeys_.back()(q, 0);
    std::printf("{\"mode\": \"%s\", \"step\": \"scan_context\", \"i\": %d, \"ring_key_sum\": %.17g}\n", mode, k, ring_sum);
    // SMO:602-618: the last (at most ten) keyframes moved into the newest one's frame
    const std::size_t first = kf_frame.size() > 10 ? kf_frame.size() - 10 : 0;
    PoseVector rel;
    std::vector<Cloud::ConstPtr> clouds;
    std::vector<int> ids;
    for (std::size_t q = first; q < kf_frame.size(); ++q) {
      rel.push_back(mul(rigid_inverse(odom), kf_odom[q]));
      clouds.push_back(frames[kf_frame[q]]);
      ids.push_back(kf_id[q]);
    }
    Cloud::ConstPtr sub = store ? s2m.setInputTargetSubmap(*store, ids, rel, leaf) : s2m.setInputTargetSubmap(clouds, rel, leaf);
    n_submap = (int)sub->size();
    have_submap = true;
    const PointT& p = sub->points[n_submap / 2];
    std::printf("{\"mode\": \"%s\", \"step\": \"submap\", \"i\": %d, \"n_target\": %d, \"mid\": [%.9g, %.9g, %.9g, %.9g]}\n", mode, k, n_submap, p.x, p.y, p.z, p.normal_x);
  };

  new_keyframe(0, Eigen::Matrix4d::Identity(), false);
  for (int k = 1; k < (int)frames.size(); ++k) {
    s2s.setInputSource(frames[k]);  // SMO:430-479
    Cloud aligned;
    s2s.align(aligned, prev);
    print_align(mode, "scan_to_scan", k, kf_frame.back(), s2s, s2s.getFitnessScore(), (int)s2s.getInputTarget()->size());
    if (!s2s.hasConverged()) continue;
    const Eigen::Matrix4f T = s2s.getFinalTransformation();
    if (have_submap) {
      s2m.setInputSource(frames[k]);
      Cloud moved;
      s2m.align(moved, T);
      print_align(mode, "scan_to_submap", k, kf_frame.back(), s2m, s2m.getFitnessScore(), n_submap);
    }
    prev = T;
    const Eigen::Matrix4d odom = mul(keyframe_pose, widen(T));
    // SMO:560-584
    const double dx = std::sqrt((double)T(0, 3) * T(0, 3) + (double)T(1, 3) * T(1, 3) + (double)T(2, 3) * T(2, 3));
    const double da = std::acos(std::min(1.0, std::max(-1.0, ((double)T(0, 0) + T(1, 1) + T(2, 2) - 1.0) / 2.0)));
    if (dx > delta_trans || da > delta_angle) {
      new_keyframe(k, odom, true);
      keyframe_pose = odom;
      prev = Eigen::Matrix4f::Identity();
    }
  }

  // LD:391-422: the newest keyframe is the target, every earlier keyframe a candidate source (LD:222 is the mirror image, checked on
  // the first candidate)
  const int newest = (int)kf_frame.size() - 1;
  for (int pass = 0; pass < 2 && newest > 0; ++pass) {
    for (int q = 0; q < (pass == 0 ? newest : 1); ++q) {
      const int tgt = pass == 0 ? newest : q, src = pass == 0 ? q : newest;
      if (store) {
        loop.setInputTargetKeyframe(*store, kf_id[tgt]);
        loop.setInputSourceKeyframe(*store, kf_id[src]);
      } else {
        loop.setInputTarget(frames[kf_frame[tgt]]);
        loop.setInputSource(frames[kf_frame[src]]);
      }
      const Eigen::Matrix4d g = mul(rigid_inverse(kf_odom[tgt]), kf_odom[src]);
      Eigen::Matrix4f guess;
      for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) guess(r, c) = (float)g(r, c);
      Cloud aligned;
      loop.align(aligned, guess);
      print_align(mode, pass == 0 ? "loop_target_newest" : "loop_source_newest", kf_frame[src], kf_frame[tgt], loop, loop.getFitnessScore(), (int)loop.getInputTarget()->size());
    }
  }
  if (store) {
    const gorio_kf_info_t info = store->info(kf_id[newest]);
    std::printf("{\"mode\": \"store_info\", \"keyframes\": %d, \"n\": %d, \"cov_count\": %d, \"index_built\": %d}\n", (int)store->size(), info.n, info.cov_count, info.index_built);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s frames.bin [keyframe_delta_trans [keyframe_delta_angle [voxel_leaf]]]\n", argv[0]);
    return 2;
  }
  const double delta_trans = argc > 2 ? std::atof(argv[2]) : 0.25, delta_angle = argc > 3 ? std::atof(argv[3]) : 0.15, leaf = argc > 4 ? std::atof(argv[4]) : 0.1;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int n_frames = 0;
  if (std::fread(&n_frames, 4, 1, f) != 1 || n_frames <= 0) return 2;
  std::vector<Cloud::Ptr> frames;
  for (int k = 0; k < n_frames; ++k) {
    Cloud::Ptr c = read_cloud(f);
    if (!c) return 2;
    frames.push_back(c);
  }
  std::fclose(f);
  try {
    run("host", frames, delta_trans, delta_angle, leaf, nullptr);
    Store store;
    run("store", frames, delta_trans, delta_angle, leaf, &store);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;  // no GPU: the drop-ins refuse instead of falling back to a CPU path
  }
  return 0;
}
