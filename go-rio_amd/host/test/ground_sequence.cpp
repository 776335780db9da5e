// Replays the ground segmentation step of the preprocessing nodelet (apps/preprocessing_nodelet_ntu.cpp:502-519) over a sequence of
// scans with the drop-in PatchWorkpp<PointXYZINormal>: estimate_ground(..., id) per scan, then full_scan = ground + nonground.
// Input: binary [int32 F] then per scan [int32 n][n x (x, y, z, intensity) float].
// Output (binary, to argv[2]): per scan [int32 n_ground][int32 n_full][n_full x (x, y, z, intensity) float].  argv[3]: id (default 1).
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>

#include <pcl/point_types.h>
#include <patchworkpp/patchworkpp.hpp>

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s scans.bin out.bin [id]\n", argv[0]);
    return 2;
  }
  const int id = argc > 3 ? std::atoi(argv[3]) : 1;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int F = 0;
  if (std::fread(&F, 4, 1, f) != 1 || F < 0) return 2;
  try {
    Params params;  // the nodelet: Params() with verbose off (PREP:100-102)
    PatchWorkpp<pcl::PointXYZINormal> pw(params);
    std::FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int s = 0; s < F; ++s) {
      int n = 0;
      if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
      pcl::PointCloud<pcl::PointXYZINormal> cloud;
      cloud.points.resize(n);
      for (int i = 0; i < n; ++i) {
        float r[4];
        if (std::fread(r, 4, 4, f) != 4) return 2;
        cloud.points[i].x = r[0];
        cloud.points[i].y = r[1];
        cloud.points[i].z = r[2];
        cloud.points[i].intensity = r[3];
      }
      pcl::PointCloud<pcl::PointXYZINormal> ground, nonground, full_scan;
      double ground_time = 0;
      pw.estimate_ground(cloud, Eigen::Vector3d(), ground, nonground, ground_time, id);  // PREP:511
      full_scan.points = ground.points;                                                  // PREP:519
      full_scan.points.insert(full_scan.points.end(), nonground.points.begin(), nonground.points.end());
      const int ng = (int)ground.points.size(), nf = (int)full_scan.points.size();
      std::fwrite(&ng, 4, 1, o);
      std::fwrite(&nf, 4, 1, o);
      for (const auto& p : full_scan.points) {
        const float r[4] = {p.x, p.y, p.z, p.intensity};
        std::fwrite(r, 4, 4, o);
      }
      std::fprintf(stderr, "scan %d: %d ground, %d non-ground, %.3f ms\n", s, ng, nf - ng, ground_time * 1e3);
    }
    std::fclose(o);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "ground_sequence: %s\n", e.what());
    return 3;
  }
  std::fclose(f);
  return 0;
}
