/*
 * gorio_map.h -- C ABI of the map cloud on the MI355X (libgorio_amd.so): MapCloudGenerator::generate of the back end, fed from the
 * keyframe store (include/gorio_keyframes.h) by id.  The keyframes never leave the device; only the finished map crosses to the host.
 *
 * Paths relative to the Go-RIO sources (4DRadarSLAM):
 *   MCG = src/radar_graph_slam/map_cloud_generator.cpp    RGS = apps/radar_graph_slam_nodelet.cpp
 *
 * RGS calls generate from the map-publish timer over ALL keyframes (RGS:858-878; every shipped launch file: every 6 s at
 * map_cloud_resolution = 0.05) and again from save_map_service (RGS:1184).
 *
 * Same conventions as include/gorio_keyframes.h: plain pointers, host pointers caller-owned and only read / written during the call, 0 on
 * success or a negative gorio_status (include/gorio_apd.h), gorio_map_last_error gives the text (thread-local).  No CPU fallback:
 * gorio_map_create only checks and stores its arguments; the first call that needs the device fails with GORIO_ERR_NO_DEVICE without a
 * HIP device.  Argument and state errors are reported before any device call, and a failed call changes nothing: the cloud of the last
 * successful generate stays retrievable.  (One exception: when growing the result buffer itself fails, GORIO_ERR_NO_DEVICE, the handle
 * is left with an empty result.)  One handle must not be used from two threads at once, nor at the same time as its store.
 *
 * WHAT generate COMPUTES
 *
 * Stage A (MCG:22-32).  Keyframes in the order listed, points in their stored order.
 *   gate       s = (x*x + y*y) + z*z in float, un-fused, left to right; d = the correctly rounded float square root of s (computed in
 *              double, rounded once); the point is dropped iff (double)d > 50.0.  So a point with a NaN coordinate is KEPT (the
 *              reference's `d > 50` is false for NaN), one with an infinite coordinate is dropped, (30, 40, 0) is kept.
 *   transform  M = the pose cast to float entry by entry (pose.matrix().cast<float>()); q_r = ((M_r0*x + M_r1*y) + M_r2*z) + M_r3 in
 *              float, un-fused -- the convention include/gorio_ndt.h states for pcl::transformPointCloud with a float matrix.  The fourth
 *              component of a stored point is taken as 1.  This is NOT the double transform of gorio_apd_set_target_submap_keyframes.
 *   intensity  carried over; a keyframe without an intensity column contributes 0.
 * With resolution <= 0 the result is stage A's output in that order (MCG:38-39).  A kept NaN point transforms to NaN coordinates whose
 * payload is not specified.
 *
 * Stage B (MCG:41-50) for resolution > 0: pcl::octree::OctreePointCloud::addPointsFromInputCloud + getOccupiedVoxelCenters.
 *   Only finite q take part (PCL skips the others).  The lattice is anchored at the first finite kept point q0 in stage-A order.  Per
 *   axis, in double, un-fused:
 *       a = (double)q0 - resolution / 2        k = floor(((double)q - a) / resolution)        centre = (float)(((double)k + 0.5) * resolution + a)
 *   Each occupied voxel is output once, in ascending lexicographic (kx, ky, kz) order, with intensity 0 (the reference's octree path
 *   carries none, MCG:84).
 *
 * ASSUMED ABOUT PCL.  PCL's sources were not at hand when this was written; the following is from recollection of PCL 1.10
 * (octree_pointcloud.hpp, adoptBoundingBoxToPoint / genOctreeKeyforPoint / genLeafNodeCenterFromOctreeKey).  PCL starts its bounding box
 * at q0 -+ resolution / 2, grows it by powers of two and moves its lower corner by whole multiples of the resolution; a voxel's centre is
 * (key + 0.5) * resolution + lower corner.  Its lattice is therefore the one above up to the double rounding of that moved corner: both
 * forms round the same real number from doubles that differ by about 1e-13, so every centre agrees within one float ulp per coordinate
 * (tests/test_map_cloud_restatement.py holds a NumPy emulation of that growth to this bound).  A point that lies exactly ON a cell face
 * -- float coordinates an odd multiple of 1/8 from the anchor's do at resolution 0.05 -- falls to one side by the rounding of the double
 * quotient, in PCL as here, so the two may put such a point into neighbouring voxels.  PCL's OUTPUT ORDER is a depth-first walk of its
 * tree and is not reproduced; the consumers (toROSMsg, a PCD file) do not depend on it.
 *
 * Limits, each refused before or without touching the result held:
 *   count <= 0 (the reference returns nullptr, MCG:14-17), null arguments, a non-finite pose entry in rows 0..2,
 *   a NaN resolution, a store on another device, more than INT_MAX / 2 listed points in total          GORIO_ERR_INVALID
 *   an id never added GORIO_ERR_INVALID, a released id GORIO_ERR_STATE (the texts of the keyframe store)
 *   a cell coordinate with |k| >= 2^30, an occupied-voxel bounding box of 2^21 cells or more on an
 *   axis (the sort key holds 3 x 21 bits), more than 65535 keyframes in one call                       GORIO_ERR_UNSUPPORTED
 * "Every point dropped" is not an error: GORIO_OK with 0 points.
 */
#ifndef GORIO_MAP_H
#define GORIO_MAP_H

#include "gorio_keyframes.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gorio_map gorio_map_t; /* the MapCloudGenerator object, RGS:113 */

/* map_cloud_generator.reset(new MapCloudGenerator()) (RGS:113, MCG:9).  Only checks and stores its arguments (device >= 0). */
int gorio_map_create(gorio_map_t** out, int device);
/* MCG:11. */
void gorio_map_destroy(gorio_map_t* m);

/*
 * generate(snapshot, resolution), MCG:13-89, as RGS:858-878 and RGS:1184 call it: ids[count] in the order the keyframes are listed,
 * poses[count][16] row-major double (the snapshot's poses of the moment; rows 0..2 are read).  A keyframe may be listed more than once.
 * n_points receives the size of the cloud, which gorio_map_get then hands out.  The store's counters do not move.
 * On the device: a frame table goes up; per 256-point block the gate is counted (ballot + popcount), one exclusive scan over all block
 * counts, one pass writes every kept point, transformed, at its rank and takes the rank of the first finite one (an integer atomicMin);
 * then cells and their integer bounding box, ONE small record back for the limit checks, 64-bit keys, the tiled sort, one centre per
 * first occurrence of a key.  The voxel count comes back in one 4-byte copy.  No floating-point atomics: the result is deterministic.
 */
int gorio_map_generate(gorio_map_t* m, gorio_kf_t* kf, const int* ids, const double* poses, int count, double resolution, int* n_points);

/* The cloud of the last successful generate (what RGS:876 / RGS:1197 hand to toROSMsg / savePCDFileBinary): xyz / intensity may be NULL;
 * stride_bytes between points for both arrays (a multiple of 4; >= 12 with xyz); capacity in points >= the cloud's size.  Returns
 * GORIO_OK and writes nothing before the first generate (0 points). */
int gorio_map_get(gorio_map_t* m, float* xyz, float* intensity, int stride_bytes, int capacity);

typedef struct {
  int n_listed;     /* points of the listed keyframes */
  int n_kept;       /* after the gate: the size of stage A's output */
  int n_finite;     /* kept points with a finite q (0 with resolution <= 0: stage B did not run) */
  int n_voxels;     /* occupied voxels (0 with resolution <= 0) */
  double anchor[3]; /* a = (double)q0 - resolution / 2 (0 without a finite point) */
  int min_k[3];     /* the occupied cells' bounding box (0 without a finite point) */
  int max_k[3];
} gorio_map_info_t;
/* Parity hook, no device call: the figures of the last successful generate (all 0 before the first). */
int gorio_map_info(const gorio_map_t* m, gorio_map_info_t* out);

/* Cumulative since create: generates = successful gorio_map_generate calls; points_downloaded = points handed out by gorio_map_get;
 * bytes_uploaded = all that generate sends to the device: the frame table, 72 bytes per listed keyframe (two pointers, two counts, twelve
 * floats of the pose), and with resolution > 0 the 52-byte record in its initial state.  Any pointer may be NULL. */
int gorio_map_get_counters(const gorio_map_t* m, long long* generates, long long* points_downloaded, long long* bytes_uploaded);
/* Elements per device buffer, as gorio_ndt_get_capacities: capacities[6] = frame table (bytes), block counts, stage A points, sort keys,
 * result points, record (bytes).  Buffers grow and are kept when a smaller map follows. */
int gorio_map_get_capacities(const gorio_map_t* m, long long* capacities);

const char* gorio_map_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GORIO_MAP_H */
