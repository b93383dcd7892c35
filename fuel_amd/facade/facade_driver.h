// facade_driver.h -- what every facade_*.cpp driver needs before its own main: the stand-ins for the open ends of
// libfuelmi_facade.so, the reference's launch-file parameters, and the occupancy-grid load.  A new driver is this
// include, the parameter calls it needs, and main.
//
// Included by EXACTLY ONE translation unit per executable: it defines non-inline members of ViewNode and
// PerceptionUtils, and the one class MapROS a program may have.
#ifndef FUELMI_FACADE_DRIVER_H
#define FUELMI_FACADE_DRIVER_H

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <plan_env/edt_environment.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>

namespace fast_planner {
// The facade library refers to ViewNode and PerceptionUtils and does not replace them: in a FUEL workspace they are the
// active_perception package's own graph_node.cpp (A* through the map) and perception_utils.cpp.  Here: straight flight
// plus a yaw term, the path is its two end points (tests/test_facade_gpu.py rebuilds the expected cost matrix with the
// same formula).  Only a FrontierFinder without frontier/device_path_cost reaches them.
double ViewNode::computeCost(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2, const double& y1, const double& y2,
                             const Eigen::Vector3d&, const double&, std::vector<Eigen::Vector3d>& path) {
  path = {p1, p2};
  return (p2 - p1).norm() + 0.1 * std::fabs(y2 - y1);
}
double ViewNode::searchPath(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2, std::vector<Eigen::Vector3d>& path) {
  path = {p1, p2};
  return (p2 - p1).norm();
}
PerceptionUtils::PerceptionUtils(ros::NodeHandle&) {}

// The reference's MapROS is a friend of SDFMap: it calls the private clearAndInflateLocalMap
// (plan_env/src/map_ros.cpp:142,170) and reads mp_ / md_ in its display loops (:217-346).  This stand-in does the same;
// a driver that restates such a loop builds it as a free function on param() and data().
class MapROS {
public:
  static void inflate(SDFMap& m) { m.clearAndInflateLocalMap(); }
  // the named host mirrors of the inclusive index box, from the device, whatever setHostMirror says
  static void refresh(SDFMap& m, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi, bool occ, bool infl, bool dist) {
    m.syncMirrors(lo, hi, occ, infl, dist);
  }
  static void mirrors(SDFMap& m, int out[3]) {
    out[0] = m.ext_->mirror_occ, out[1] = m.ext_->mirror_infl, out[2] = m.ext_->mirror_dist;
  }
  static const MapParam& param(SDFMap& m) { return *m.mp_; }
  static const MapData& data(SDFMap& m) { return *m.md_; }
};
}  // namespace fast_planner
using namespace fast_planner;

// ---- files ----
template <typename T>
static void rd(FILE* f, T* p, size_t n) {
  if (fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
}
// every record of k doubles up to the end of the file, back to back
static inline std::vector<double> read_records(FILE* f, size_t k) {
  std::vector<double> all, rec(k);
  while (fread(rec.data(), sizeof(double), k, f) == k) all.insert(all.end(), rec.begin(), rec.end());
  return all;
}

// one point-cloud frame of facade_demo's scenario format: int n, double cam[3], float xyz[n][3]
struct Frame {
  pcl::PointCloud<pcl::PointXYZ> cloud;
  std::vector<float> xyz;
  double cam[3];
  void fuse(SDFMap& map) const { map.inputPointCloud(cloud, (int)cloud.points.size(), Eigen::Vector3d(cam[0], cam[1], cam[2])); }
};
static inline Frame read_frame(FILE* f) {
  Frame fr;
  int n;
  rd(f, &n, 1);
  rd(f, fr.cam, 3);
  fr.xyz.resize((size_t)n * 3);
  rd(f, fr.xyz.data(), fr.xyz.size());
  fr.cloud.points.resize(n);
  for (int i = 0; i < n; ++i) fr.cloud.points[i] = pcl::PointXYZ(fr.xyz[3 * i], fr.xyz[3 * i + 1], fr.xyz[3 * i + 2]);
  return fr;
}

template <class F>
static double median_us(int reps, F f) {
  std::vector<double> us;
  for (int r = 0; r < reps; ++r) {
    const auto a = std::chrono::steady_clock::now();
    f();
    us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count());
  }
  std::sort(us.begin(), us.end());
  return us[us.size() / 2];
}

// ---- parameters: the values of the reference's launch files (exploration_manager/launch/algorithm.xml) ----
static inline void sdf_map_params(ros::NodeHandle& nh, const double map_size[3], const double box_min[3],
                                  const double box_max[3], double resolution = 0.1, double ground_height = -1.0) {
  auto& P = nh.num;
  P["sdf_map/resolution"] = resolution;
  P["sdf_map/map_size_x"] = map_size[0], P["sdf_map/map_size_y"] = map_size[1], P["sdf_map/map_size_z"] = map_size[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = ground_height;
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    P[std::string("sdf_map/box_min_") + ax[i]] = box_min[i];
    P[std::string("sdf_map/box_max_") + ax[i]] = box_max[i];
  }
}
// the box of a driver whose scenario names none: the whole map from the ground up ...
static inline void whole_map_box(const double map_size[3], double ground_height, double lo[3], double hi[3]) {
  for (int i = 0; i < 3; ++i) {
    lo[i] = i < 2 ? -map_size[i] / 2.0 : ground_height;
    hi[i] = lo[i] + map_size[i];
  }
}
// ... or 0.3 m inside it on every side
static inline void inset_box(const double map_size[3], double lo[3], double hi[3]) {
  const double org[3] = {-map_size[0] / 2.0, -map_size[1] / 2.0, -1.0};
  for (int i = 0; i < 3; ++i) lo[i] = org[i] + 0.3, hi[i] = org[i] + map_size[i] - 0.3;
}

// frontier/* and the camera of perception_utils/* (algorithm.xml:103-120)
static inline void frontier_params(ros::NodeHandle& nh, double cluster_min, double cluster_size_xy, double min_visib_num) {
  auto& P = nh.num;
  P["frontier/cluster_min"] = cluster_min;
  P["frontier/cluster_size_xy"] = cluster_size_xy;
  P["frontier/down_sample"] = 3;
  P["frontier/candidate_rmin"] = 1.5;
  P["frontier/candidate_rmax"] = 2.5;
  P["frontier/candidate_rnum"] = 3;
  P["frontier/candidate_dphi"] = 15 * 3.1415926 / 180.0;
  P["frontier/min_candidate_clearance"] = 0.21;
  P["frontier/min_visib_num"] = min_visib_num;
  P["frontier/min_candidate_dist"] = 0.75;
  P["frontier/min_view_finish_fraction"] = 0.2;
  P["perception_utils/top_angle"] = 0.56125;
  P["perception_utils/left_angle"] = 0.69222;
  P["perception_utils/right_angle"] = 0.68901;
  P["perception_utils/max_dist"] = 4.5;
}
// the ViewNode parameters the device path costs and the tour refinement need (algorithm.xml:95-99)
static inline void exploration_params(ros::NodeHandle& nh) {
  auto& P = nh.num;
  P["exploration/vm"] = 2.0;
  P["exploration/yd"] = 60 * 3.1415926 / 180.0;
  P["exploration/w_dir"] = 1.5;
}
// optimization/* (algorithm.xml:170-194) without the wall-clock caps: a result must not depend on the clock.  A driver
// that deviates overrides single keys after the call.
static inline void optimization_params(ros::NodeHandle& nh) {
  auto& P = nh.num;
  P["optimization/ld_smooth"] = 20.0, P["optimization/ld_dist"] = 10.0, P["optimization/ld_feasi"] = 2.0;
  P["optimization/ld_start"] = 100.0, P["optimization/ld_end"] = 0.5, P["optimization/ld_guide"] = 1.5;
  P["optimization/ld_waypt"] = 0.3, P["optimization/ld_view"] = 0.0, P["optimization/ld_time"] = 1.0;
  P["optimization/dist0"] = 0.7, P["optimization/max_vel"] = 2.0, P["optimization/max_acc"] = 2.0;
  P["optimization/dlmin"] = 0.0, P["optimization/wnl"] = 1.0;
  P["optimization/max_iteration_num1"] = 2, P["optimization/max_iteration_num2"] = 100;
  P["optimization/max_iteration_num3"] = 100, P["optimization/max_iteration_num4"] = 100;
  P["manager/bspline_degree"] = 3;
}

// ---- the map ----
struct DriverMap {
  SDFMap::Ptr map;
  EDTEnvironment::Ptr edt;
  int voxels;
};
// a map on the device from nh's sdf_map/* and its environment; mirrors_off: no mutator refreshes a host mirror
static inline DriverMap make_map(ros::NodeHandle& nh, bool mirrors_off) {
  DriverMap d;
  d.map.reset(new SDFMap);
  d.map->initMap(nh);
  if (!d.map->device()) std::exit(3);
  if (mirrors_off) d.map->setHostMirror(false, false, false);
  d.edt.reset(new EDTEnvironment);
  d.edt->setMap(d.map);
  d.voxels = d.map->getVoxelNum();
  return d;
}

// What follows the upload of an occupancy log-odds grid, in this order.  The drivers differ here on purpose: a step is
// made only where the driver names it.
enum {
  LOAD_BOUND = 1,        // the whole map as the local bound
  LOAD_INFLATE = 2,      // clearAndInflateLocalMap as MapROS calls it (refreshes the inflate mirror if that is on)
  LOAD_INFLATE_ABI = 4,  // fuelmi_map_inflate_local alone
  LOAD_ESDF = 8,         // updateESDF3d
};
// ... and last, with a box, that box as the updated box the next frontier search reads
static inline void upload_occupancy(SDFMap& map, const std::vector<double>& occ, int steps, const double* box_lo = nullptr,
                                    const double* box_hi = nullptr) {
  fuelmi_map* m = map.device();
  fuelmi_map_info info;
  fuelmi_map_get_info(m, &info);
  const int b0[3] = {0, 0, 0};
  const int b1[3] = {info.voxel_num[0] - 1, info.voxel_num[1] - 1, info.voxel_num[2] - 1};
  if (occ.size() != (size_t)map.getVoxelNum() || fuelmi_map_upload_occupancy(m, occ.data()) ||
      ((steps & LOAD_BOUND) && fuelmi_map_set_local_bound(m, b0, b1)) ||
      ((steps & LOAD_INFLATE_ABI) && fuelmi_map_inflate_local(m))) {
    std::fprintf(stderr, "occupancy upload failed: %s\n", fuelmi_last_error());
    std::exit(3);
  }
  if (steps & LOAD_INFLATE) MapROS::inflate(map);
  if (steps & LOAD_ESDF) map.updateESDF3d();
  if (box_lo) fuelmi_map_set_updated_box(m, box_lo, box_hi);
}
// the same for the next grid of a scenario file (f64, the map's voxel count)
static inline void load_occupancy(SDFMap& map, FILE* in, int steps, const double* box_lo = nullptr,
                                  const double* box_hi = nullptr) {
  std::vector<double> occ((size_t)map.getVoxelNum());
  rd(in, occ.data(), occ.size());
  upload_occupancy(map, occ, steps, box_lo, box_hi);
}
#endif
