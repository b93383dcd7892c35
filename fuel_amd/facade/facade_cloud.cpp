// facade_cloud.cpp -- the three map scans of MapROS::visCallback (plan_env/src/map_ros.cpp:87-103) WITH EVERY MIRROR
// SWITCHED OFF: a map, a few fusions, then the clouds of publishMapLocal, publishMapAll with its known-voxel count, and
// publishUnknown, each through two routes:
//   device  SDFMap::extractCloud / countVoxels (fuelmi_map_extract_cloud)
//   host    refresh the occupancy mirror for the box (fuelmi_map_sync_host), then the reference's loops restated below
// and prints one JSON document: counts, whether the two routes are byte-equal, the median time of each route.
//   facade_cloud [map_size_x map_size_y map_size_z [reps]]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>

namespace fast_planner {
// the package's own ViewNode in a FUEL workspace (graph_node.cpp); the facade library refers to it, nothing here calls it
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
// the reference's MapROS is a friend of SDFMap: it calls clearAndInflateLocalMap and reads mp_ / md_
class MapROS {
public:
  static void inflate(SDFMap& m) { m.clearAndInflateLocalMap(); }
  static void refresh(SDFMap& m, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi) {
    m.syncMirrors(lo, hi, true, false, false);
  }
  static void mirrors(SDFMap& m, int out[3]) {
    out[0] = m.ext_->mirror_occ, out[1] = m.ext_->mirror_infl, out[2] = m.ext_->mirror_dist;
  }
  static void cuts(SDFMap& m, Eigen::Vector3i& min_cut, Eigen::Vector3i& max_cut) {  // map_ros.cpp:263-266, :320-323
    min_cut = m.md_->local_bound_min_, max_cut = m.md_->local_bound_max_;
    m.boundIndex(min_cut);
    m.boundIndex(max_cut);
  }
  static void box(SDFMap& m, Eigen::Vector3i& lo, Eigen::Vector3i& hi) { lo = m.mp_->box_min_, hi = m.mp_->box_max_; }

  // one selected voxel -> the cloud (map_ros.cpp:224-231, :274-282, :329-336)
  static void push(SDFMap& m, int x, int y, int z, double z_low, double z_high, std::vector<float>& xyz) {
    Eigen::Vector3d pos;
    m.indexToPos(Eigen::Vector3i(x, y, z), pos);
    if (pos(2) > z_high) return;
    if (pos(2) < z_low) return;
    xyz.push_back((float)pos(0));
    xyz.push_back((float)pos(1));
    xyz.push_back((float)pos(2));
  }
  // publishMapAll's first loop (map_ros.cpp:220-233): the box, upper bounds exclusive
  static void loopMapAll(SDFMap& m, double z_low, double z_high, std::vector<float>& xyz) {
    for (int x = m.mp_->box_min_(0); x < m.mp_->box_max_(0); ++x)
      for (int y = m.mp_->box_min_(1); y < m.mp_->box_max_(1); ++y)
        for (int z = m.mp_->box_min_(2); z < m.mp_->box_max_(2); ++z)
          if (m.md_->occupancy_buffer_[m.toAddress(x, y, z)] > m.mp_->min_occupancy_log_) push(m, x, y, z, z_low, z_high, xyz);
  }
  // ... and its second (map_ros.cpp:246-251), counting instead of summing 0.1 * 0.1 * 0.1
  static long loopKnown(SDFMap& m) {
    long n = 0;
    for (int x = m.mp_->box_min_(0); x < m.mp_->box_max_(0); ++x)
      for (int y = m.mp_->box_min_(1); y < m.mp_->box_max_(1); ++y)
        for (int z = m.mp_->box_min_(2); z < m.mp_->box_max_(2); ++z)
          if (m.md_->occupancy_buffer_[m.toAddress(x, y, z)] > m.mp_->clamp_min_log_ - 1e-3) ++n;
    return n;
  }
  // publishMapLocal (map_ros.cpp:269-283): the local bound in x and y, the box in z
  static void loopMapLocal(SDFMap& m, const Eigen::Vector3i& min_cut, const Eigen::Vector3i& max_cut, double z_low,
                           double z_high, std::vector<float>& xyz) {
    for (int x = min_cut(0); x <= max_cut(0); ++x)
      for (int y = min_cut(1); y <= max_cut(1); ++y)
        for (int z = m.mp_->box_min_(2); z < m.mp_->box_max_(2); ++z)
          if (m.md_->occupancy_buffer_[m.toAddress(x, y, z)] > m.mp_->min_occupancy_log_) push(m, x, y, z, z_low, z_high, xyz);
  }
  // publishUnknown (map_ros.cpp:325-337)
  static void loopUnknown(SDFMap& m, const Eigen::Vector3i& min_cut, const Eigen::Vector3i& max_cut, double z_low,
                          double z_high, std::vector<float>& xyz) {
    for (int x = min_cut(0); x <= max_cut(0); ++x)
      for (int y = min_cut(1); y <= max_cut(1); ++y)
        for (int z = min_cut(2); z <= max_cut(2); ++z)
          if (m.md_->occupancy_buffer_[m.toAddress(x, y, z)] < m.mp_->clamp_min_log_ - 1e-3) push(m, x, y, z, z_low, z_high, xyz);
  }
};
}  // namespace fast_planner
using namespace fast_planner;

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

static bool same(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

int main(int argc, char** argv) {
  double size[3] = {20.0, 16.0, 3.0};
  if (argc > 3)
    for (int i = 0; i < 3; ++i) size[i] = atof(argv[1 + i]);
  const int reps = argc > 4 ? std::max(atoi(argv[4]), 1) : 5;
  ros::NodeHandle nh;
  auto& P = nh.num;
  P["sdf_map/resolution"] = 0.1;
  P["sdf_map/map_size_x"] = size[0], P["sdf_map/map_size_y"] = size[1], P["sdf_map/map_size_z"] = size[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = -1.0;
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  const double org[3] = {-size[0] / 2.0, -size[1] / 2.0, -1.0};
  for (int i = 0; i < 3; ++i) {  // a box a little inside the map
    P[std::string("sdf_map/box_min_") + ax[i]] = org[i] + 0.3;
    P[std::string("sdf_map/box_max_") + ax[i]] = org[i] + size[i] - 0.3;
  }
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  if (!map->device()) return 3;
  map->setHostMirror(false, false, false);  // nothing below refreshes a mirror unless it says so
  // a few fusions: a wavy wall 2 to 3.5 m in front of a camera that moves along x and turns
  const int n_frames = 6;
  for (int k = 0; k < n_frames; ++k) {
    const double yaw = 0.5 * k;
    const Eigen::Vector3d cam(-0.3 * size[0] + 0.6 * size[0] * k / (n_frames - 1), 0.2 * size[1] * std::sin(1.3 * k), 0.2);
    pcl::PointCloud<pcl::PointXYZ> cloud;
    for (int i = 0; i < 120; ++i)
      for (int j = 0; j < 60; ++j) {
        const double az = yaw - 0.7 + 1.4 * i / 119.0, el = -0.35 + 0.7 * j / 59.0;
        const double r = 2.7 + 0.7 * std::sin(5.0 * az + k) + 0.1 * std::cos(9.0 * el);
        cloud.push_back(pcl::PointXYZ((float)(cam(0) + r * std::cos(el) * std::cos(az)),
                                      (float)(cam(1) + r * std::cos(el) * std::sin(az)), (float)(cam(2) + r * std::sin(el))));
      }
    map->inputPointCloud(cloud, (int)cloud.size(), cam);
    MapROS::inflate(*map);
  }
  int mir[3];
  MapROS::mirrors(*map, mir);
  const double z_low = -0.35, z_high = 1.0;  // visualization_truncate_low_ / _height_
  Eigen::Vector3i min_cut, max_cut, bmin, bmax;
  MapROS::cuts(*map, min_cut, max_cut);
  MapROS::box(*map, bmin, bmax);
  const Eigen::Vector3i bhi = bmax - Eigen::Vector3i(1, 1, 1);  // the reference's `<`
  std::vector<float> dev, host;
  std::printf("{\"mirrors\": [%d, %d, %d], \"voxels\": [%d, %d, %d], \"reps\": %d", mir[0], mir[1], mir[2],
              (int)std::ceil(size[0] / 0.1), (int)std::ceil(size[1] / 0.1), (int)std::ceil(size[2] / 0.1), reps);

  // publishMapLocal
  {
    const Eigen::Vector3i lo(min_cut(0), min_cut(1), bmin(2)), hi(max_cut(0), max_cut(1), bhi(2));
    int n_dev = 0;
    const double us_dev = median_us(reps, [&] { n_dev = map->extractCloud(SDFMap::CLOUD_OCCUPIED, lo, hi, z_low, z_high, dev); });
    const double us_host = median_us(reps, [&] {
      MapROS::refresh(*map, lo, hi);
      host.clear();
      MapROS::loopMapLocal(*map, min_cut, max_cut, z_low, z_high, host);
    });
    std::printf(",\n\"publishMapLocal\": {\"n_device\": %d, \"n_host\": %zu, \"byte_equal\": %s, \"device_us\": %.1f, "
                "\"sync_and_host_loop_us\": %.1f, \"box_voxels\": %ld}",
                n_dev, host.size() / 3, same(dev, host) ? "true" : "false", us_dev, us_host,
                (long)(hi(0) - lo(0) + 1) * (hi(1) - lo(1) + 1) * (hi(2) - lo(2) + 1));
  }
  // publishMapAll and known_volumn
  {
    int n_dev = 0, known_dev = 0;
    long known_host = 0;
    const double us_dev = median_us(reps, [&] { n_dev = map->extractCloud(SDFMap::CLOUD_OCCUPIED, bmin, bhi, z_low, z_high, dev); });
    const double us_kdev = median_us(reps, [&] { known_dev = map->countVoxels(SDFMap::CLOUD_KNOWN, bmin, bhi); });
    double us_loop2 = 0.0;
    const double us_host = median_us(reps, [&] {
      MapROS::refresh(*map, bmin, bhi);
      host.clear();
      MapROS::loopMapAll(*map, z_low, z_high, host);
      const auto a = std::chrono::steady_clock::now();
      known_host = MapROS::loopKnown(*map);
      us_loop2 = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count();
    });
    std::printf(",\n\"publishMapAll\": {\"n_device\": %d, \"n_host\": %zu, \"byte_equal\": %s, \"known_device\": %d, "
                "\"known_host\": %ld, \"known_volumn\": %.17g, \"device_us\": %.1f, \"known_device_us\": %.1f, "
                "\"sync_and_host_loops_us\": %.1f, \"of_which_known_loop_us\": %.1f, \"box_voxels\": %ld}",
                n_dev, host.size() / 3, same(dev, host) ? "true" : "false", known_dev, known_host,
                known_dev * (0.1 * 0.1 * 0.1), us_dev, us_kdev, us_host, us_loop2,
                (long)(bhi(0) - bmin(0) + 1) * (bhi(1) - bmin(1) + 1) * (bhi(2) - bmin(2) + 1));
  }
  // publishUnknown
  {
    int n_dev = 0;
    const double us_dev = median_us(reps, [&] { n_dev = map->extractCloud(SDFMap::CLOUD_UNKNOWN, min_cut, max_cut, z_low, z_high, dev); });
    const double us_host = median_us(reps, [&] {
      MapROS::refresh(*map, min_cut, max_cut);
      host.clear();
      MapROS::loopUnknown(*map, min_cut, max_cut, z_low, z_high, host);
    });
    std::printf(",\n\"publishUnknown\": {\"n_device\": %d, \"n_host\": %zu, \"byte_equal\": %s, \"device_us\": %.1f, "
                "\"sync_and_host_loop_us\": %.1f, \"box_voxels\": %ld}",
                n_dev, host.size() / 3, same(dev, host) ? "true" : "false", us_dev, us_host,
                (long)(max_cut(0) - min_cut(0) + 1) * (max_cut(1) - min_cut(1) + 1) * (max_cut(2) - min_cut(2) + 1));
  }
  std::printf("}\n");
  return 0;
}
