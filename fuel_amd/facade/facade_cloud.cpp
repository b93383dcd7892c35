// facade_cloud.cpp -- the three map scans of MapROS::visCallback (plan_env/src/map_ros.cpp:87-103) WITH EVERY MIRROR
// SWITCHED OFF: a map, a few fusions, then the clouds of publishMapLocal, publishMapAll with its known-voxel count, and
// publishUnknown, each through two routes:
//   device  SDFMap::extractCloud / countVoxels (fuelmi_map_extract_cloud)
//   host    refresh the occupancy mirror for the box (fuelmi_map_sync_host), then the reference's loops restated below
// and prints one JSON document: counts, whether the two routes are byte-equal, the median time of each route.
//   facade_cloud [map_size_x map_size_y map_size_z [reps]]
#include "facade_driver.h"

#include <cstring>

// The reference's display loops, on what its MapROS reads as a friend of SDFMap: mp_ and md_.
static void cuts(SDFMap& m, Eigen::Vector3i& min_cut, Eigen::Vector3i& max_cut) {  // map_ros.cpp:263-266, :320-323
  min_cut = MapROS::data(m).local_bound_min_, max_cut = MapROS::data(m).local_bound_max_;
  m.boundIndex(min_cut);
  m.boundIndex(max_cut);
}
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
  const MapParam& mp = MapROS::param(m);
  const MapData& md = MapROS::data(m);
  for (int x = mp.box_min_(0); x < mp.box_max_(0); ++x)
    for (int y = mp.box_min_(1); y < mp.box_max_(1); ++y)
      for (int z = mp.box_min_(2); z < mp.box_max_(2); ++z)
        if (md.occupancy_buffer_[m.toAddress(x, y, z)] > mp.min_occupancy_log_) push(m, x, y, z, z_low, z_high, xyz);
}
// ... and its second (map_ros.cpp:246-251), counting instead of summing 0.1 * 0.1 * 0.1
static long loopKnown(SDFMap& m) {
  const MapParam& mp = MapROS::param(m);
  const MapData& md = MapROS::data(m);
  long n = 0;
  for (int x = mp.box_min_(0); x < mp.box_max_(0); ++x)
    for (int y = mp.box_min_(1); y < mp.box_max_(1); ++y)
      for (int z = mp.box_min_(2); z < mp.box_max_(2); ++z)
        if (md.occupancy_buffer_[m.toAddress(x, y, z)] > mp.clamp_min_log_ - 1e-3) ++n;
  return n;
}
// publishMapLocal (map_ros.cpp:269-283): the local bound in x and y, the box in z
static void loopMapLocal(SDFMap& m, const Eigen::Vector3i& min_cut, const Eigen::Vector3i& max_cut, double z_low,
                         double z_high, std::vector<float>& xyz) {
  const MapParam& mp = MapROS::param(m);
  const MapData& md = MapROS::data(m);
  for (int x = min_cut(0); x <= max_cut(0); ++x)
    for (int y = min_cut(1); y <= max_cut(1); ++y)
      for (int z = mp.box_min_(2); z < mp.box_max_(2); ++z)
        if (md.occupancy_buffer_[m.toAddress(x, y, z)] > mp.min_occupancy_log_) push(m, x, y, z, z_low, z_high, xyz);
}
// publishUnknown (map_ros.cpp:325-337)
static void loopUnknown(SDFMap& m, const Eigen::Vector3i& min_cut, const Eigen::Vector3i& max_cut, double z_low,
                        double z_high, std::vector<float>& xyz) {
  const MapParam& mp = MapROS::param(m);
  const MapData& md = MapROS::data(m);
  for (int x = min_cut(0); x <= max_cut(0); ++x)
    for (int y = min_cut(1); y <= max_cut(1); ++y)
      for (int z = min_cut(2); z <= max_cut(2); ++z)
        if (md.occupancy_buffer_[m.toAddress(x, y, z)] < mp.clamp_min_log_ - 1e-3) push(m, x, y, z, z_low, z_high, xyz);
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
  double box_lo[3], box_hi[3];
  inset_box(size, box_lo, box_hi);
  sdf_map_params(nh, size, box_lo, box_hi);
  const SDFMap::Ptr map = make_map(nh, true).map;  // nothing below refreshes a mirror unless it says so
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
  cuts(*map, min_cut, max_cut);
  bmin = MapROS::param(*map).box_min_, bmax = MapROS::param(*map).box_max_;
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
      MapROS::refresh(*map, lo, hi, true, false, false);
      host.clear();
      loopMapLocal(*map, min_cut, max_cut, z_low, z_high, host);
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
      MapROS::refresh(*map, bmin, bhi, true, false, false);
      host.clear();
      loopMapAll(*map, z_low, z_high, host);
      const auto a = std::chrono::steady_clock::now();
      known_host = loopKnown(*map);
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
      MapROS::refresh(*map, min_cut, max_cut, true, false, false);
      host.clear();
      loopUnknown(*map, min_cut, max_cut, z_low, z_high, host);
    });
    std::printf(",\n\"publishUnknown\": {\"n_device\": %d, \"n_host\": %zu, \"byte_equal\": %s, \"device_us\": %.1f, "
                "\"sync_and_host_loop_us\": %.1f, \"box_voxels\": %ld}",
                n_dev, host.size() / 3, same(dev, host) ? "true" : "false", us_dev, us_host,
                (long)(max_cut(0) - min_cut(0) + 1) * (max_cut(1) - min_cut(1) + 1) * (max_cut(2) - min_cut(2) + 1));
  }
  std::printf("}\n");
  return 0;
}
