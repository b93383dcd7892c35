// facade_trajcheck.cpp -- drives BsplineOptimizer::checkTrajCollision the way the exploration FSM's safetyCallback calls
// FastPlannerManager::checkTrajCollision (fast_exploration_fsm.cpp:335-345) WITH THE INFLATE MIRROR SWITCHED OFF, and
// prints one JSON document that tests/test_traj_check_gpu.py reads: per problem the device's answer, and what the
// reference's host loop answers through the facade's getters on the mirror nobody refreshed.
//   facade_trajcheck <scenario.bin> [reps]
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height; one occupancy log-odds grid
// (f64, the map's voxel count); then any number of problems, double degree, n_ctrl, knot span, t_now and n_ctrl x 3
// control points.  With reps > 0 every problem is also timed, median of reps calls each: the device call, and the route
// it replaces (refresh the inflate mirror for the trajectory's box, then the host loop).
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
#include <bspline_opt/bspline_optimizer.h>

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
class MapROS {
public:
  static void inflate(SDFMap& m) { m.clearAndInflateLocalMap(); }
  static void refresh(SDFMap& m, const Eigen::Vector3i& lo, const Eigen::Vector3i& hi) {
    m.syncMirrors(lo, hi, false, true, false);
  }
};
}  // namespace fast_planner
using namespace fast_planner;

// a uniform position spline on the host: setUniformBspline's knots and evaluateDeBoorT
struct HostSpline {
  Eigen::MatrixXd ctrl;
  int p;
  std::vector<double> u;
  HostSpline(const Eigen::MatrixXd& c, int degree, double dt) : ctrl(c), p(degree) {
    const int m = (int)c.rows() + p;
    u.assign(m + 1, 0.0);
    for (int i = 0; i <= m; ++i) u[i] = i <= p ? double(i - p) * dt : u[i - 1] + dt;
  }
  double duration() const { return u[ctrl.rows()] - u[p]; }
  Eigen::Vector3d at(double t) const {
    const double ub = std::min(std::max(u[p], t + u[p]), u[ctrl.rows()]);
    int k = p;
    while (u[k + 1] < ub) ++k;
    std::vector<Eigen::Vector3d> d;
    for (int i = 0; i <= p; ++i) d.push_back(Eigen::Vector3d(ctrl(k - p + i, 0), ctrl(k - p + i, 1), ctrl(k - p + i, 2)));
    for (int r = 1; r <= p; ++r)
      for (int i = p; i >= r; --i) {
        const double alpha = (ub - u[i + k - p]) / (u[i + 1 + k - r] - u[i + k - p]);
        d[i] = (1 - alpha) * d[i - 1] + alpha * d[i];
      }
    return d[p];
  }
};

// the reference's loop on the host mirror (planner_manager.cpp:96-118)
static bool host_loop(SDFMap& map, const HostSpline& s, double t_now, double& distance) {
  const Eigen::Vector3d cur = s.at(t_now);
  const double duration = s.duration();
  double radius = 0.0, fut_t = 0.02;
  while (radius < 6.0 && t_now + fut_t < duration) {
    const Eigen::Vector3d fut = s.at(t_now + fut_t);
    if (map.getInflateOccupancy(fut) == 1) {
      distance = radius;
      return false;
    }
    radius = (fut - cur).norm();
    fut_t += 0.02;
  }
  return true;
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

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const int reps = argc > 2 ? atoi(argv[2]) : 0;
  double hdr[11];
  if (fread(hdr, sizeof(double), 11, in) != 11) return 2;
  ros::NodeHandle nh;
  auto& P = nh.num;
  P["sdf_map/resolution"] = hdr[9];
  P["sdf_map/map_size_x"] = hdr[0], P["sdf_map/map_size_y"] = hdr[1], P["sdf_map/map_size_z"] = hdr[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = hdr[10];
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    P[std::string("sdf_map/box_min_") + ax[i]] = hdr[3 + i];
    P[std::string("sdf_map/box_max_") + ax[i]] = hdr[6 + i];
  }
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  map->setHostMirror(false, false, false);  // nothing below refreshes a mirror unless it says so
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  fuelmi_map* m = map->device();
  fuelmi_map_info info;
  fuelmi_map_get_info(m, &info);
  const int N = info.voxel_num[0] * info.voxel_num[1] * info.voxel_num[2];
  {
    std::vector<double> occ(N);
    if (fread(occ.data(), sizeof(double), N, in) != (size_t)N) return 2;
    const int b0[3] = {0, 0, 0};
    const int b1[3] = {info.voxel_num[0] - 1, info.voxel_num[1] - 1, info.voxel_num[2] - 1};
    if (fuelmi_map_upload_occupancy(m, occ.data()) || fuelmi_map_set_local_bound(m, b0, b1)) return 3;
    MapROS::inflate(*map);
  }
  P["optimization/ld_smooth"] = 20.0, P["optimization/ld_dist"] = 10.0, P["optimization/ld_feasi"] = 2.0;
  P["optimization/ld_start"] = 100.0, P["optimization/ld_end"] = 0.5, P["optimization/ld_guide"] = 1.5;
  P["optimization/ld_waypt"] = 0.3, P["optimization/ld_view"] = 0.0, P["optimization/ld_time"] = 1.0;
  P["optimization/dist0"] = 0.7, P["optimization/max_vel"] = 2.0, P["optimization/max_acc"] = 2.0;
  P["optimization/dlmin"] = 0.0, P["optimization/wnl"] = 1.0;
  P["optimization/max_iteration_num1"] = 2, P["optimization/max_iteration_num2"] = 100;
  P["optimization/max_iteration_num3"] = 100, P["optimization/max_iteration_num4"] = 100;
  P["manager/bspline_degree"] = 3;
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(edt);
  std::printf("{\"problems\": [");
  double head[4];
  for (int b = 0; fread(head, sizeof(double), 4, in) == 4; ++b) {
    const int degree = (int)head[0], n_ctrl = (int)head[1];
    const double dt = head[2], t_now = head[3];
    if (n_ctrl < 1 || n_ctrl > 4096) return 2;
    std::vector<double> c(3 * (size_t)n_ctrl);
    if (fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 2;
    Eigen::MatrixXd ctrl(n_ctrl, 3);
    for (int i = 0; i < n_ctrl; ++i)
      for (int k = 0; k < 3; ++k) ctrl(i, k) = c[3 * i + k];
    double distance = -7.0;  // (untouched when safe)
    const bool safe = opt.checkTrajCollision(ctrl, degree, dt, t_now, distance);
    const HostSpline s(ctrl, degree, dt);
    double stale_distance = -7.0;
    const bool stale_safe = host_loop(*map, s, t_now, stale_distance);
    std::printf("%s\n{\"safe\": %d, \"distance\": %.17g, \"stale_mirror_safe\": %d", b ? "," : "", safe ? 1 : 0, distance,
                stale_safe ? 1 : 0);
    if (reps > 0) {
      // the route the device call replaces: refresh the inflate mirror for the control points' box (the spline lies in
      // their hull), then the host loop
      Eigen::Vector3d lo(ctrl(0, 0), ctrl(0, 1), ctrl(0, 2)), hi = lo;
      for (int i = 1; i < n_ctrl; ++i)
        for (int k = 0; k < 3; ++k) lo(k) = std::min(lo(k), ctrl(i, k)), hi(k) = std::max(hi(k), ctrl(i, k));
      Eigen::Vector3i ilo, ihi;
      map->posToIndex(lo, ilo);
      map->posToIndex(hi, ihi);
      map->boundIndex(ilo);
      map->boundIndex(ihi);
      double d = 0.0;
      bool mirror_safe = true;
      const double us_dev = median_us(reps, [&] { opt.checkTrajCollision(ctrl, degree, dt, t_now, d); });
      const double us_host = median_us(reps, [&] {
        MapROS::refresh(*map, ilo, ihi);
        mirror_safe = host_loop(*map, s, t_now, d);
      });
      std::printf(", \"fresh_mirror_safe\": %d, \"device_us\": %.3f, \"sync_and_host_loop_us\": %.3f, \"box_voxels\": %ld",
                  mirror_safe ? 1 : 0, us_dev, us_host,
                  (long)(ihi(0) - ilo(0) + 1) * (ihi(1) - ilo(1) + 1) * (ihi(2) - ilo(2) + 1));
    }
    std::printf("}");
  }
  fclose(in);
  std::printf("\n]}\n");
  return 0;
}
