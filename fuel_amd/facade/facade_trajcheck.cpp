// facade_trajcheck.cpp -- drives BsplineOptimizer::checkTrajCollision the way the exploration FSM's safetyCallback calls
// FastPlannerManager::checkTrajCollision (fast_exploration_fsm.cpp:335-345) WITH THE INFLATE MIRROR SWITCHED OFF, and
// prints one JSON document that tests/test_traj_check_gpu.py reads: per problem the device's answer, and what the
// reference's host loop answers through the facade's getters on the mirror nobody refreshed.
//   facade_trajcheck <scenario.bin> [reps]
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height; one occupancy log-odds grid
// (f64, the map's voxel count); then any number of problems, double degree, n_ctrl, knot span, t_now and n_ctrl x 3
// control points.  With reps > 0 every problem is also timed, median of reps calls each: the device call, and the route
// it replaces (refresh the inflate mirror for the trajectory's box, then the host loop).
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

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

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const int reps = argc > 2 ? atoi(argv[2]) : 0;
  double hdr[11];
  rd(in, hdr, 11);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6, hdr[9], hdr[10]);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, true);  // nothing below refreshes a mirror unless it says so
  const SDFMap::Ptr& map = dm.map;
  load_occupancy(*map, in, LOAD_BOUND | LOAD_INFLATE);
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(dm.edt);
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
        MapROS::refresh(*map, ilo, ihi, false, true, false);
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
