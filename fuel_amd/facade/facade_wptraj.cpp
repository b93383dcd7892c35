// facade_wptraj.cpp -- drives FrontierFinder::planPathToViewpoint and then BsplineOptimizer::planThroughWaypoints the way
// FastExplorationManager::planExploreMotion calls planExploreTraj on the close / far branch
// (fast_exploration_manager.cpp:244-263, plan_manage/src/planner_manager.cpp:266-316), and prints what
// tests/test_waypoint_traj_gpu.py compares: the way-points, the spline handed to the solve, the solved spline and its cost.
//   facade_wptraj <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; one occupancy log-odds grid (f64, the map's voxel count);
// then any number of problems, double start[3], goal[3], velocity[3], acceleration[3] each.
#include "facade_driver.h"

#include <active_perception/frontier_finder.h>
#include <bspline_opt/bspline_optimizer.h>

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[9];
  rd(in, hdr, 9);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6);
  frontier_params(nh, 10, 1.0, 3);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, false);
  FrontierFinder ff(dm.edt, nh);
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE | LOAD_ESDF, hdr + 3, hdr + 6);
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(dm.edt);
  const std::vector<double> pr = read_records(in, 12);
  fclose(in);
  // an empty tour is refused, not indexed
  {
    Eigen::MatrixXd c;
    double d = 0.0;
    std::printf("empty %d\n", opt.planThroughWaypoints({}, Eigen::Vector3d(0, 0, 0), Eigen::Vector3d(0, 0, 0), 2.0, 0.45,
                                                         BsplineOptimizer::NORMAL_PHASE, -1.0, c, d));
  }
  for (size_t b = 0; b < pr.size() / 12; ++b) {
    const double* q = pr.data() + 12 * b;
    const Eigen::Vector3d pos(q[0], q[1], q[2]), next_pos(q[3], q[4], q[5]), vel(q[6], q[7], q[8]), acc(q[9], q[10], q[11]);
    std::vector<Eigen::Vector3d> path_next_goal;
    Eigen::Vector3d next_goal(0, 0, 0);
    const int branch = ff.planPathToViewpoint(pos, next_pos, path_next_goal, next_goal);
    std::printf("goal %zu %d %zu %.17g %.17g %.17g\n", b, branch, path_next_goal.size(), next_goal(0), next_goal(1),
                next_goal(2));
    for (auto& w : path_next_goal) std::printf("way %zu %.17g %.17g %.17g\n", b, w(0), w(1), w(2));
    if (branch != FUELMI_GOAL_CLOSE && branch != FUELMI_GOAL_FAR) continue;  // (the mid branch is kinodynamicReplan's)
    Eigen::MatrixXd ctrl_pts;
    double dt = 0.0;
    const int cost_mask = BsplineOptimizer::NORMAL_PHASE | BsplineOptimizer::MINTIME;
    const int status = opt.planThroughWaypoints(path_next_goal, vel, acc, 2.0, 0.45, cost_mask, -1.0, ctrl_pts, dt);
    std::printf("traj %zu %d %d %.17g %.17g %.17g\n", b, status, (int)ctrl_pts.rows(), opt.init_knot_span_, dt,
                opt.final_cost_);
    if (status != FUELMI_WPTRAJ_OK) continue;
    for (int i = 0; i < opt.init_ctrl_pts_.rows(); ++i)
      std::printf("init %zu %.17g %.17g %.17g\n", b, opt.init_ctrl_pts_(i, 0), opt.init_ctrl_pts_(i, 1), opt.init_ctrl_pts_(i, 2));
    for (int i = 0; i < ctrl_pts.rows(); ++i)
      std::printf("ctrl %zu %.17g %.17g %.17g\n", b, ctrl_pts(i, 0), ctrl_pts(i, 1), ctrl_pts(i, 2));
  }
  return 0;
}
