// facade_yaw.cpp -- drives FrontierFinder::planPathToViewpoint, BsplineOptimizer::planThroughWaypoints and then
// BsplineOptimizer::planYawExplore the way FastExplorationManager::planExploreMotion calls planExploreTraj and
// planYawExplore on the close / far branch (fast_exploration_manager.cpp:244-281), and prints one JSON document that
// tests/test_yaw_plan_gpu.py reads: per problem the branch, the solved position spline and the yaw spline.
//   facade_yaw <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; one occupancy log-odds grid (f64, the map's voxel count);
// then any number of problems, double start[3], goal[3], velocity[3], acceleration[3], start_yaw[3], end_yaw, relax_time.
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
  const std::vector<double> pr = read_records(in, 17);
  fclose(in);
  std::printf("{\"problems\": [");
  for (size_t b = 0; b < pr.size() / 17; ++b) {
    const double* q = pr.data() + 17 * b;
    const Eigen::Vector3d pos(q[0], q[1], q[2]), next_pos(q[3], q[4], q[5]), vel(q[6], q[7], q[8]), acc(q[9], q[10], q[11]);
    const Eigen::Vector3d yaw(q[12], q[13], q[14]);
    const double next_yaw = q[15], relax_time = q[16];
    std::vector<Eigen::Vector3d> path_next_goal;
    Eigen::Vector3d next_goal(0, 0, 0);
    const int branch = ff.planPathToViewpoint(pos, next_pos, path_next_goal, next_goal);
    std::printf("%s\n{\"branch\": %d", b ? "," : "", branch);
    if (branch == FUELMI_GOAL_CLOSE || branch == FUELMI_GOAL_FAR) {  // (the mid branch is kinodynamicReplan's)
      Eigen::MatrixXd ctrl_pts, yaw_ctrl;
      double dt = 0.0, dt_yaw = 0.0;
      const int cost_mask = BsplineOptimizer::NORMAL_PHASE | BsplineOptimizer::MINTIME;
      const int status = opt.planThroughWaypoints(path_next_goal, vel, acc, 2.0, 0.45, cost_mask, -1.0, ctrl_pts, dt);
      std::printf(", \"traj_status\": %d", status);
      if (status == FUELMI_WPTRAJ_OK) {
        std::printf(", \"pos_dt\": %.17g, \"pos_ctrl\": [", dt);
        for (int i = 0; i < ctrl_pts.rows(); ++i)
          std::printf("%s[%.17g, %.17g, %.17g]", i ? ", " : "", ctrl_pts(i, 0), ctrl_pts(i, 1), ctrl_pts(i, 2));
        // fast_exploration_manager.cpp:281: planYawExplore(yaw, next_yaw, true, relax_time)
        const int ys = opt.planYawExplore(ctrl_pts, 3, dt, yaw, next_yaw, true, relax_time, yaw_ctrl, dt_yaw);
        std::printf("], \"yaw_status\": %d, \"yaw_rows\": %d, \"dt_yaw\": %.17g, \"yaw_ctrl\": [", ys, (int)yaw_ctrl.rows(),
                    dt_yaw);
        for (int i = 0; i < yaw_ctrl.rows(); ++i) std::printf("%s%.17g", i ? ", " : "", yaw_ctrl(i, 0));
        // a hover: start (0, 0, 0) to end 0 is refused with its status, and the outputs stay as they were
        Eigen::MatrixXd keep = Eigen::MatrixXd(2, 1);
        keep(0, 0) = 5.0, keep(1, 0) = 6.0;
        double keep_dt = -1.0;
        const int zs = opt.planYawExplore(ctrl_pts, 3, dt, Eigen::Vector3d(0, 0, 0), 0.0, false, relax_time, keep, keep_dt);
        std::printf("], \"hover_status\": %d, \"hover_untouched\": %d", zs,
                    (keep.rows() == 2 && keep(0, 0) == 5.0 && keep(1, 0) == 6.0 && keep_dt == -1.0) ? 1 : 0);
        // planYaw on the same spline
        std::vector<double> path_yaw;
        Eigen::MatrixXd fy;
        double fdt = 0.0;
        const int fs = opt.planYaw(ctrl_pts, 3, dt, yaw, fy, fdt, &path_yaw);
        std::printf(", \"follow_status\": %d, \"follow_rows\": %d, \"follow_dt_yaw\": %.17g, \"follow_path_yaw\": %d", fs,
                    (int)fy.rows(), fdt, (int)path_yaw.size());
      }
    }
    std::printf("}");
  }
  std::printf("\n]}\n");
  return 0;
}
