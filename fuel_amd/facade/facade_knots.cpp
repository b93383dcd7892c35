// facade_knots.cpp -- drives what the reference does with a TIME-ADJUSTED trajectory, through BsplineOptimizer:
// adjustTime (the reallocation loop of FastPlannerManager, plan_manage/src/planner_manager.cpp:222-230) and then, on the
// knots it returned, the four methods that take them where they took a knot span: checkTrajCollision (the safety
// callback's walk, :96-118), evaluateCommand (traj_server's pos_traj.setKnot(knots) and cmdCallback,
// plan_manage/src/traj_server.cpp:230, :266-290), replanState (fast_exploration_fsm.cpp:86-95) and planYaw (:695-758).
// Prints one JSON document that tests/test_knots_facade_gpu.py compares with the direct calls.
//   facade_knots <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3], resolution, ground_height; one occupancy log-odds grid
// (f64, the map's voxel count); then any number of problems, double degree, n_ctrl, knot span, t_now, n_t, limit_vel,
// limit_acc, then n_ctrl x 3 control points and n_t times.
#include "facade_driver.h"

#include <bspline_opt/bspline_optimizer.h>

static void print_rows(const char* name, const Eigen::MatrixXd& m) {
  std::printf("\"%s\": [", name);
  for (int i = 0; i < (int)m.rows(); ++i)
    for (int k = 0; k < (int)m.cols(); ++k) std::printf("%s%.17g", i + k ? ", " : "", m(i, k));
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[11];
  rd(in, hdr, 11);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6, hdr[9], hdr[10]);
  optimization_params(nh);
  const DriverMap dm = make_map(nh, true);  // none of the calls below reads a mirror
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE);
  BsplineOptimizer opt;
  opt.setParam(nh);
  opt.setEnvironment(dm.edt);
  std::printf("{\"problems\": [");
  double head[7];
  for (int b = 0; fread(head, sizeof(double), 7, in) == 7; ++b) {
    const int degree = (int)head[0], n_ctrl = (int)head[1], n_t = (int)head[4];
    const double dt = head[2], t_now = head[3];
    if (n_ctrl < 1 || n_ctrl > 4096 || n_t < 1 || n_t > (1 << 20)) return 2;
    std::vector<double> c(3 * (size_t)n_ctrl), t((size_t)n_t);
    if (fread(c.data(), sizeof(double), c.size(), in) != c.size()) return 2;
    if (fread(t.data(), sizeof(double), t.size(), in) != t.size()) return 2;
    Eigen::MatrixXd ctrl(n_ctrl, 3);
    for (int i = 0; i < n_ctrl; ++i)
      for (int k = 0; k < 3; ++k) ctrl(i, k) = c[3 * i + k];
    // the time adjustment: uniform knots in (an empty vector), the moved knots out
    BsplineOptimizer::TrajAdjust cfg;
    cfg.limit_vel = head[5], cfg.limit_acc = head[6];
    BsplineOptimizer::TrajMetrics met;
    Eigen::VectorXd knots;
    if (!opt.adjustTime(ctrl, degree, dt, knots, FUELMI_TRAJADJ_LENGTHEN | FUELMI_TRAJADJ_REALLOC, nullptr, cfg, met, nullptr)) return 4;
    // ... into the four consumers
    double distance = -7.0;  // (untouched when safe)
    const bool safe = opt.checkTrajCollision(ctrl, degree, knots, t_now, distance);
    const Eigen::MatrixXd no_yaw(0, 1);
    std::vector<int> status;
    Eigen::MatrixXd pos, vel, acc, jerk, yaw;
    double flight[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!opt.evaluateCommand(ctrl, degree, knots, no_yaw, 3, 1.0, t, nullptr, status, pos, vel, acc, jerk, yaw, flight)) return 4;
    Eigen::Vector3d s_pt, s_vel, s_acc, s_yaw;
    if (!opt.replanState(ctrl, degree, knots, no_yaw, 3, 1.0, t[n_t / 2], s_pt, s_vel, s_acc, s_yaw)) return 4;
    Eigen::MatrixXd yaw_ctrl;
    double dt_yaw = 0.0;
    std::vector<double> path_yaw;
    const int yaw_status = opt.planYaw(ctrl, degree, knots, Eigen::Vector3d(0.3, 0.1, 0.0), yaw_ctrl, dt_yaw, &path_yaw);

    std::printf("%s\n{\"iters\": %d, \"duration\": %.17g, \"knots\": [", b ? "," : "", met.info[FUELMI_TRAJADJ_I_ITERS], met.duration());
    for (int i = 0; i < (int)knots.rows(); ++i) std::printf("%s%.17g", i ? ", " : "", knots(i));
    std::printf("], \"safe\": %d, \"distance\": %.17g, \"status\": [", safe ? 1 : 0, distance);
    for (size_t k = 0; k < status.size(); ++k) std::printf("%s%d", k ? ", " : "", status[k]);
    std::printf("], ");
    print_rows("pos", pos), std::printf(", "), print_rows("vel", vel), std::printf(", "), print_rows("acc", acc);
    std::printf(", "), print_rows("jerk", jerk);
    std::printf(", \"flight\": [");
    for (int k = 0; k < 8; ++k) std::printf("%s%.17g", k ? ", " : "", flight[k]);
    std::printf("], \"state\": [");
    for (int k = 0; k < 9; ++k) std::printf("%s%.17g", k ? ", " : "", k < 3 ? s_pt(k) : k < 6 ? s_vel(k - 3) : s_acc(k - 6));
    std::printf("], \"yaw_status\": %d, \"dt_yaw\": %.17g, ", yaw_status, dt_yaw);
    print_rows("yaw_ctrl", yaw_ctrl);
    std::printf(", \"path_yaw\": [");
    for (size_t k = 0; k < path_yaw.size(); ++k) std::printf("%s%.17g", k ? ", " : "", path_yaw[k]);
    std::printf("]}");
  }
  fclose(in);
  std::printf("\n]}\n");
  return 0;
}
