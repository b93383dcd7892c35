// facade_heading.cpp -- drives HeadingPlanner the way FastPlannerManager does (plan_manage/src/planner_manager.cpp:84-85,
// planner_manager_dev.cpp:63, 210) with every host mirror of the map switched off: searchPathOfYaw per trajectory and all
// of them through searchPathsOfYaw, calcInfoGain per pose and all of them through calcInfoGains.  Prints what
// tests/test_heading_facade_gpu.py compares with fuelmi_map_yaw_paths / fuelmi_map_info_gains on an equal map; doubles as
// hexadecimal floats.
//   facade_heading <scenario.bin>
// scenario.bin (doubles): map_size[3], box_min[3], box_max[3], half_vert_num, yaw_diff, max_yaw_rate, w, weight_type,
// lambda1, lambda2, far, n_path, n_pose; one occupancy log-odds grid (the map's voxel count); per trajectory L, dt, n_ctrl,
// pts[L][3], yaws[L], ctrl[n_ctrl][3]; per pose pt[3], yaw.
#include "facade_driver.h"

#include <active_perception/heading_planner.h>

static void put(const char* tag, size_t b, const std::vector<double>& v) {
  std::printf("%s %zu %zu", tag, b, v.size());
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[19];
  rd(in, hdr, 19);
  ros::NodeHandle nh;
  auto& P = nh.num;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6);
  P["heading_planner/half_vert_num"] = hdr[9], P["heading_planner/yaw_diff"] = hdr[10];
  P["heading_planner/max_yaw_rate"] = hdr[11], P["heading_planner/w"] = hdr[12], P["heading_planner/weight_type"] = hdr[13];
  P["heading_planner/lambda1"] = hdr[14], P["heading_planner/lambda2"] = hdr[15];
  const int n_path = (int)hdr[17], n_pose = (int)hdr[18];
  const DriverMap dm = make_map(nh, true);  // nothing below reads a mirror
  load_occupancy(*dm.map, in, 0);        // the grid alone: the planner reads occupancy, no bound, no inflation
  HeadingPlanner hp(nh);
  hp.setMap(dm.map);
  hp.far_ = hdr[16];
  vector<vector<Eigen::Vector3d>> pts(n_path);
  vector<vector<double>> yaws(n_path);
  vector<double> dts(n_path);
  vector<Eigen::MatrixXd> ctrl(n_path);
  for (int b = 0; b < n_path; ++b) {
    double h3[3];
    if (fread(h3, sizeof(double), 3, in) != 3) return 2;
    const int L = (int)h3[0], nc = (int)h3[2];
    dts[b] = h3[1];
    std::vector<double> buf(4 * (size_t)L + 3 * (size_t)nc);
    if (fread(buf.data(), sizeof(double), buf.size(), in) != buf.size()) return 2;
    for (int i = 0; i < L; ++i) pts[b].push_back(Eigen::Vector3d(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]));
    yaws[b].assign(buf.begin() + 3 * L, buf.begin() + 4 * L);
    ctrl[b] = Eigen::MatrixXd(nc, 3);
    for (int i = 0; i < nc; ++i)
      for (int k = 0; k < 3; ++k) ctrl[b](i, k) = buf[4 * L + 3 * i + k];
  }
  vector<Eigen::Vector3d> poses(n_pose);
  vector<double> pose_yaw(n_pose);
  for (int b = 0; b < n_pose; ++b) {
    double q[4];
    if (fread(q, sizeof(double), 4, in) != 4) return 2;
    poses[b] = Eigen::Vector3d(q[0], q[1], q[2]), pose_yaw[b] = q[3];
  }
  fclose(in);
  for (int b = 0; b < n_path; ++b) {
    vector<double> path;
    hp.searchPathOfYaw(pts[b], yaws[b], dts[b], ctrl[b], path);
    std::printf("call %d %d %d\n", b, hp.last_rc_, hp.last_status_.empty() ? 0 : hp.last_status_[0]);
    put("path", b, path);
    if (!hp.last_gains_.empty()) put("gains", b, hp.last_gains_[0]), put("g_value", b, hp.last_g_value_[0]);
  }
  vector<vector<double>> paths;
  const int rc = hp.searchPathsOfYaw(pts, yaws, dts, ctrl, paths);
  std::printf("batch_call %d\n", rc);
  for (size_t b = 0; b < paths.size(); ++b) put("batch_path", b, paths[b]);
  for (int b = 0; b < n_pose; ++b) put("gain", b, {hp.calcInfoGain(poses[b], pose_yaw[b], 0)});
  vector<double> gains;
  std::printf("batch_gain_call %d\n", hp.calcInfoGains(poses, pose_yaw, gains));
  put("batch_gain", 0, gains);
  return 0;
}
