// facade_yaw.cpp -- drives FrontierFinder::planPathToViewpoint, BsplineOptimizer::planThroughWaypoints and then
// BsplineOptimizer::planYawExplore the way FastExplorationManager::planExploreMotion calls planExploreTraj and
// planYawExplore on the close / far branch (fast_exploration_manager.cpp:244-281), and prints one JSON document that
// tests/test_yaw_plan_gpu.py reads: per problem the branch, the solved position spline and the yaw spline.
//   facade_yaw <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; one occupancy log-odds grid (f64, the map's voxel count);
// then any number of problems, double start[3], goal[3], velocity[3], acceleration[3], start_yaw[3], end_yaw, relax_time.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <plan_env/edt_environment.h>
#include <active_perception/frontier_finder.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>
#include <bspline_opt/bspline_optimizer.h>

namespace fast_planner {
// the package's own ViewNode in a FUEL workspace (graph_node.cpp); here the demo's stand-in: straight flight plus a
// yaw term, the path is its two end points
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
};
}  // namespace fast_planner
using namespace fast_planner;

static void load(SDFMap& map, FILE* in, int N, const double lo[3], const double hi[3]) {
  std::vector<double> occ(N);
  if (fread(occ.data(), sizeof(double), N, in) != (size_t)N) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
  fuelmi_map* m = map.device();
  fuelmi_map_info info;
  fuelmi_map_get_info(m, &info);
  const int b0[3] = {0, 0, 0};
  const int b1[3] = {info.voxel_num[0] - 1, info.voxel_num[1] - 1, info.voxel_num[2] - 1};
  if (fuelmi_map_upload_occupancy(m, occ.data()) || fuelmi_map_set_local_bound(m, b0, b1)) std::exit(3);
  MapROS::inflate(map);
  map.updateESDF3d();
  fuelmi_map_set_updated_box(m, lo, hi);
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[9];
  if (fread(hdr, sizeof(double), 9, in) != 9) return 2;
  ros::NodeHandle nh;
  auto& P = nh.num;
  P["sdf_map/resolution"] = 0.1;
  P["sdf_map/map_size_x"] = hdr[0], P["sdf_map/map_size_y"] = hdr[1], P["sdf_map/map_size_z"] = hdr[2];
  P["sdf_map/obstacles_inflation"] = 0.199, P["sdf_map/local_bound_inflate"] = 0.5, P["sdf_map/ground_height"] = -1.0;
  P["sdf_map/default_dist"] = 0.0, P["sdf_map/optimistic"] = 0, P["sdf_map/signed_dist"] = 0;
  P["sdf_map/p_hit"] = 0.65, P["sdf_map/p_miss"] = 0.35, P["sdf_map/p_min"] = 0.12, P["sdf_map/p_max"] = 0.90;
  P["sdf_map/p_occ"] = 0.80, P["sdf_map/max_ray_length"] = 4.5, P["sdf_map/virtual_ceil_height"] = -10;
  const char* ax[3] = {"x", "y", "z"};
  for (int i = 0; i < 3; ++i) {
    P[std::string("sdf_map/box_min_") + ax[i]] = hdr[3 + i];
    P[std::string("sdf_map/box_max_") + ax[i]] = hdr[6 + i];
  }
  P["frontier/cluster_min"] = 10;
  P["frontier/cluster_size_xy"] = 1.0;
  P["frontier/down_sample"] = 3;
  P["frontier/candidate_rmin"] = 1.5;
  P["frontier/candidate_rmax"] = 2.5;
  P["frontier/candidate_rnum"] = 3;
  P["frontier/candidate_dphi"] = 15 * 3.1415926 / 180.0;
  P["frontier/min_candidate_clearance"] = 0.21;
  P["frontier/min_visib_num"] = 3;
  P["frontier/min_candidate_dist"] = 0.75;
  P["frontier/min_view_finish_fraction"] = 0.2;
  P["perception_utils/top_angle"] = 0.56125;
  P["perception_utils/left_angle"] = 0.69222;
  P["perception_utils/right_angle"] = 0.68901;
  P["perception_utils/max_dist"] = 4.5;
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  fuelmi_map_info info;
  fuelmi_map_get_info(map->device(), &info);
  const int N = info.voxel_num[0] * info.voxel_num[1] * info.voxel_num[2];
  FrontierFinder ff(edt, nh);
  load(*map, in, N, hdr + 3, hdr + 6);
  // exploration_manager/launch/algorithm.xml:170-194, without the wall-clock cap (a result must not depend on the clock)
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
  std::vector<double> pr;
  double rec[17];
  while (fread(rec, sizeof(double), 17, in) == 17) pr.insert(pr.end(), rec, rec + 17);
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
