// facade_kino.cpp -- drives FrontierFinder::planPathToViewpoint and then, on the MID branch, BsplineOptimizer::planKinodynamic
// the way FastExplorationManager::planExploreMotion calls kinodynamicReplan there (fast_exploration_manager.cpp:264-270,
// plan_manage/src/planner_manager.cpp:124-185); the close / far branches take planThroughWaypoints as in facade_wptraj.
// Prints what tests/test_kino_path_gpu.py compares: the branch, the search's status and counters, the spline handed to
// the solve, the solved spline and its cost.
//   facade_kino <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; one occupancy log-odds grid (f64, the map's voxel count);
// then any number of problems, double start[3], goal[3], velocity[3], acceleration[3] each.
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
  double rec[12];
  while (fread(rec, sizeof(double), 12, in) == 12) pr.insert(pr.end(), rec, rec + 12);
  fclose(in);
  // exploration_manager/launch/algorithm.xml:149-162 (max_vel includes vel_margin); a pool of 4096 nodes
  fuelmi_kino_cfg kc = {0.8, 1.0, 2.25, 2.0, 10.0, 5.0, 0.1, 10.0, 1 / 2.0, 1 / 1.0, 1 / 20.0, 0.45 / 2.0, 4096, 10, 0, 8, 0, 1, 256};
  for (size_t b = 0; b < pr.size() / 12; ++b) {
    const double* q = pr.data() + 12 * b;
    const Eigen::Vector3d pos(q[0], q[1], q[2]), next_pos(q[3], q[4], q[5]), vel(q[6], q[7], q[8]), acc(q[9], q[10], q[11]);
    std::vector<Eigen::Vector3d> path_next_goal;
    Eigen::Vector3d next_goal(0, 0, 0);
    const int branch = ff.planPathToViewpoint(pos, next_pos, path_next_goal, next_goal);
    std::printf("goal %zu %d %zu %.17g %.17g %.17g\n", b, branch, path_next_goal.size(), next_goal(0), next_goal(1),
                next_goal(2));
    if (branch != FUELMI_GOAL_CLOSE && branch != FUELMI_GOAL_FAR && branch != FUELMI_GOAL_MID) continue;
    Eigen::MatrixXd ctrl_pts;
    double dt = 0.0;
    const int cost_mask = BsplineOptimizer::NORMAL_PHASE | BsplineOptimizer::MINTIME;
    if (branch == FUELMI_GOAL_MID) {  // :264-270: kinodynamicReplan(pos, vel, acc, next_pos, Vector3d(0, 0, 0), time_lb)
      const int status = opt.planKinodynamic(pos, vel, acc, next_goal, Eigen::Vector3d(0, 0, 0), kc, 2.0, 0.45, cost_mask,
                                             -1.0, ctrl_pts, dt);
      std::printf("kino %zu %d %d %d %d %d %.17g %.17g %.17g\n", b, status, opt.kino_which_, opt.kino_iter_num_,
                  opt.kino_use_node_num_, (int)ctrl_pts.rows(), opt.init_knot_span_, dt, opt.final_cost_);
      if (status != FUELMI_KINO_REACH_HORIZON && status != FUELMI_KINO_REACH_END && status != FUELMI_KINO_NEAR_END) continue;
    } else {
      const int status = opt.planThroughWaypoints(path_next_goal, vel, acc, 2.0, 0.45, cost_mask, -1.0, ctrl_pts, dt);
      std::printf("traj %zu %d %d %.17g %.17g %.17g\n", b, status, (int)ctrl_pts.rows(), opt.init_knot_span_, dt,
                  opt.final_cost_);
      if (status != FUELMI_WPTRAJ_OK) continue;
    }
    for (int i = 0; i < opt.init_ctrl_pts_.rows(); ++i)
      std::printf("init %zu %.17g %.17g %.17g\n", b, opt.init_ctrl_pts_(i, 0), opt.init_ctrl_pts_(i, 1), opt.init_ctrl_pts_(i, 2));
    for (int i = 0; i < ctrl_pts.rows(); ++i)
      std::printf("ctrl %zu %.17g %.17g %.17g\n", b, ctrl_pts(i, 0), ctrl_pts(i, 1), ctrl_pts(i, 2));
  }
  return 0;
}
