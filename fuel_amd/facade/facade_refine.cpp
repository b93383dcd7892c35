// facade_refine.cpp -- drives FrontierFinder::refineLocalTour / refineSingleDestination as FastExplorationManager
// does (fast_exploration_manager.cpp:134-158, 185-220) after one frontier search and prints what
// tests/test_refine_gpu.py compares: the layers getViewpointsInfo built, the refined choices and tour, and the
// single-destination pick.
//   facade_refine <scenario.bin> <with_params 0|1>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; then one occupancy log-odds grid (f64, the map's voxel
// count).  Without the exploration/* parameters the refinement refuses (prints "refine 0").
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
  fuelmi_map_set_updated_box(m, lo, hi);
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
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
  if (atoi(argv[2])) {  // the ViewNode parameters (algorithm.xml:95-99)
    P["exploration/vm"] = 2.0;
    P["exploration/yd"] = 60 * 3.1415926 / 180.0;
    P["exploration/w_dir"] = 1.5;
  }
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  fuelmi_map_info info;
  fuelmi_map_get_info(map->device(), &info);
  const int N = info.voxel_num[0] * info.voxel_num[1] * info.voxel_num[2];
  FrontierFinder ff(edt, nh);
  load(*map, in, N, hdr + 3, hdr + 6);
  fclose(in);
  ff.searchFrontiers();
  ff.computeFrontiersToVisit();
  std::vector<std::vector<Eigen::Vector3d>> act;
  ff.getFrontiers(act);
  const int n = (int)act.size();
  // exploration/refined_num 7, top_view_num 15, max_decay 0.8 (algorithm.xml:91-94); the tour order: list order
  std::vector<int> ids;
  for (int i = 0; i < n && i < 7; ++i) ids.push_back(i);
  const Eigen::Vector3d cur(hdr[3] + 1.5, 0.1, 1.0), vel(0.5, -0.3, 0.1), cur_yaw(0.3, 0.2, 0.0);
  std::printf("clusters %d\n", n);
  std::printf("cur %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", cur(0), cur(1), cur(2), vel(0), vel(1), vel(2),
              cur_yaw(0));
  std::vector<std::vector<Eigen::Vector3d>> n_points;
  std::vector<std::vector<double>> n_yaws;
  ff.getViewpointsInfo(cur, ids, 15, 0.8, n_points, n_yaws);
  for (size_t i = 0; i < n_points.size(); ++i) {
    std::printf("layer %zu", i);
    for (size_t j = 0; j < n_points[i].size(); ++j)
      std::printf(" %.17g %.17g %.17g %.17g", n_points[i][j](0), n_points[i][j](1), n_points[i][j](2), n_yaws[i][j]);
    std::printf("\n");
  }
  std::vector<Eigen::Vector3d> pts, tour;
  std::vector<double> yaws;
  const bool ok = ff.refineLocalTour(cur, vel, cur_yaw, n_points, n_yaws, pts, yaws, &tour);
  std::printf("refine %d\n", (int)ok);
  if (!ok) return 0;
  for (size_t i = 0; i < pts.size(); ++i)
    std::printf("refined %.17g %.17g %.17g %.17g\n", pts[i](0), pts[i](1), pts[i](2), yaws[i]);
  for (auto& q : tour) std::printf("pt %.17g %.17g %.17g\n", q(0), q(1), q(2));
  // the single-destination branch on the first cluster (:193-208)
  std::vector<std::vector<Eigen::Vector3d>> p0;
  std::vector<std::vector<double>> y0;
  ff.getViewpointsInfo(cur, {0}, 15, 0.8, p0, y0);
  int id = -1;
  const bool ok1 = ff.refineSingleDestination(cur, vel, cur_yaw, p0[0], y0[0], id);
  std::printf("single %d %d\n", (int)ok1, id);
  return 0;
}
