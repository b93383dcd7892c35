// facade_goalpath.cpp -- drives FrontierFinder::planPathToViewpoint where FastExplorationManager::planExploreMotion
// searches and shortens the path to the next viewpoint (fast_exploration_manager.cpp:234-276) and prints what
// tests/test_goal_path_gpu.py compares: per problem the branch, next_goal and the way-points.
//   facade_goalpath <scenario.bin>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; one occupancy log-odds grid (f64, the map's voxel count);
// then any number of problems, double start[3], goal[3] each.
#include "facade_driver.h"

#include <active_perception/frontier_finder.h>

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[9];
  rd(in, hdr, 9);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6);
  frontier_params(nh, 10, 1.0, 3);
  const DriverMap dm = make_map(nh, false);
  FrontierFinder ff(dm.edt, nh);
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE, hdr + 3, hdr + 6);
  const std::vector<double> pr = read_records(in, 6);
  fclose(in);
  for (size_t b = 0; b < pr.size() / 6; ++b) {
    const Eigen::Vector3d pos(pr[6 * b], pr[6 * b + 1], pr[6 * b + 2]), next_pos(pr[6 * b + 3], pr[6 * b + 4], pr[6 * b + 5]);
    std::vector<Eigen::Vector3d> path_next_goal;
    Eigen::Vector3d next_goal(0, 0, 0);
    const int branch = ff.planPathToViewpoint(pos, next_pos, path_next_goal, next_goal);
    std::printf("goal %zu %d %zu %.17g %.17g %.17g\n", b, branch, path_next_goal.size(), next_goal(0), next_goal(1),
                next_goal(2));
    for (auto& q : path_next_goal) std::printf("way %zu %.17g %.17g %.17g\n", b, q(0), q(1), q(2));
  }
  return 0;
}
