// facade_pathcost.cpp -- drives the facade's tour-planning group as FastExplorationManager does
// (fast_exploration_manager.cpp:97-118, 187, 334-335, 423) over two rounds of frontier search and prints what
// tests/test_path_cost_gpu.py compares: the best viewpoint of every active cluster, the full cost matrix and the
// path along a tour.
//   facade_pathcost <scenario.bin> <device_path_cost 0|1>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; then two occupancy log-odds grids (f64, the map's voxel
// count each), the state before the first and before the second search.
#include "facade_driver.h"

#include <active_perception/frontier_finder.h>

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  double hdr[9];
  rd(in, hdr, 9);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6);
  frontier_params(nh, 10, 1.0, 3);
  if (atoi(argv[2])) {  // the opt-in and the ViewNode parameters it needs
    nh.num["frontier/device_path_cost"] = 1;
    exploration_params(nh);
  }
  const DriverMap dm = make_map(nh, false);
  const SDFMap::Ptr& map = dm.map;
  FrontierFinder ff(dm.edt, nh);
  const int steps = LOAD_BOUND | LOAD_INFLATE;
  // round 1: every cluster new, all links new x new
  load_occupancy(*map, in, steps, hdr + 3, hdr + 6);
  ff.searchFrontiers();
  ff.computeFrontiersToVisit();
  ff.updateFrontierCostMatrix();
  std::vector<std::vector<Eigen::Vector3d>> act;
  ff.getFrontiers(act);
  const int n1 = (int)act.size();
  // round 2: more of the map known; survivors keep their entries, new clusters are linked to them (old x new)
  load_occupancy(*map, in, steps, hdr + 3, hdr + 6);
  fclose(in);
  ff.searchFrontiers();
  const int n_removed = (int)ff.removedIds().size();
  ff.computeFrontiersToVisit();
  ff.updateFrontierCostMatrix();
  ff.getFrontiers(act);
  const int n = (int)act.size();
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  std::vector<std::vector<Eigen::Vector3d>> vp;
  std::vector<std::vector<double>> vy;
  ff.getViewpointsInfo(Eigen::Vector3d(1e6, 1e6, 1e6), ids, 1, 0.0, vp, vy);  // the best viewpoint of each
  std::printf("clusters %d %d %d\n", n1, n_removed, n);
  for (int i = 0; i < n; ++i) std::printf("vp %.17g %.17g %.17g %.17g\n", vp[i][0](0), vp[i][0](1), vp[i][0](2), vy[i][0]);
  const Eigen::Vector3d cur(hdr[3] + 1.5, 0.1, 1.0), vel(0.5, -0.3, 0.1), cur_yaw(0.3, 0.2, 0.0);
  std::printf("cur %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", cur(0), cur(1), cur(2), vel(0), vel(1), vel(2),
              cur_yaw(0), cur_yaw(1));
  Eigen::MatrixXd mat;
  ff.getFullCostMatrix(cur, vel, cur_yaw, mat);
  for (int i = 0; i < mat.rows(); ++i) {
    std::printf("row");
    for (int j = 0; j < mat.cols(); ++j) std::printf(" %.17g", mat(i, j));
    std::printf("\n");
  }
  std::vector<int> tour;
  for (int k = 0; k < n && k < 5; ++k) tour.push_back((k * 3 + n - 1) % n);
  std::vector<Eigen::Vector3d> tpath;
  ff.getPathForTour(cur, tour, tpath);
  std::printf("tour");
  for (int t : tour) std::printf(" %d", t);
  std::printf("\n");
  for (auto& q : tpath) std::printf("pt %.17g %.17g %.17g\n", q(0), q(1), q(2));
  return 0;
}
