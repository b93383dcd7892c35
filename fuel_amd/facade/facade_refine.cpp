// facade_refine.cpp -- drives FrontierFinder::refineLocalTour / refineSingleDestination as FastExplorationManager
// does (fast_exploration_manager.cpp:134-158, 185-220) after one frontier search and prints what
// tests/test_refine_gpu.py compares: the layers getViewpointsInfo built, the refined choices and tour, and the
// single-destination pick.
//   facade_refine <scenario.bin> <with_params 0|1>
// scenario.bin: double map_size[3], box_min[3], box_max[3]; then one occupancy log-odds grid (f64, the map's voxel
// count).  Without the exploration/* parameters the refinement refuses (prints "refine 0").
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
  if (atoi(argv[2])) exploration_params(nh);  // the ViewNode parameters
  const DriverMap dm = make_map(nh, false);
  FrontierFinder ff(dm.edt, nh);
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE, hdr + 3, hdr + 6);
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
