// facade_tsp.cpp -- drives the global tour as FastExplorationManager::findGlobalTour does
// (fast_exploration_manager.cpp:327-420), both ways, and prints what tests/test_tsp_gpu.py compares:
//   facade_tsp <scenario.bin> <tsp_dir>
//     one full-box frontier search and viewpoint sampling on the scenario's map (frontier/device_path_cost = true),
//     then FrontierFinder::findGlobalTour ("indices", "tour_points"), the full cost matrix ("row"), and the drop-in
//     route: single.par / single.tsp written into tsp_dir in the reference's format, solveTSPLKH (libfuelmi_lkh.so),
//     single.txt read back as the reference reads it ("lkh_rc", "lkh").
//   facade_tsp --malformed <tsp_dir>
//     a stale single.txt, a problem file with a TSP type, solveTSPLKH: "lkh_rc" and whether a tour file is left.
// scenario.bin: double map_size[3], box_min[3], box_max[3]; then the occupancy log-odds grid (f64, the map's voxels).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include <plan_env/sdf_map.h>
#include <plan_env/edt_environment.h>
#include <active_perception/frontier_finder.h>
#include <active_perception/graph_node.h>
#include <active_perception/perception_utils.h>
#include <lkh_tsp_solver/lkh_interface.h>

namespace fast_planner {
// the package's own ViewNode is not used with frontier/device_path_cost (the driver's stand-ins are never reached)
double ViewNode::computeCost(const Eigen::Vector3d& p1, const Eigen::Vector3d& p2, const double&, const double&,
                             const Eigen::Vector3d&, const double&, std::vector<Eigen::Vector3d>& path) {
  path = {p1, p2};
  return (p2 - p1).norm();
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

// the parameter and problem files in the format findGlobalTour writes (:342-376), the tour back as it reads it
// (:381-410): lines after TOUR_SECTION, node 1 skipped, up to -1, id - 2
static void write_files(const std::string& dir, const Eigen::MatrixXd& m) {
  std::ofstream par(dir + "/single.par");
  par << "PROBLEM_FILE = " << dir << "/single.tsp\nGAIN23 = NO\nOUTPUT_TOUR_FILE = " << dir << "/single.txt\nRUNS = 1\n";
  std::ofstream tsp(dir + "/single.tsp");
  tsp << "NAME : single\nTYPE : ATSP\nDIMENSION : " << m.rows()
      << "\nEDGE_WEIGHT_TYPE : EXPLICIT\nEDGE_WEIGHT_FORMAT : FULL_MATRIX\nEDGE_WEIGHT_SECTION\n";
  for (int i = 0; i < m.rows(); ++i) {
    for (int j = 0; j < m.cols(); ++j) tsp << (int)(m(i, j) * 100) << " ";
    tsp << "\n";
  }
  tsp << "EOF";
}

static std::vector<int> read_tour(const std::string& path) {
  std::ifstream in(path);
  std::string line;
  std::vector<int> ids;
  while (std::getline(in, line))
    if (line == "TOUR_SECTION") break;
  while (std::getline(in, line)) {
    const int id = std::stoi(line);
    if (id == 1) continue;
    if (id == -1) break;
    ids.push_back(id - 2);
  }
  return ids;
}

static bool exists(const std::string& path) {
  std::ifstream f(path);
  return f.good();
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  if (std::string(argv[1]) == "--malformed") {
    const std::string dir = argv[2];
    std::ofstream(dir + "/single.txt") << "NAME : stale\nTYPE : TOUR\nDIMENSION : 3\nTOUR_SECTION\n1\n3\n2\n-1\nEOF\n";
    std::ofstream(dir + "/single.par") << "problem_file = " << dir << "/single.tsp\nOUTPUT_TOUR_FILE = " << dir
                                       << "/single.txt\n";
    std::ofstream(dir + "/single.tsp") << "NAME : single\nTYPE : TSP\nDIMENSION : 3\nEDGE_WEIGHT_TYPE : EXPLICIT\n"
                                          "EDGE_WEIGHT_FORMAT : FULL_MATRIX\nEDGE_WEIGHT_SECTION\n0 1 2 \n1 0 3 \n2 3 0 \nEOF";
    const int rc = solveTSPLKH((dir + "/single.par").c_str());
    std::printf("lkh_rc %d\ntour_file %d\n", rc, (int)exists(dir + "/single.txt"));
    return 0;
  }
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::string dir = argv[2];
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
  P["frontier/cluster_min"] = 100;
  P["frontier/cluster_size_xy"] = 2.0;
  P["frontier/down_sample"] = 3;
  P["frontier/candidate_rmin"] = 1.5;
  P["frontier/candidate_rmax"] = 2.5;
  P["frontier/candidate_rnum"] = 3;
  P["frontier/candidate_dphi"] = 15 * 3.1415926 / 180.0;
  P["frontier/min_candidate_clearance"] = 0.21;
  P["frontier/min_visib_num"] = 15;
  P["frontier/min_candidate_dist"] = 0.75;
  P["frontier/min_view_finish_fraction"] = 0.2;
  P["perception_utils/top_angle"] = 0.56125;
  P["perception_utils/left_angle"] = 0.69222;
  P["perception_utils/right_angle"] = 0.68901;
  P["perception_utils/max_dist"] = 4.5;
  P["frontier/device_path_cost"] = 1;
  P["exploration/vm"] = 2.0;
  P["exploration/yd"] = 60 * 3.1415926 / 180.0;
  P["exploration/w_dir"] = 1.5;
  SDFMap::Ptr map(new SDFMap);
  map->initMap(nh);
  EDTEnvironment::Ptr edt(new EDTEnvironment);
  edt->setMap(map);
  fuelmi_map* m = map->device();
  fuelmi_map_info info;
  fuelmi_map_get_info(m, &info);
  const int N = info.voxel_num[0] * info.voxel_num[1] * info.voxel_num[2];
  std::vector<double> occ(N);
  if (fread(occ.data(), sizeof(double), N, in) != (size_t)N) return 2;
  fclose(in);
  const int b0[3] = {0, 0, 0};
  const int b1[3] = {info.voxel_num[0] - 1, info.voxel_num[1] - 1, info.voxel_num[2] - 1};
  if (fuelmi_map_upload_occupancy(m, occ.data()) || fuelmi_map_set_local_bound(m, b0, b1)) return 3;
  MapROS::inflate(*map);
  fuelmi_map_set_updated_box(m, hdr + 3, hdr + 6);
  FrontierFinder ff(edt, nh);
  ff.searchFrontiers();
  ff.computeFrontiersToVisit();
  std::vector<std::vector<Eigen::Vector3d>> act;
  ff.getFrontiers(act);
  const int n = (int)act.size();
  std::vector<int> ids(n);
  for (int i = 0; i < n; ++i) ids[i] = i;
  std::vector<std::vector<Eigen::Vector3d>> vp;
  std::vector<std::vector<double>> vy;
  ff.getViewpointsInfo(Eigen::Vector3d(1e6, 1e6, 1e6), ids, 1, 0.0, vp, vy);
  const Eigen::Vector3d cur = vp[0][0] + Eigen::Vector3d(0.3, -0.2, 0.0), vel(0.5, -0.3, 0.1), cur_yaw(0.3, 0.2, 0.0);
  std::vector<int> indices;
  std::vector<Eigen::Vector3d> tour;
  if (!ff.findGlobalTour(cur, vel, cur_yaw, indices, &tour)) return 4;
  std::printf("clusters %d\nindices", n);
  for (int k : indices) std::printf(" %d", k);
  std::printf("\ntour_points %zu\n", tour.size());
  Eigen::MatrixXd mat;
  ff.getFullCostMatrix(cur, vel, cur_yaw, mat);  // the matrix findGlobalTour solved (the cost matrix is up to date)
  for (int i = 0; i < mat.rows(); ++i) {
    std::printf("row");
    for (int j = 0; j < mat.cols(); ++j) std::printf(" %.17g", mat(i, j));
    std::printf("\n");
  }
  write_files(dir, mat);
  const int rc = solveTSPLKH((dir + "/single.par").c_str());
  std::printf("lkh_rc %d\nlkh", rc);
  for (int k : read_tour(dir + "/single.txt")) std::printf(" %d", k);
  std::printf("\n");
  return 0;
}
