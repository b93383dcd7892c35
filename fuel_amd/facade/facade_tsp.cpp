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
#include "facade_driver.h"

#include <fstream>
#include <sstream>

#include <active_perception/frontier_finder.h>
#include <lkh_tsp_solver/lkh_interface.h>

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
  rd(in, hdr, 9);
  ros::NodeHandle nh;
  sdf_map_params(nh, hdr, hdr + 3, hdr + 6);
  frontier_params(nh, 100, 2.0, 15);  // the launch file's own cluster sizes
  nh.num["frontier/device_path_cost"] = 1;  // (the stand-in ViewNode is never reached)
  exploration_params(nh);
  const DriverMap dm = make_map(nh, false);
  load_occupancy(*dm.map, in, LOAD_BOUND | LOAD_INFLATE, hdr + 3, hdr + 6);
  fclose(in);
  FrontierFinder ff(dm.edt, nh);
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
